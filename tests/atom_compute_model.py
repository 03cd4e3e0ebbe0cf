"""A NumPy restatement of the per-atom computes: stress/atom, contact/atom, ke/atom and
erotate/sphere/atom from a state, a history and the pair parameters.

It does its own pair search -- every ordered pair (i, j), the partner moved to each periodic image (x_j + shift first, then the
difference: the sum a ghost atom holds), touching where rsq < (radi + radj)^2 -- and takes the contact law from
tests/contact_model.py (`pair_law`, the reference's plain IEEE algebra, shearupdate = false).  Atom i keeps the half share
of every pair force on it,
    W_ab(i) = sum_j 1/2 del_a F_b,   del = x_i - x_j,   F = del ccel + fs  (the force on i from j),
which is ev_tally_xyz under newton off, and
    stress/atom = -( [ke] m v_a v_b + [pair] W_ab )   in the order xx yy zz xy xz yz."""
import itertools

import numpy as np

from tests import contact_model as cm

PAIRS6 = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def touching_pairs(boxlo, boxhi, periodic, x, radius):
    """every ordered touching pair: (I, J, D = x_I - image of x_J, wrapped)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    prd = np.asarray(boxhi, dtype=np.float64) - np.asarray(boxlo, dtype=np.float64)
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    I, J, D, W = [], [], [], []
    for s in itertools.product(*[((-1, 0, 1) if periodic[k] else (0,)) for k in range(3)]):
        xj = x[jj] + np.asarray(s, dtype=np.float64) * prd
        d = x[ii] - xj
        rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        radsum = radius[ii] + radius[jj]
        hit = rsq < radsum * radsum
        I.append(ii[hit]); J.append(jj[hit]); D.append(d[hit]); W.append(np.full(int(hit.sum()), any(s)))
    return np.concatenate(I), np.concatenate(J), np.concatenate(D), np.concatenate(W)


def per_atom(boxlo, boxhi, periodic, tag, x, radius, mass, v, omega, history, pair, frozen=None):
    """dict of per-atom arrays in the order of `tag`: virial[n, 6] (W, the pair part, before the sign), kin[n, 6]
    (m v_a v_b), contacts[n], ke[n], erotate[n]; and per ordered pair I, J, D, F, capped, wrapped.
    history: {(tag_lo, tag_hi): shear[3]} as the lower tag's side holds it (the other side sees it negated)"""
    tag = np.asarray(tag)
    x, v, omega = (np.asarray(a, dtype=np.float64) for a in (x, v, omega))
    n = len(tag)
    frozen = np.zeros(n, bool) if frozen is None else np.asarray(frozen, bool)
    I, J, D, wrapped = touching_pairs(boxlo, boxhi, periodic, x, radius)
    sh = np.zeros((len(I), 3))
    for k, (a, b) in enumerate(zip(tag[I].tolist(), tag[J].tolist())):
        h = history.get((min(a, b), max(a, b)))
        if h is not None:
            sh[k] = h if a < b else -np.asarray(h)
    vr = v[I] - v[J]
    wsum = radius[I][:, None] * omega[I] + radius[J][:, None] * omega[J]
    r, ccel, fs, capped = cm.pair_law(pair, D, vr, wsum, radius[I], radius[J], mass[I], mass[J], frozen[I], frozen[J], sh)
    F = D * ccel[:, None] + fs
    W = np.zeros((n, 6))
    for c, (a, b) in enumerate(PAIRS6):
        np.add.at(W[:, c], I, 0.5 * D[:, a] * F[:, b])
    kin = np.stack([mass * v[:, a] * v[:, b] for a, b in PAIRS6], axis=1)
    return dict(virial=W, kin=kin, contacts=np.bincount(I, minlength=n), ke=0.5 * mass * np.sum(v * v, axis=1),
                erotate=0.5 * (0.4 * mass * radius * radius) * np.sum(omega * omega, axis=1),
                I=I, J=J, D=D, F=F, capped=capped, wrapped=wrapped)


def stress(m, ke=True, pair=True, group=None):
    """stress/atom from per_atom()'s dict: -( [ke] kin + [pair] virial ), 0 outside the group"""
    s = -((m["kin"] if ke else 0.0) + (m["virial"] if pair else 0.0)) + np.zeros_like(m["kin"])
    if group is not None:
        s = np.where(np.asarray(group, bool)[:, None], s, 0.0)
    return s


def column_errors(got, want):
    """per column: max |got - want| over the bed against the largest magnitude of the same column of `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.ndim == 1:
        got, want = got[:, None], want[:, None]
    scale = np.max(np.abs(want), axis=0)
    return np.max(np.abs(got - want), axis=0) / np.where(scale > 0, scale, 1.0)


GATE = cm.GATE        # one force evaluation, per atom: 1e-12 against the column's largest magnitude
SUM_GATE = 1e-10      # a tensor summed over the bed, against its largest component (tests/test_thermo_gpu.py)
