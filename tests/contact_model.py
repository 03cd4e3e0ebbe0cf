"""A NumPy restatement of what a row of `compute pair/local` is: plain IEEE algebra written the way
the reference writes its pair laws (pair_gran_hertzFix_history.cpp:142-261 and the [3P] Hookean twins, as oracle/orc_contact.c
restates them), not the fast-math arrangement of csrc/sf_physics.h.

A row is one touching pair (rsq < (radi + radj)^2) of two atoms of the group, written once: tag1 the lower tag, del =
x(tag1) - x(tag2) with the partner moved to the periodic image that touches (x(tag2) + shift first, then the difference: the
sum a ghost atom of the reference holds), forces on tag1, evaluated from the state given with shearupdate = false:
    dist = r   force = r ccel   f = del ccel   fs = the tangential force   fsmag = |fs|
so that f + fs is the pair force the contact law gives tag1."""
import itertools

import numpy as np

PI = 3.14159265358979323846   # MathConst::MY_PI


def pair_params(style, kn, kt, gamman, gammat, xmu, dampflag=1):
    """the settings of pair_style gran/* (pair_gran_hertzFix_history.cpp:295-316): style 'hooke' (gran/hooke/history),
    'hertz' (gran/hertzFix/history), 'hooke_plain' (gran/hooke); kt / gammat None = NULL"""
    kt = kn * 2.0 / 7.0 if kt is None else kt
    gammat = 0.5 * gamman if gammat is None else gammat
    if dampflag == 0:
        gammat = 0.0
    return dict(style=style, kn=kn, kt=kt, gamman=gamman, gammat=gammat, xmu=xmu)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross_del_wr(d, w):
    return np.stack([d[:, 2] * w[:, 1] - d[:, 1] * w[:, 2], d[:, 0] * w[:, 2] - d[:, 2] * w[:, 0],
                     d[:, 1] * w[:, 0] - d[:, 0] * w[:, 1]], axis=1)


def pair_law(p, d, vr, wsum, radi, radj, mi, mj, frozen_i, frozen_j, sh):
    """the contact law on arrays of pairs, shearupdate = 0: (r, ccel, fs[n, 3], capped[n])"""
    rsq = _dot(d, d)
    r = np.sqrt(rsq)
    rinv = 1.0 / r
    rsqinv = 1.0 / rsq
    radsum = radi + radj
    vnnr = _dot(vr, d)
    vn = np.stack([d[:, k] * vnnr * rsqinv for k in range(3)], axis=1)
    vt = vr - vn
    wr = wsum * rinv[:, None]
    meff = mi * mj / (mi + mj)
    meff = np.where(frozen_i, mj, meff)   # pair_gran_hertzFix_history.cpp:188-189
    meff = np.where(frozen_j, mi, meff)
    vtr = vt - _cross_del_wr(d, wr)
    kn, kt, xmu = p["kn"], p["kt"], p["xmu"]
    if p["style"] == "hertz":
        polyhertz = np.sqrt((radsum - r) * radi * radj / radsum)
        sn = 2.0 * 1.0 / 1.82 * kn * polyhertz
        st = 8.0 * 1.0 / 8.84 * kn * polyhertz
        lg = np.log(p["gamman"]) / np.log(np.exp(1.0))
        beta = -(lg) / np.sqrt(lg * lg + PI * PI)
        damp = 2.0 * np.sqrt(5.0 / 6.0) * beta * vnnr * rsqinv
        ccel = polyhertz * 4.0 / 5.46 * kn * (radsum - r) * rinv - np.sqrt(sn * meff) * damp
        sdamp = np.sqrt(st * meff) * 2.0 * np.sqrt(5.0 / 6.0) * beta
        fs = -(polyhertz * 8.0 / 8.84 * kt)[:, None] * sh - sdamp[:, None] * vtr
    else:
        damp = meff * p["gamman"] * vnnr * rsqinv
        ccel = kn * (radsum - r) * rinv - damp
        fs = -(kt * sh + (meff * p["gammat"])[:, None] * vtr)
    fn = xmu * np.abs(ccel * r)
    if p["style"] == "hooke_plain":
        vrel = np.sqrt(_dot(vtr, vtr))
        fsd = meff * p["gammat"] * vrel
        with np.errstate(invalid="ignore", divide="ignore"):
            ft = np.where(vrel != 0.0, np.minimum(fn, fsd) / vrel, 0.0)
        fs = -ft[:, None] * vtr
        capped = (vrel != 0.0) & (fn < fsd)
    else:
        shrmag = np.sqrt(_dot(sh, sh))
        fsmag = np.sqrt(_dot(fs, fs))
        capped = fsmag > fn
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = np.where(capped, np.where(shrmag != 0.0, fn / fsmag, 0.0), 1.0)
        fs = np.where(capped[:, None], fs * scale[:, None], fs)
    return r, ccel, fs, capped


def contact_rows(boxlo, boxhi, periodic, tag, x, radius, mass, v, omega, history, pair, frozen=None, group=None):
    """rows sorted by (tag1, tag2): dict of tag1 tag2 dist force f[n, 3] fs[n, 3] fsmag, plus `capped` (the Coulomb cap
    acted) and `wrapped` (the partner is a periodic image).  history: {(tag_lo, tag_hi): shear[3]} as the lower tag's side
    holds it; pairs it does not name have zero history.  frozen / group: boolean masks per atom"""
    tag = np.asarray(tag)
    x = np.asarray(x, dtype=np.float64)
    n = len(tag)
    frozen = np.zeros(n, bool) if frozen is None else np.asarray(frozen, bool)
    group = np.ones(n, bool) if group is None else np.asarray(group, bool)
    prd = np.asarray(boxhi, dtype=np.float64) - np.asarray(boxlo, dtype=np.float64)
    ii, jj = np.nonzero((tag[:, None] < tag[None, :]) & group[:, None] & group[None, :])
    shifts = itertools.product(*[((-1, 0, 1) if periodic[k] else (0,)) for k in range(3)])
    I, J, D, W = [], [], [], []
    for s in shifts:
        xj = x[jj] + np.asarray(s, dtype=np.float64) * prd   # (what a ghost atom holds)
        d = x[ii] - xj
        rsq = _dot(d, d)
        radsum = radius[ii] + radius[jj]
        hit = rsq < radsum * radsum
        I.append(ii[hit]); J.append(jj[hit]); D.append(d[hit]); W.append(np.full(int(hit.sum()), any(s)))
    I, J, D, W = np.concatenate(I), np.concatenate(J), np.concatenate(D), np.concatenate(W)
    o = np.lexsort((tag[J], tag[I]))
    I, J, D, W = I[o], J[o], D[o], W[o]
    sh = np.array([history.get((int(tag[a]), int(tag[b])), np.zeros(3)) for a, b in zip(I, J)]).reshape(-1, 3)
    vr = v[I] - v[J]
    wsum = radius[I][:, None] * omega[I] + radius[J][:, None] * omega[J]
    r, ccel, fs, capped = pair_law(pair, D, vr, wsum, radius[I], radius[J], mass[I], mass[J], frozen[I], frozen[J], sh)
    return dict(tag1=tag[I].astype(np.int32), tag2=tag[J].astype(np.int32), dist=r, force=r * ccel, f=D * ccel[:, None],
                fs=fs, fsmag=np.sqrt(_dot(fs, fs)), capped=capped, wrapped=W)


def per_atom_sums(rows, tag):
    """the rows summed per atom: + (f + fs) for tag1, - for tag2; in the order of `tag`"""
    pos = {int(t): k for k, t in enumerate(tag)}
    out = np.zeros((len(tag), 3))
    tot = rows["f"] + rows["fs"]
    for a, b, F in zip(rows["tag1"], rows["tag2"], tot):
        out[pos[int(a)]] += F
        out[pos[int(b)]] -= F
    return out


GATE = 1e-12   # the project's gate for one force evaluation (tests/test_dem_gpu.py)


def columns(rows):
    """the nine double columns of a row by their script names"""
    c = dict(dist=rows["dist"], force=rows["force"], p4=rows["fsmag"])
    for k in range(3):
        c["fx fy fz".split()[k]] = rows["f"][:, k]
        c["p1 p2 p3".split()[k]] = rows["fs"][:, k]
    return c


def column_errors(got, want):
    """relative error per column against that column's largest magnitude; p1 .. p4 against the largest magnitude of
    `force`: the tangential force is a difference of two forces of that size"""
    g, w = columns(got), columns(want)
    fscale = float(np.max(np.abs(w["force"]))) if len(w["force"]) else 1.0
    out = {}
    for k in w:
        scale = fscale if k[0] == "p" else (float(np.max(np.abs(w[k]))) if len(w[k]) else 1.0)
        out[k] = float(np.max(np.abs(g[k] - w[k]))) / (scale if scale > 0 else 1.0) if len(w[k]) else 0.0
    return out
