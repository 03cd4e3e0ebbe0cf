"""The rules of `compute rdf ... cutoff Rc`, `compute coord/atom cutoff Rc` and `fix ave/time ... mode vector` (DESIGN.md
section 20) in NumPy and plain Python: brute force over all ordered pairs, O(n^2).  Written from the rules, not from the
engine's code; tests/test_nbr_model.py holds it to answers worked out by hand and tests/test_nbr_gpu.py holds the engine to it.
Every quantity is an integer count or a fixed sequence of IEEE operations on integer counts, each rounded on its own in
float64, so the engine must equal this model with ==."""
import numpy as np

from tests import global_model as gm

PI = 3.14159265358979323846
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def type_range(word):
    """an integer, a*b, a*, *b or * -> (lo, hi), both ends included; an open end is every type from or up to there"""
    word = str(word)
    if "*" not in word:
        return int(word), int(word)
    a, b = word.split("*")
    return (int(a) if a else INT_MIN), (int(b) if b else INT_MAX)


def _in(types, rng):
    return (types >= rng[0]) & (types <= rng[1])


def pair_rsq(x, boxlo, boxhi, periodic):
    """rsq[i, j] of d = x[j] - x[i] per component, in a periodic dimension of length L: d > 0.5 L -> d - L, else
    d < -0.5 L -> d + L, applied once; rsq = (dx dx + dy dy) + dz dz"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    d = x[None, :, :] - x[:, None, :]
    for a in range(3):
        if periodic[a]:
            L = np.float64(boxhi[a]) - np.float64(boxlo[a])
            half = np.float64(0.5) * L
            da = d[:, :, a]
            d[:, :, a] = np.where(da > half, da - L, np.where(da < -half, da + L, da))
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def check_box(rc, boxlo, boxhi, periodic):
    for a in range(3):
        if periodic[a] and (np.float64(boxhi[a]) - np.float64(boxlo[a])) < 2.0 * rc:
            raise ValueError("cutoff is longer than half a periodic box length")


def rdf_counts(x, types, group, boxlo, boxhi, periodic, nbin, rc, pairs=(("*", "*"),), rsq=None):
    """dict(counts [npairs, nbin], icount, jcount, duplicates [npairs]), all int64.  group: bool per atom; rsq: pair_rsq of
    these positions where the caller has it already"""
    check_box(rc, boxlo, boxhi, periodic)
    types = np.asarray(types).reshape(-1)
    group = np.asarray(group, dtype=bool).reshape(-1)
    n = len(types)
    delr = np.float64(rc) / np.float64(nbin)
    delrinv = np.float64(1.0) / delr
    if rsq is None:
        rsq = pair_rsq(x, boxlo, boxhi, periodic) if n else np.zeros((0, 0))
    q = np.sqrt(rsq) * delrinv
    ok = (q < np.float64(nbin)) & group[:, None] & group[None, :] & ~np.eye(n, dtype=bool)
    ibin = np.where(ok, q, 0.0).astype(np.int64)   # (int)(r * delrinv)
    counts = np.zeros((len(pairs), nbin), np.int64)
    ic, jc, dup = (np.zeros(len(pairs), np.int64) for _ in range(3))
    for m, (iw, jw) in enumerate(pairs):
        ti, tj = _in(types, type_range(iw)), _in(types, type_range(jw))
        sel = ok & ti[:, None] & tj[None, :]
        counts[m] = np.bincount(ibin[sel], minlength=nbin)[:nbin]
        ic[m], jc[m], dup[m] = (group & ti).sum(), (group & tj).sum(), (group & ti & tj).sum()
    return dict(counts=counts, icount=ic, jcount=jc, duplicates=dup)


def rdf_array(c, boxlo, boxhi, nbin, rc):
    """the global array [nbin, 1 + 2 npairs] from the counts, operation by operation in the order of the rule"""
    npairs = len(c["icount"])
    out = np.zeros((nbin, 1 + 2 * npairs))
    f = np.float64
    L = [f(boxhi[a]) - f(boxlo[a]) for a in range(3)]
    delr = f(rc) / f(nbin)
    constant = f(4.0) * f(PI) / (f(3.0) * L[0] * L[1] * L[2])
    for ibin in range(nbin):
        out[ibin, 0] = (f(ibin) + f(0.5)) * delr
    for m in range(npairs):
        icount, jcount, dup = int(c["icount"][m]), int(c["jcount"][m]), int(c["duplicates"][m])
        normfac = f(jcount) - f(dup) / f(icount) if icount > 0 else f(0.0)
        ncoord = f(0.0)
        for ibin in range(nbin):
            rlower, rupper = f(ibin) * delr, f(ibin + 1) * delr
            vfrac = constant * (rupper * rupper * rupper - rlower * rlower * rlower)
            vn = vfrac * normfac
            gr = f(int(c["counts"][m, ibin])) / (vn * f(icount)) if vn != 0.0 else f(0.0)
            if icount != 0:
                ncoord = ncoord + gr * vfrac * normfac
            out[ibin, 1 + 2 * m] = gr
            out[ibin, 2 + 2 * m] = ncoord
    return out


def rdf(x, types, group, boxlo, boxhi, periodic, nbin, rc, pairs=(("*", "*"),)):
    return rdf_array(rdf_counts(x, types, group, boxlo, boxhi, periodic, nbin, rc, pairs), boxlo, boxhi, nbin, rc)


def coord_atom(x, types, group, boxlo, boxhi, periodic, rc, ranges=("*",), rsq=None):
    """[n, nranges] float64: for the atoms i of the group the atoms j != i of ANY group with rsq < rc rc (strict) whose type
    is in the range; 0 for the others"""
    check_box(rc, boxlo, boxhi, periodic)
    types = np.asarray(types).reshape(-1)
    group = np.asarray(group, dtype=bool).reshape(-1)
    n = len(types)
    if rsq is None:
        rsq = pair_rsq(x, boxlo, boxhi, periodic) if n else np.zeros((0, 0))
    near = (rsq < np.float64(rc) * np.float64(rc)) & ~np.eye(n, dtype=bool) & group[:, None]
    out = np.zeros((n, len(ranges)))
    for k, w in enumerate(ranges):
        out[:, k] = (near & _in(types, type_range(w))[None, :]).sum(axis=1)
    return out


class VectorAverager(gm.TimeAverager):
    """fix ave/time mode vector over nvalues columns of nrows rows: add_sample(columns [nrows, nvalues]) per sample step,
    output() [nrows, nvalues] after every Nrepeat of them -- every element averaged as a scalar value is"""

    def __init__(self, nrows, nvalues, nrepeat, ave="one", window=0):
        super().__init__(nrows * nvalues, nrepeat, ave, window)
        self.shape = (nrows, nvalues)

    def add_sample(self, columns):
        columns = np.asarray(columns, dtype=np.float64)
        assert columns.shape == self.shape
        super().add_sample(columns.reshape(-1))

    def output(self):
        return super().output().reshape(self.shape)


def vector_header(fix_id, words, title1=None, title2=None, title3=None):
    t1 = "# Time-averaged data for fix %s" % fix_id
    t2 = "# TimeStep Number-of-rows"
    t3 = "# Row" + "".join(" " + w for w in words)
    return "".join((t if t is not None else d) + "\n" for t, d in ((title1, t1), (title2, t2), (title3, t3)))


def vector_block(step, values, fmt=" %g"):
    """one output: `step nrows`, then per row its number from 1 and the format applied to each value"""
    values = np.asarray(values, dtype=np.float64)
    text = "%d %d\n" % (step, values.shape[0])
    for r in range(values.shape[0]):
        text += "%d" % (r + 1) + "".join(fmt % float(v) for v in values[r]) + "\n"
    return text
