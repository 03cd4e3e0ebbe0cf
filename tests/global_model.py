"""The rules of `compute reduce`, `fix ave/time` and the c_ columns of thermo in NumPy and plain
Python: the six modes over a group mask and over an empty set, the sample schedule with `start`, the averages one, running and
window, the file text, and a thermo cell with its normalisation.  Written from the rules, not from the engine's code;
tests/test_global_model.py holds it to hand-computed answers and tests/test_global_gpu.py holds the engine to it.  Sums are
taken in index order, one element after the other, in float64."""
import numpy as np

BIG = 1.0e20
MODES = ("sum", "min", "max", "ave", "sumsq", "avesq")
EPS = 2.0 ** -53


def _terms(mode, values, mask=None):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if mask is not None:
        v = v[np.asarray(mask, dtype=bool).reshape(-1)]
    return v * v if mode in ("sumsq", "avesq") else v


def in_order_sum(terms):
    s = 0.0
    for t in terms:
        s += float(t)
    return s


def reduce(mode, values, mask=None):
    """one input of compute reduce over the elements the mask selects (None: all): sum | min | max | ave | sumsq | avesq.
    An empty set: sum = sumsq = 0, min = 1e20, max = -1e20; ave and avesq divide by the count unless it is 0"""
    t = _terms(mode, values, mask)
    if mode == "min":
        return float(min(BIG, t.min())) if len(t) else BIG
    if mode == "max":
        return float(max(-BIG, t.max())) if len(t) else -BIG
    s = in_order_sum(t)
    if mode in ("ave", "avesq") and len(t) > 0:
        s = s / float(len(t))
    return s


def gate(mode, values, mask=None):
    """what two summations of the same terms in different orders may differ by: each is within n 2^-53 sum |term| of the
    exact sum (n the number of terms), so 2 n 2^-53 sum |term|; 0 for min and max.  ave and avesq: that of the sum over the
    count, plus one rounding of each of the two divisions, 2 2^-53 |result|"""
    if mode in ("min", "max"):
        return 0.0
    t = _terms(mode, values, mask)
    n = len(t)
    g = 2.0 * n * EPS * float(np.sum(np.abs(t)))
    if mode in ("ave", "avesq") and n > 0:
        g = g / n + 2.0 * EPS * abs(reduce(mode, values, mask))
    return g


def extensive(mode):
    return mode in ("sum", "sumsq")


def first_valid(t0, nevery, nrepeat, nfreq, start=0):
    nv = (t0 // nfreq) * nfreq + nfreq
    while nv < start:
        nv += nfreq
    if nv - nfreq == t0 and nrepeat == 1:
        nv = t0
    else:
        nv -= (nrepeat - 1) * nevery
    if nv < t0:
        nv += nfreq
    return nv


def schedule(t0, nevery, nrepeat, nfreq, end, start=0):
    """[(output step, [sample steps])] of a fix defined at step t0, for the outputs that fall at or before step `end`"""
    out = []
    nv = first_valid(t0, nevery, nrepeat, nfreq, start)
    while True:
        samples = [nv + k * nevery for k in range(nrepeat)]
        if samples[-1] > end:
            return out
        out.append((samples[-1], samples))
        nv = samples[-1] + nfreq - (nrepeat - 1) * nevery


class TimeAverager:
    """fix ave/time in scalar mode: add_sample(values) per sample step, output() after every Nrepeat of them"""

    def __init__(self, nvalues, nrepeat, ave="one", window=0):
        assert ave in ("one", "running", "window") and (ave != "window" or window > 0)
        self.nv, self.nrepeat, self.ave, self.window = nvalues, nrepeat, ave, window
        self.acc = [0.0] * nvalues
        self.blocks = []
        self.nsample = 0

    def add_sample(self, values):
        assert len(values) == self.nv
        for j, v in enumerate(values):
            self.acc[j] += float(v)
        self.nsample += 1

    def output(self):
        assert self.nsample == self.nrepeat
        block = [a / float(self.nrepeat) for a in self.acc]
        self.acc = [0.0] * self.nv
        self.nsample = 0
        self.blocks.append(block)
        if self.ave == "one":
            use = self.blocks[-1:]
        elif self.ave == "running":
            use = self.blocks
        else:
            use = self.blocks[-self.window:]
        return np.array([in_order_sum(b[j] for b in use) / float(len(use)) for j in range(self.nv)])


def header(fix_id, words, title1=None, title2=None):
    t1 = "# Time-averaged data for fix %s" % fix_id
    t2 = "# TimeStep" + "".join(" " + w for w in words)
    return (title1 if title1 is not None else t1) + "\n" + (title2 if title2 is not None else t2) + "\n"


def line(step, values, fmt=" %g"):
    return "%d" % step + "".join(fmt % float(v) for v in values) + "\n"


def thermo_value(value, is_extensive, norm, natoms):
    return value / float(natoms) if (is_extensive and norm and natoms > 0) else value


def thermo_cell(value):
    return "%12.8g " % value
