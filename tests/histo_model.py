"""The rules of `fix ave/histo` in NumPy and plain Python: the bins and their coordinates, the bin of
one value under beyond ignore | end | extra, the stats (total, missing, min, max), the accumulation of the Nrepeat samples of a
block, the averages one, running and window over the blocks, and the file text.  Written from the rules, not from the engine's
code; tests/test_histo_model.py holds it to hand-computed answers and tests/test_ave_histo_gpu.py holds the engine to it with
==.  Every expression is IEEE float64 without contraction, every count a whole number: no tolerance applies.  The sample
schedule is that of fix ave/time (global_model.schedule)."""
import numpy as np

BIG = 1.0e20
BEYOND = ("ignore", "end", "extra")


class Bins:
    def __init__(self, lo, hi, nbin, beyond="ignore"):
        assert lo < hi and nbin > 0 and beyond in BEYOND
        self.lo, self.hi, self.nbin, self.beyond = np.float64(lo), np.float64(hi), int(nbin), beyond
        self.nbins = self.nbin + (2 if beyond == "extra" else 0)
        self.binsize = (self.hi - self.lo) / np.float64(self.nbin)
        self.bininv = np.float64(1.0) / self.binsize
        c = np.zeros(self.nbins)
        for i in range(self.nbins):
            if beyond != "extra":
                c[i] = self.lo + (i + 0.5) * self.binsize
            elif i == 0:
                c[i] = self.lo
            elif i == self.nbins - 1:
                c[i] = self.hi
            else:
                c[i] = self.lo + (i - 1 + 0.5) * self.binsize
        self.coord = c


class Block:
    """counts and stats of one block (or of an average over blocks)"""

    def __init__(self, nbins):
        self.count = np.zeros(nbins)
        self.total, self.missing, self.min, self.max = 0.0, 0.0, BIG, -BIG

    def add(self, other):
        self.count = self.count + other.count
        self.total += other.total
        self.missing += other.missing
        self.min = min(self.min, other.min)
        self.max = max(self.max, other.max)

    @property
    def frac(self):
        return self.count / self.total if self.total > 0 else np.zeros(len(self.count))


def bin_values(bins, values, block=None):
    """the values (any shape) binned into `block` (a new one when None), one after the other by the rule"""
    b = block if block is not None else Block(bins.nbins)
    for v in np.asarray(values, dtype=np.float64).reshape(-1):
        b.min = min(b.min, float(v))
        b.max = max(b.max, float(v))
        if v < bins.lo:
            if bins.beyond == "ignore":
                b.missing += 1
                continue
            ibin = 0
        elif v > bins.hi:
            if bins.beyond == "ignore":
                b.missing += 1
                continue
            ibin = bins.nbins - 1
        else:
            ibin = int((v - bins.lo) * bins.bininv)
            ibin = min(ibin, bins.nbins - 1)
            if bins.beyond == "extra":
                ibin += 1
        b.count[ibin] += 1
        b.total += 1
    return b


class Averager:
    """ave one | running | window M over the blocks as they come"""

    def __init__(self, nbins, ave="one", window=0):
        assert ave in ("one", "running", "window") and (ave != "window" or window > 0)
        self.nbins, self.ave, self.window, self.blocks = nbins, ave, window, []

    def output(self, block):
        self.blocks.append(block)
        use = self.blocks[-1:] if self.ave == "one" else (self.blocks if self.ave == "running" else self.blocks[-self.window:])
        out = Block(self.nbins)
        for b in use:
            out.add(b)
        return out


def header(fix_id, title1=None, title2=None, title3=None):
    t = ["# Histogrammed data for fix %s" % fix_id,
         "# TimeStep Number-of-bins Total-counts Missing-counts Min-value Max-value", "# Bin Coord Count Count/Total"]
    return "".join((given if given is not None else default) + "\n" for given, default in zip((title1, title2, title3), t))


def text(step, bins, block):
    out = "%d %d %g %g %g %g\n" % (step, bins.nbins, block.total, block.missing, block.min, block.max)
    for i in range(bins.nbins):
        if block.total > 0:
            out += "%d %g %g %g\n" % (i + 1, bins.coord[i], block.count[i], block.count[i] / block.total)
        else:
            out += "%d %g 0 0\n" % (i + 1, bins.coord[i])
    return out
