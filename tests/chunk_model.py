"""The rules of `compute chunk/atom bin/1d|2d|3d` and `fix ave/chunk` in NumPy: the layers of a
dimension, the chunk ID of an atom, chunk volumes and centres, the sample schedule, the three norms, `ave running` and the
file text.  Written from the rules, not from the engine's code; tests/test_chunk_model.py holds it to hand-computed answers and
tests/test_ave_chunk_gpu.py holds the engine to it.  Every expression that decides a layer is evaluated in float64 in the
order the rules give, so chunk IDs compare with ==."""
import numpy as np

GATE = 1e-13   # per entry of a value column, against the column's largest chunk mean of |value| (summation order only)
DIMS = {"x": 0, "y": 1, "z": 2}


def layers(origin, delta, minvalue, maxvalue):
    """(offset, invdelta, nlayers) of one dimension"""
    invdelta = 1.0 / delta
    lo = origin + int((minvalue - origin) * invdelta) * delta
    if lo > minvalue:
        lo -= delta
    hi = origin + int((maxvalue - origin) * invdelta) * delta
    if hi < maxvalue:
        hi += delta
    return lo, invdelta, int((hi - lo) * invdelta + 0.5)


def bins(line, boxlo, boxhi, periodic):
    """the bins of `compute ID group chunk/atom bin/Nd dim origin delta ... units box|reduced [bound dim lo hi] [discard
    yes|no|mixed]` on this box (the accepted no-op keywords are skipped)"""
    w = line.split()
    assert w[0] == "compute" and w[3] == "chunk/atom" and w[4] in ("bin/1d", "bin/2d", "bin/3d"), line
    ndim = int(w[4][4])
    trip = [(DIMS[w[5 + 3 * a]], w[6 + 3 * a], float(w[7 + 3 * a])) for a in range(ndim)]
    k = 5 + 3 * ndim
    units, discard, bound = None, "mixed", {}
    while k < len(w):
        if w[k] == "units":
            units = w[k + 1]; k += 2
        elif w[k] == "discard":
            discard = w[k + 1]; k += 2
        elif w[k] == "bound":
            bound[DIMS[w[k + 1]]] = (w[k + 2], w[k + 3]); k += 4
        elif w[k] in ("nchunk", "ids", "limit", "compress", "pbc"):
            k += 2
        else:
            raise ValueError(w[k])
    assert units in ("box", "reduced"), line
    B = dict(ndim=ndim, dim=[], offset=[], invdelta=[], delta=[], nlayers=[], discard=[], periodic=[], lo=[], hi=[], prd=[])
    volume = 1.0
    for d, org, delta in trip:
        lo, hi = float(boxlo[d]), float(boxhi[d])
        prd = hi - lo
        conv = (lambda f: lo + f * prd) if units == "reduced" else (lambda f: f)
        if units == "reduced":
            delta = delta * prd
        origin = {"lower": lo, "upper": hi, "center": 0.5 * (lo + hi)}[org] if org in ("lower", "upper", "center") else conv(float(org))
        mn, mx = lo, hi
        if d in bound:
            if bound[d][0] != "lower":
                mn = conv(float(bound[d][0]))
            if bound[d][1] != "upper":
                mx = conv(float(bound[d][1]))
        off, inv, nl = layers(origin, delta, mn, mx)
        B["dim"].append(d); B["offset"].append(off); B["invdelta"].append(inv); B["delta"].append(delta); B["nlayers"].append(nl)
        B["discard"].append(discard == "yes" or (discard == "mixed" and d in bound))
        B["periodic"].append(bool(periodic[d])); B["lo"].append(lo); B["hi"].append(hi); B["prd"].append(prd)
        volume *= delta
    for d in range(3):
        if d not in B["dim"]:
            volume *= float(boxhi[d]) - float(boxlo[d])
    B["volume"] = volume
    B["nchunk"] = int(np.prod(B["nlayers"]))
    return B


def assign(B, x, in_group=None):
    """chunk IDs (int64) of the atoms at x[n, 3]: 1 + ((i1 n2) + i2) n3 + i3, 0 outside the group or discarded"""
    x = np.asarray(x, dtype=np.float64)
    lin = np.zeros(len(x), np.int64)
    out = np.zeros(len(x), bool)
    for a in range(B["ndim"]):
        xr = x[:, B["dim"][a]].copy()
        if B["periodic"][a]:
            xr = np.where(xr < B["lo"][a], xr + B["prd"][a], xr)
            xr = np.where(xr >= B["hi"][a], xr - B["prd"][a], xr)
        ibin = ((xr - B["offset"][a]) * B["invdelta"][a]).astype(np.int64)   # (truncates toward zero, like the C cast)
        ibin -= xr < B["offset"][a]
        last = B["nlayers"][a] - 1
        outside = (ibin < 0) | (ibin > last)
        if B["discard"][a]:
            out |= outside
        ibin = np.clip(ibin, 0, last)
        lin = lin * B["nlayers"][a] + ibin
    ids = np.where(out, 0, 1 + lin)
    if in_group is not None:
        ids = np.where(in_group, ids, 0)
    return ids


def coords(B):
    """centres [nchunk, ndim], chunk 1 first"""
    grids = np.meshgrid(*[B["offset"][a] + (np.arange(B["nlayers"][a]) + 0.5) * B["delta"][a] for a in range(B["ndim"])],
                        indexing="ij")
    return np.stack([g.reshape(-1) for g in grids], axis=1)


def first_valid(t0, nevery, nrepeat, nfreq):
    nv = (t0 // nfreq) * nfreq + nfreq
    if nv - nfreq == t0 and nrepeat == 1:
        nv = t0
    else:
        nv -= (nrepeat - 1) * nevery
    if nv < t0:
        nv += nfreq
    return nv


def schedule(t0, nevery, nrepeat, nfreq, end):
    """[(output step, [sample steps])] of a fix defined at step t0, for the outputs that fall at or before step `end`"""
    out = []
    nv = first_valid(t0, nevery, nrepeat, nfreq)
    while True:
        samples = [nv + k * nevery for k in range(nrepeat)]
        if samples[-1] > end:
            return out
        out.append((samples[-1], samples))
        nv = samples[-1] + nfreq - (nrepeat - 1) * nevery


DENSITIES = ("density/number", "density/mass")


class Averager:
    """the sums of fix ave/chunk: add_sample() per sample step, output() after every Nrepeat of them"""

    def __init__(self, B, names, norm="all", running=False, nrepeat=1):
        self.B, self.names, self.norm, self.running, self.nrepeat = B, list(names), norm, running, nrepeat
        n, m = B["nchunk"], len(self.names)
        self.count, self.sums = np.zeros(n), np.zeros((n, m))
        self.tot_count, self.tot_sums, self.res_sum, self.nout = np.zeros(n), np.zeros((n, m)), np.zeros((n, 1 + m)), 0

    def add_sample(self, ids, columns):
        """ids: chunk IDs of the atoms that count (0: none); columns: {name: per-atom values}; density/number needs none,
        density/mass takes columns["mass"]"""
        n = self.B["nchunk"]
        per = lambda wgt: np.bincount(ids, weights=wgt, minlength=n + 1)[1:]
        cnt = per(np.ones(len(ids)))
        self.count += cnt
        for j, name in enumerate(self.names):
            if name == "density/number":
                s = cnt
            elif name == "density/mass":
                s = per(columns["mass"])
            else:
                s = per(columns[name])
                if self.norm == "sample":
                    s = np.where(cnt > 0, s / np.where(cnt > 0, cnt, 1.0), 0.0)
            self.sums[:, j] += s

    def output(self):
        """(Ncount[nchunk], values[nchunk, nvalues]) of the samples since the last output"""
        nrep, V = float(self.nrepeat), self.B["volume"]
        self.tot_count += self.count
        self.tot_sums += self.sums
        cnt, sums = (self.tot_count, self.tot_sums) if self.running else (self.count, self.sums)
        res = np.zeros((self.B["nchunk"], 1 + len(self.names)))
        res[:, 0] = self.count / nrep
        for j, name in enumerate(self.names):
            if name in DENSITIES:
                res[:, 1 + j] = self.sums[:, j] / nrep / V
            elif self.norm == "all":
                res[:, 1 + j] = np.where(cnt > 0, sums[:, j] / np.where(cnt > 0, cnt, 1.0), 0.0)
            else:
                res[:, 1 + j] = self.sums[:, j] / nrep
        self.nout += 1
        self.res_sum += res
        if self.running:
            mean = self.res_sum / float(self.nout)
            for j, name in enumerate(self.names):
                if self.norm == "all" and name not in DENSITIES:
                    mean[:, 1 + j] = res[:, 1 + j]
            res = mean
        self.count, self.sums = np.zeros_like(self.count), np.zeros_like(self.sums)
        return res[:, 0].copy(), res[:, 1:].copy()


def header(fix_id, group, B, names, titles=(None, None, None)):
    t = ["# Chunk-averaged data for fix %s and group %s" % (fix_id, group), "# Timestep Number-of-chunks Total-count",
         "# Chunk " + " ".join("Coord%d" % (a + 1) for a in range(B["ndim"])) + " Ncount " + " ".join(names)]
    return "".join((titles[k] if titles[k] is not None else t[k]) + "\n" for k in range(3))


def text(step, B, count, values, fmt="%g"):
    """the body of one output"""
    xyz = coords(B)
    total = 0.0
    for c in count:   # (added one after another, as the engine's host code does)
        total += float(c)
    out = ["%d %d %g\n" % (step, B["nchunk"], total)]
    for c in range(B["nchunk"]):
        out.append("  %d" % (c + 1) + "".join(" %g" % v for v in xyz[c]) + " %g" % count[c] + "".join(" " + fmt % v for v in values[c]) + "\n")
    return "".join(out)


def column_errors(got, want, scale):
    """max |got - want| per value column over its scale (the largest chunk mean of |value|, from an Averager fed |columns|)"""
    s = np.max(np.abs(scale), axis=0)
    return np.max(np.abs(np.asarray(got) - np.asarray(want)), axis=0) / np.where(s > 0, s, 1.0)
