"""Inputs of the neighbour-list tests (tests/test_neigh_model.py on the CPU, tests/test_neigh_list_gpu.py on the GPU):
random clouds, lattices whose pair distances are exact in binary, and the hot beds whose lists are rebuilt inside a run.
Every bed is an explicit dictionary; the references are computed once per process and shared."""
import functools

import numpy as np

from tests import neigh_model as nm

D = 1.0e-3                 # largest diameter of every cloud
SKIN = 0.25e-3
CUT = D + SKIN             # 2 rmax + skin
CFG = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=0.0, dt=1.0e-6, skin=SKIN)
COHESIVE = (1.0e-13, 1.0e-7, 1.0e-7, 1.0e-4, 1)
LUB = (1.0e-3, 1, 1, 1.001e-3, 1.1e-3, 1, 1)   # cut_global 1.1 mm: the absolute cutoff 1.35 mm exceeds 2 rmax + skin


def walls_of(bed):
    return [(k, float(bed["boxlo"][k]), float(bed["boxhi"][k])) for k in range(3) if not bed["periodic"][k]]


def _cloud(n, cutoffs, periodic, seed, lo=(0.0, 0.0, 0.0), dmin=None):
    """n points uniform in a box of `cutoffs` x CUT; the first atom always has the diameter D, so that 2 rmax + skin = CUT"""
    assert n >= 300 and n % 64 != 0
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, dtype=np.float64)
    hi = lo + np.asarray(cutoffs, dtype=np.float64) * CUT
    x = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    x = np.minimum(np.maximum(x, lo), np.nextafter(hi, lo))   # (lo + u * len may round up to hi)
    diam = np.full(n, D) if dmin is None else rng.uniform(dmin, D, size=n)
    diam[0] = D
    return dict(x=x, v=np.zeros((n, 3)), diameter=diam, density=np.full(n, 2650.0), boxlo=lo, boxhi=hi,
                periodic=tuple(periodic), n=n)


# name -> (atoms, box in cutoffs, periodic, seed, lo, smallest diameter).  The seeds are the first ones, counted from 1, whose
# cloud has no candidate pair within neigh_model.BAND of its cutoff (checked by test_neigh_model.py for every cloud and cutoff).
CLOUDS = {
    "periodic_5x4x6": (539, (5.3, 4.1, 6.2), (1, 1, 1), 1, (0.0, 0.0, 0.0), None),
    "periodic_3x3x3_exact": (325, (3.0, 3.0, 3.0), (1, 1, 1), 1, (-0.7e-3, 0.4e-3, -1.1e-3), None),
    "xz_periodic_thin": (323, (2.2, 9.7, 3.0), (1, 0, 1), 1, (0.0, 0.0, 0.0), None),
    "closed_4p5": (469, (4.5, 4.5, 4.5), (0, 0, 0), 1, (0.0, 0.0, 0.0), None),
    "poly_ratio3": (1511, (7.3, 6.9, 7.5), (1, 1, 1), 1, (0.0, 0.0, 0.0), D / 3.0),
    "dense": (787, (3.1, 3.1, 3.1), (1, 1, 1), 1, (0.0, 0.0, 0.0), None),
}
# (cloud, extra settings, absolute cutoff of the list)
CLOUD_RUNS = [
    ("periodic_5x4x6", {}, 0.0),
    ("periodic_3x3x3_exact", {}, 0.0),
    ("xz_periodic_thin", {}, 0.0),
    ("closed_4p5", {}, 0.0),
    ("poly_ratio3", {}, 0.0),
    ("poly_ratio3", {"cohesive": COHESIVE}, CUT),
    ("poly_ratio3", {"lub": LUB}, LUB[4] + SKIN),
    ("dense", {}, 0.0),
]


@functools.lru_cache(maxsize=None)
def cloud(name):
    n, cutoffs, periodic, seed, lo, dmin = CLOUDS[name]
    return _cloud(n, cutoffs, periodic, seed, lo, dmin)


def cloud_cfg(name, extra):
    bed = cloud(name)
    return dict(CFG, walls=walls_of(bed), **extra)


@functools.lru_cache(maxsize=None)
def cloud_model(name, cut_abs):
    """(rows as a set, band, rows as an array) of a cloud, read-only"""
    bed = cloud(name)
    rows, band = nm.neighbor_rows(bed["x"], 0.5 * bed["diameter"], bed["boxlo"], bed["boxhi"], bed["periodic"], SKIN,
                                  cut_abs)
    rows.setflags(write=False)
    return frozenset(nm.as_set(rows)), band, rows


# ---- exact cases: every length an integer multiple of u = 2^-14 m, so that every rsq and cut^2 is a small integer times
# 2^-28 and both the engine and the model compute them exactly -- no band ----
U = 2.0 ** -14
EX_K = (5, 4, 6)                     # box lengths in cutoffs


def exact_cfg(bed):
    return dict(CFG, skin=bed["skin"], walls=walls_of(bed))
EX_BOXES = {"ppp": (1, 1, 1), "pfp": (1, 0, 1), "fff": (0, 0, 0)}
EX_LO = {"origin": 0, "shifted": -37}
# A second size of the lattice alone, diameter 40 u + skin 9 u.  With the cutoff 20 u the rounded inverse of the cell width
# errs upwards and floor((x - lo) * inv) is right on every corner; with 49 u it errs downwards: a cell as wide as the cutoff
# then puts the corners 4 and 5 of a ghost-extended grid into the cells 3 and 5, two apart
EX_SIZES = {"cut20": (16, 4), "cut49": (40, 9)}


def exact_case(box, lo_name, lattice_only=False, size="cut20"):
    """-> bed + "xw" (the positions after the periodic wrap), "pairs_at_cutoff" (tag pairs that must be listed),
    "pairs_beyond" (tag pairs that must not be), "wrapped" (tags of the atoms given at hi of a periodic dimension)"""
    periodic = EX_BOXES[box]
    du, su = EX_SIZES[size]
    c = du + su                                              # the cutoff in units of u
    assert c == 20 or lattice_only
    lo = np.full(3, EX_LO[lo_name], dtype=np.int64)          # in units of u
    hi = lo + c * np.asarray(EX_K, dtype=np.int64)
    # simple cubic lattice on the cell corners; a walled dimension also holds the layer at exactly hi
    cnt = [EX_K[k] if periodic[k] else EX_K[k] + 1 for k in range(3)]
    abc = np.stack(np.meshgrid(*[np.arange(c) for c in cnt], indexing="ij"), axis=-1).reshape(-1, 3)
    pts = [lo + c * abc]
    nsc = len(abc)
    at_cut, beyond, wrapped = [], [], []
    if not lattice_only:
        # second lattice: a third of the corners, displaced by (12, 16, 0) u: 12^2 + 16^2 = 20^2 exactly
        sel = np.nonzero((abc[:, 0] + 2 * abc[:, 1] + 3 * abc[:, 2]) % 3 == 0)[0]
        second = lo + 20 * abc[sel] + np.array([12, 16, 0])
        inside = np.all(second < hi, axis=1)
        sel, second = sel[inside], second[inside]
        pts.append(second)
        at_cut += [(nsc + 1 + k, int(s) + 1) for k, s in enumerate(sel)]
        # a probe one u further in z from a corner that has no second-lattice atom: 12^2 + 16^2 + 1 = 401 > 400
        p0 = int(np.nonzero((abc == (2, 1, 2)).all(axis=1))[0][0])
        assert p0 not in sel
        pts.append((lo + 20 * abc[p0] + np.array([12, 16, 1]))[None, :])
        beyond.append((nsc + len(sel) + 1, p0 + 1))
        # one atom at exactly hi of every dimension (periodic: wrapped to lo; walled: stays on the wall)
        off = np.array([27, 31, 33])
        for k in range(3):
            p = lo + np.roll(off, k)
            p[k] = hi[k]
            pts.append(p[None, :])
            if periodic[k]:
                wrapped.append(nsc + len(sel) + 2 + k)
    xi = np.concatenate(pts, axis=0)
    n = len(xi)
    xw = xi.copy()
    for k in range(3):
        if periodic[k]:
            xw[:, k] = np.where(xw[:, k] >= hi[k], xw[:, k] - c * EX_K[k], xw[:, k])
    return dict(x=xi * U, xw=xw * U, v=np.zeros((n, 3)), diameter=np.full(n, du * U), density=np.full(n, 2650.0),
                boxlo=lo * U, boxhi=hi * U, periodic=periodic, n=n, nsc=nsc, pairs_at_cutoff=at_cut, pairs_beyond=beyond,
                wrapped=wrapped, skin=su * U)


def exact_lattice_rows(box):
    """rows of the simple cubic lattice alone: two per bond of one cutoff's length"""
    periodic = EX_BOXES[box]
    cnt = [EX_K[k] if periodic[k] else EX_K[k] + 1 for k in range(3)]
    total = 0
    for k in range(3):
        others = int(np.prod([cnt[m] for m in range(3) if m != k]))
        total += 2 * (cnt[k] if periodic[k] else cnt[k] - 1) * others
    return total


@functools.lru_cache(maxsize=None)
def exact_model(box, lo_name, lattice_only=False, size="cut20"):
    bed = exact_case(box, lo_name, lattice_only, size)
    rows, band = nm.neighbor_rows(bed["xw"], 0.5 * bed["diameter"], bed["boxlo"], bed["boxhi"], bed["periodic"], bed["skin"])
    return frozenset(nm.as_set(rows)), band, rows


# ---- hot beds: lists rebuilt inside a run (jittered FCC lattices, fast grains, thin skin) ----
def fcc_bed(ncells, periodic, seed, **kw):
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(ncells, seed=seed, **kw)
    if not periodic:   # closed box: walls on every side, lattice shifted one radius inside
        bed["periodic"] = (0, 0, 0)
        bed["x"][:, 0] += 0.3e-3
        bed["x"][:, 2] += 0.3e-3
        bed["boxhi"][0] += 0.6e-3
        bed["boxhi"][2] += 0.6e-3
    return bed


HOT_BASE = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.03e-3)


def hot_bed(name):
    """-> bed, cfg, sub-steps per leg"""
    if name == "loose_periodic":
        bed = fcc_bed((7, 6, 8), True, 23, vmax=0.5, jitter=0.3, spacing=1.1)
        cfg, leg = dict(HOT_BASE), 50
    elif name == "closed":
        bed = fcc_bed((5, 5, 5), False, 5, vmax=0.5)
        cfg, leg = dict(HOT_BASE), 50
    else:
        bed = fcc_bed((5, 5, 5), True, 11, poly=(0.85e-3, 1.0e-3), spacing=0.95, vmax=0.3)
        cfg, leg = dict(HOT_BASE, cohesive=COHESIVE, lub=LUB), 45
    cfg["walls"] = walls_of(bed)
    return bed, cfg, leg


def hot_cut_abs(bed, cfg):
    """the absolute cutoff of the engine's one list: cut_global + skin with lubricate/poly, at least 2 rmax + skin with fix
    cohesive, 0 for a granular style alone"""
    c = 0.0
    if cfg.get("lub"):
        c = cfg["lub"][4] + cfg["skin"]
    if cfg.get("cohesive"):
        c = max(c, max(float(np.max(bed["diameter"])), cfg["lub"][4] if cfg.get("lub") else 0.0) + cfg["skin"])
    return c
