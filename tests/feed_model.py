"""The rules of the cloud's particle add / delete schedules, stated in pure Python / NumPy (no GPU, no library):

  point_in_region   softParticleCloud::pointInRegion         softParticleCloud.C:1354-1417
  cell_centres      mesh_.C() of a tensor-product block, in OpenFOAM label order
  add_cells         softParticleCloud::findAddParticleCells  softParticleCloud.C:1271-1352
  Lcg48             srand48 / drand48 with skip-ahead
  positions         centre + randomPerturb * (0.5 - u)       softParticleCloud.C:1183-1197
  Schedule          the per-sub-cycle order: enhancedCloud.C:698-711 + addAndDeleteParticle (softParticleCloud.C:1206-1268)

Scalars are Python floats (IEEE doubles, every operation rounded once), so a value computed here is the value a C
double expression in the same order gives."""
import math

import numpy as np

ROOTVSMALL = 1.0e-150
MASK48 = (1 << 48) - 1
LCG_A, LCG_C = 0x5DEECE66D, 0xB
PI_TYPO = 3.14159265358917323846      # library.cpp:460


def point_in_region(option, box, ecc, p):
    x1, x2, y1, y2, z1, z2, r1, r2 = [float(b) for b in box[:8]]
    px, py, pz = float(p[0]), float(p[1]), float(p[2])
    if option == 1:
        return (px - x1) * (px - x2) < ROOTVSMALL and (py - y1) * (py - y2) < ROOTVSMALL and \
            (pz - z1) * (pz - z2) < ROOTVSMALL
    if option == 2:
        a = (x2 - x1, y2 - y1, z2 - z1)
        q = (px - x1, py - y1, pz - z1)
        h = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        dot = a[0] * q[0] + a[1] * q[1] + a[2] * q[2]
        if dot < 0.0 or dot > math.pow(h, 2):
            return False
        qe = (q[0] - float(ecc[0]), q[1] - float(ecc[1]), q[2] - float(ecc[2]))
        dsq = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - dot * dot / math.pow(h, 2)
        dsqE = (qe[0] * qe[0] + qe[1] * qe[1] + qe[2] * qe[2]) - dot * dot / math.pow(h, 2)
        return dsqE > r1 * r1 and dsq < r2 * r2
    return False


def in_region(option, box, ecc, x):
    """point_in_region of every row of x"""
    return np.array([point_in_region(option, box, ecc, p) for p in np.asarray(x, dtype=np.float64).reshape(-1, 3)], bool)


def cell_centres(origin, dx, n, faces=None, labels=None):
    """[ncells, 3] in label order; grid order ix + nx (iy + ny iz) through `labels` (None: identity).  A uniform axis:
    origin + (i + 0.5) dx; a graded one: 0.5 (f[i] + f[i+1])"""
    n = [int(k) for k in n]
    ax = []
    for k in range(3):
        fk = None if faces is None else faces[k]
        if fk is None:
            ax.append([float(origin[k]) + (i + 0.5) * float(dx[k]) for i in range(n[k])])
        else:
            ax.append([0.5 * (float(fk[i]) + float(fk[i + 1])) for i in range(n[k])])
    out = np.zeros((n[0] * n[1] * n[2], 3))
    for iz in range(n[2]):
        for iy in range(n[1]):
            for ix in range(n[0]):
                g = ix + n[0] * (iy + n[1] * iz)
                out[g if labels is None else int(labels[g])] = (ax[0][ix], ax[1][iy], ax[2][iz])
    return out


def add_cells(option, box, ecc, centres, reduce_number_factor):
    inside = [c for c in range(len(centres)) if point_in_region(option, box, ecc, centres[c])]
    n_cell = len(inside)
    coarse = int(reduce_number_factor)
    n_line = int(math.pow(n_cell, 0.5))
    out = []
    for i, c in enumerate(inside):
        n_row, n_column = i % coarse, i // n_line
        if n_row % coarse == 0 and n_column % coarse == 0:
            out.append(c)
    return np.array(out, np.int32)


class Lcg48:
    """X' = (a X + c) mod 2^48, X0 = (seed << 16) | 0x330E with the low 32 bits of the seed, u = X / 2^48: srand48 / drand48"""

    def __init__(self, seed):
        self.x = ((int(seed) & 0xFFFFFFFF) << 16) | 0x330E

    def skip(self, n):
        ra, rc, ba, bc = 1, 0, LCG_A, LCG_C
        n = int(n)
        while n:
            if n & 1:
                ra, rc = (ba * ra) & MASK48, (ba * rc + bc) & MASK48
            ba, bc = (ba * ba) & MASK48, (ba * bc + bc) & MASK48
            n >>= 1
        self.x = (ra * self.x + rc) & MASK48
        return self

    def next(self):
        self.x = (LCG_A * self.x + LCG_C) & MASK48
        return self.x / 281474976710656.0

    @staticmethod
    def draw(seed, j):
        """draw j (0-based) after srand48(seed), reached by skip-ahead"""
        return Lcg48(seed).skip(j).next()


def positions(centres, random_perturb, seed):
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(c)
    for i in range(len(c)):
        for k in range(3):
            u = Lcg48.draw(seed, 3 * i + k)
            out[i, k] = float(c[i, k]) + float(random_perturb) * (0.5 - u)
    return out


def created_mass(diameter, rho):
    r = 0.5 * diameter
    return 4.0 * PI_TYPO / 3.0 * r * r * r * rho


class Schedule:
    """keys: the cloudDict keys; centres: cell_centres(...) of the mesh; deltaT: the CFD step.  sub_cycle() is one pass of
    the loop body of enhancedCloud::evolve in front of the drag assembly, on the grains (x, tag, type) as they stand; it
    returns what has to happen, in order: dict(clear=tags, add=None | dict(pos, tags), delete=tags)."""

    def __init__(self, keys, centres, deltaT):
        self.k = keys
        self.option = int(keys.get("addParticle", 0))
        self.delete = int(keys.get("deleteParticle", 0))
        self.before = int(keys.get("deleteBeforeAdd", 0))
        self.ecc = keys.get("eccentricity", (0.0, 0.0, 0.0))
        self.deltaT = float(deltaT)
        self.centres = np.asarray(centres)
        if self.option > 0:
            self.step = float(keys["addParticleTimeStep"])
            self.cells = add_cells(self.option, keys.get("addParticleBox", (0.0,) * 9), self.ecc, self.centres,
                                   int(keys.get("reduceNumberFactor", 1)))
        else:
            self.step = 1.0 / ROOTVSMALL
            self.cells = np.zeros(0, np.int32)
        self.time_to_add = self.step
        self.totalAdd = self.totalDelete = self.totalDeleteBeforeAdd = 0

    def sub_cycle(self, x, tag, type_):
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        tag = np.asarray(tag)
        one = np.asarray(type_) == 1
        out = dict(clear=np.zeros(0, np.int32), add=None, delete=np.zeros(0, np.int32))
        add_due = self.option > 0 and self.time_to_add <= 0.0
        cleared = np.zeros(len(tag), bool)
        if add_due:
            if self.before and self.delete > 0:
                cleared = one & in_region(self.option, self.k.get("clearInitialBox", (0.0,) * 9), self.ecc, x)
        deleted = np.zeros(len(tag), bool)
        if self.delete > 0:
            deleted = one & ~cleared & in_region(self.option, self.k.get("deleteParticleBox", (0.0,) * 9), self.ecc, x)
        if add_due:
            out["clear"] = tag[cleared].astype(np.int32)
            self.totalDeleteBeforeAdd += int(cleared.sum())
            max_tag = int(tag[~cleared].max()) if (~cleared).any() else 0
            nadd = len(self.cells)
            seed = len(tag) - int(cleared.sum()) + nadd - int(deleted.sum())
            if nadd:
                out["add"] = dict(pos=positions(self.centres[self.cells], float(self.k["randomPerturb"]), seed),
                                  tags=np.arange(max_tag + 1, max_tag + 1 + nadd, dtype=np.int32))
            self.totalAdd += nadd
            self.time_to_add = self.step
        else:
            self.time_to_add -= self.deltaT
        out["delete"] = tag[deleted].astype(np.int32)
        self.totalDelete += int(deleted.sum())
        return out
