"""Brute-force reference of the neighbour list: plain NumPy in float64, all pairs times all periodic images, no cells.

A row (tag_i, tag_j, sx, sy, sz) is in the list when (j, s) != (i, 0) and
    |x_i - (x_j + s * L)|^2 <= cut^2,   cut = max(r_i + r_j + skin, cut_abs)
(LAMMPS' rsq <= cutsq of the granular list; cut_abs is the absolute cutoff of lubricate/poly or of fix cohesive's regular
list, 0 for a granular style alone).  s runs over {-1, 0, 1} in the periodic dimensions, the image is formed as
x_j + s * L, the position a ghost copy gets.

The "band" is the number of candidate pairs whose rsq lies within 16 * 2^-52 of cut^2: a GPU kernel contracts
dx*dx + dy*dy + dz*dz into FMAs and NumPy does not, so only such pairs may be decided differently.  A test input is chosen
so that its band is empty; the comparison is then exact."""
import itertools

import numpy as np

BAND = 16.0 * 2.0 ** -52


def shifts(periodic):
    """the image vectors s, (0, 0, 0) first"""
    rng = [(0, -1, 1) if p else (0,) for p in periodic]
    return [s for s in itertools.product(*rng)]


def neighbor_rows(x, radius, boxlo, boxhi, periodic, skin, cut_abs=0.0, tag=None, chunk=256, touching=False):
    """-> (rows, band): rows = (m, 5) int64 array of tag_i, tag_j, sx, sy, sz (unsorted, no duplicates), band = number of
    candidates within BAND of the cutoff.  touching=True: the criterion is rsq < (r_i + r_j)^2 instead (pairs in
    contact), band = 0."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(radius, dtype=np.float64)
    n = x.shape[0]
    tag = np.arange(1, n + 1, dtype=np.int64) if tag is None else np.asarray(tag, dtype=np.int64)
    prd = np.asarray(boxhi, dtype=np.float64) - np.asarray(boxlo, dtype=np.float64)
    out = []
    band = 0
    idx = np.arange(n)
    for s in shifts(periodic):
        xj = x + np.asarray(s, dtype=np.float64) * prd          # x_j + s * L
        self_image = all(c == 0 for c in s)
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            dx = x[a:b, None, 0] - xj[None, :, 0]
            dy = x[a:b, None, 1] - xj[None, :, 1]
            dz = x[a:b, None, 2] - xj[None, :, 2]
            rsq = dx * dx + dy * dy + dz * dz
            if touching:
                rs = r[a:b, None] + r[None, :]
                ok = rsq < rs * rs
            else:
                cut = np.maximum(r[a:b, None] + r[None, :] + skin, cut_abs)
                csq = cut * cut
                ok = rsq <= csq
                near = np.abs(rsq - csq) <= BAND * csq
            if self_image:
                diag = idx[a:b, None] == idx[None, :]
                ok &= ~diag
                if not touching:
                    near &= ~diag
            if not touching:
                band += int(np.count_nonzero(near))
            ii, jj = np.nonzero(ok)
            if ii.size:
                rows = np.empty((ii.size, 5), dtype=np.int64)
                rows[:, 0] = tag[a + ii]
                rows[:, 1] = tag[jj]
                rows[:, 2:] = s
                out.append(rows)
    rows = np.concatenate(out, axis=0) if out else np.zeros((0, 5), dtype=np.int64)
    return rows, band


def as_set(rows):
    return set(map(tuple, np.asarray(rows).tolist()))


def half_count(rows):
    """what a half list with ghost atoms holds: every owned-owned pair once, every (owned atom, image) pair once"""
    rows = np.asarray(rows)
    img = np.any(rows[:, 2:] != 0, axis=1)
    n0 = int(np.count_nonzero(~img))
    assert n0 % 2 == 0
    return n0 // 2 + int(np.count_nonzero(img))


def longest_row(rows):
    rows = np.asarray(rows)
    return int(np.bincount(rows[:, 0]).max()) if len(rows) else 0


def min_image_sq(d, boxlo, boxhi, periodic):
    """|d|^2 with the minimum image taken in the periodic dimensions"""
    d = np.array(d, dtype=np.float64)
    prd = np.asarray(boxhi, dtype=np.float64) - np.asarray(boxlo, dtype=np.float64)
    for k in range(3):
        if periodic[k]:
            d[:, k] -= prd[k] * np.rint(d[:, k] / prd[k])
    return np.sum(d * d, axis=1)
