"""What fix rigid/nve costs: sub-steps per second of
  * the 21 780-sphere lattice block of tests/test_rigid_gpu.py under `rigid/nve single`,
  * a bed of N spheres (default 1 M) in 4-sphere clumps under `rigid/nve molecule`, next to the same bed under
    `fix nve/sphere`.
usage: python tools/rigid_cost.py [--n 1000000] [--steps 200] [--json]
A per-kernel split comes from running this under `rocprofv3 --kernel-trace --stats -- python tools/rigid_cost.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sedifoam_amd import Lammps  # noqa: E402


def engine(x, d, rho, lo, hi, periodic, dt, skin, pair):
    lmp = Lammps()
    lmp.set_box(lo, hi)
    lmp.create_atoms(x, np.full(len(x), d), np.full(len(x), rho))
    for line in ("atom_style sphere", "boundary %s %s %s" % tuple("p" if q else "f" for q in periodic), "newton off",
                 "communicate single vel yes", "neighbor %.17g bin" % skin, "neigh_modify delay 0", "pair_style " + pair,
                 "pair_coeff * *", "timestep %.17g" % dt, "fix g all gravity 9.81 vector 0 -1 0"):
        lmp.command(line)
    return lmp


def rate(lmp, steps):
    lmp.step(20)   # setup, first rebuilds
    lmp.sync()
    t0 = time.perf_counter()
    lmp.step(steps)
    lmp.sync()
    return steps / (time.perf_counter() - t0)


def block(steps):
    s, d = 0.000606, 0.0005
    i, j, k = np.meshgrid(np.arange(33), np.arange(20), np.arange(33), indexing="ij")
    x = np.stack([i.ravel() * s + 0.003, j.ravel() * s + 0.5 * d + 2.0e-6, k.ravel() * s + 0.003], axis=1)
    lmp = engine(x, d, 2650.0, [0.0, -0.001, 0.0], [0.026, 0.02, 0.026], (0, 0, 0), 1e-6, 0.0002,
                 "gran/hooke/history 150.0 NULL 0.0 NULL 0.4 0")
    lmp.command("fix 1 all rigid/nve single")
    lmp.command("fix w all wall/gran 150.0 NULL 0.0 NULL 0.4 0 yplane 0.0 NULL")
    return rate(lmp, steps)


def clump_bed(n, steps, rigid):
    """a cubic lattice of touching spheres (d 1 mm), every 2 x 2 x 1 cell of it one clump"""
    d = 1.0e-3
    m = int(round((n / 4) ** (1.0 / 3.0)))
    nx, ny, nz = 2 * m, 2 * m, max(1, n // (4 * m * m))
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    x = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) * d + 0.5 * d
    mol = ((i // 2) + (nx // 2) * ((j // 2) + (ny // 2) * k)).ravel() + 1
    lmp = engine(x, d * 0.999, 2650.0, [0, 0, 0], [nx * d, ny * d * 1.5, nz * d], (1, 0, 1), 1e-6, 0.25e-3,
                 "gran/hooke/history 2.0e4 NULL 50.0 NULL 0.4 1")
    lmp.command("fix w all wall/gran 2.0e4 NULL 50.0 NULL 0.4 1 yplane 0.0 NULL")
    if rigid:
        lmp.set_molecule(np.arange(1, len(x) + 1), mol)
        lmp.command("fix 1 all rigid/nve molecule")
    else:
        lmp.command("fix 1 all nve/sphere")
    return len(x), rate(lmp, steps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    out = {"block_21780_single_substeps_per_s": block(a.steps)}
    n, r = clump_bed(a.n, a.steps, True)
    out["clump_bed_atoms"] = n
    out["clump_bed_rigid_molecule_substeps_per_s"] = r
    out["clump_bed_nve_sphere_substeps_per_s"] = clump_bed(a.n, a.steps, False)[1]
    print(json.dumps(out) if a.json else "\n".join("%-44s %s" % kv for kv in out.items()))
