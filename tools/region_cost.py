"""Cost of the update of dynamic region groups, in one process: GPU time from HIP events
(`sf_lammps_region_cost`; median and spread of REPS after one that allocates) of the one launch that evaluates one and eight
dynamic groups, on the 108-grain bed of the tests and on the 1 M-grain headline bed after settling.  The eight groups: four
slabs, a sphere, a cylinder, a half space and a nested union.  Each figure is taken twice: `fresh` on groups that have never
been evaluated (every member's mask word changes and is stored) and `steady` after an update (no word changes: no store).
The yardstick: the launch streams 36 B in and at most 4 B out per atom; 40 B per atom at the achievable HBM rate is the floor.

    python tools/region_cost.py [--particles 1000000] [--settle 2000] [--reps 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def regions(bed):
    lo, hi = [float(v) for v in bed["boxlo"]], [float(v) for v in bed["boxhi"]]
    top = float(bed["x"][:, 1].max())
    mid = [0.5 * (a + b) for a, b in zip(lo, hi)]
    r = 0.25 * (hi[0] - lo[0])
    out = ["region r0 block INF INF %.17g INF INF INF units box" % (0.5 * top)]
    for k in range(1, 4):
        out.append("region r%d block INF INF %.17g %.17g INF INF units box" % (k, 0.25 * (k - 1) * top, 0.25 * k * top))
    out += ["region r4 sphere %.17g %.17g %.17g %.17g units box" % (mid[0], 0.5 * top, mid[2], r),
            "region r5 cylinder y %.17g %.17g %.17g INF INF side out units box" % (mid[0], mid[2], r),
            "region r6 plane %.17g %.17g %.17g 1 1 0 units box" % (mid[0], 0.5 * top, mid[2]),
            "region r7a intersect 2 r0 r5 units box", "region r7 union 2 r7a r4 side out units box"]
    return out


def measure(lmp, bed, reps, res, label):
    for line in regions(bed):
        lmp.command(line)
    n = int(lmp.get_local_n())

    def cost(name, group):
        ms = [lmp.region_cost(group) for _ in range(reps + 1)][1:]   # (the first one allocates)
        med = statistics.median(ms)
        res["%s_%s_gpu_us" % (label, name)] = 1.0e3 * med
        res["%s_%s_gpu_us_min_max" % (label, name)] = (1.0e3 * min(ms), 1.0e3 * max(ms))
        res["%s_%s_GB_per_s_at_40B" % (label, name)] = 40.0 * n / (med * 1.0e-3) / 1.0e9

    lmp.command("group g0 dynamic all region r0")
    cost("one_fresh", None)
    lmp.step(0)                                           # (the first piece after the definition evaluates)
    res["%s_one_members" % label] = lmp.group_count("g0")
    cost("one_steady", None)
    for k in range(1, 8):
        lmp.command("group g%d dynamic all region r%d" % (k, k))
    cost("eight_seven_fresh", None)
    lmp.step(0)
    res["%s_eight_members" % label] = [lmp.group_count("g%d" % k) for k in range(8)]
    cost("eight_steady", None)
    cost("one_of_eight_steady", "g0")
    res["%s_n" % label] = n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    from tests import dem_cases as dc
    from tests.test_contacts_gpu import _small
    res = {"reps": args.reps}
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 0")
    measure(lmp, bed, args.reps, res, "small")
    lmp.close()
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    lmp = bench.build_engine(bed, synthetic.hertz_script(bed, **bench.KW))
    lmp.setup()
    lmp.step(args.settle)
    lmp.sync()
    measure(lmp, bed, args.reps, res, "bench")
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
