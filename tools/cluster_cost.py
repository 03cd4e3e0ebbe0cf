"""Cost of `compute cluster/atom` on the headline bed, in one process: on the 1 M-grain Hertz bed after
settling, for `surface no` at 1.1 and 3 diameters and `surface yes` at a gap of 0.05 diameter, the GPU time from HIP events of
(grid build, everything after the grid: hook, compress and verify rounds with their 4-byte copies, tally, store), median and
spread of REPS evaluations after one that allocates, the verify rounds, the number of clusters and the largest one; and next to
each the walk of a `compute coord/atom` at the cutoff of the same grid -- one pass over the same edges, which is the yardstick.

Every GPU step runs under a time limit of its own: a step that overruns it ends the process with status 124 and nothing more is
started on the GPU.

    python tools/cluster_cost.py [--particles 1000000] [--settle 2000] [--reps 5]
"""
import argparse
import contextlib
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextlib.contextmanager
def limit(seconds, what):
    # (a watchdog thread, not a signal: the main thread may sit in a library call that never returns)
    def overrun():
        print("cluster_cost: %s ran past its limit of %d s: stopping" % (what, seconds), flush=True)
        os._exit(124)
    watchdog = threading.Timer(seconds, overrun)
    watchdog.daemon = True
    watchdog.start()
    try:
        yield
    finally:
        watchdog.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    with limit(120, "the build of the engine"):
        lmp = bench.build_engine(bed, script)
        lmp.setup()
    with limit(120, "settling"):
        lmp.step(args.settle)
        lmp.sync()
    d = float(bed["diameter"].max())
    cases = [("centre_1.1d", "%.17g size yes" % (1.1 * d), 1.1 * d),
             ("centre_3d", "%.17g size yes" % (3.0 * d), 3.0 * d),
             ("surface_0.05d", "%.17g surface yes size yes" % (0.05 * d), d + 0.05 * d)]
    res = {"n": int(bed["n"]), "reps": args.reps}
    for k, (name, words, grid_cut) in enumerate(cases):
        cl, st, co = "cl%d" % k, "st%d" % k, "co%d" % k
        lmp.command("compute %s all cluster/atom %s" % (cl, words))
        lmp.command("compute %s all cluster/stats %s" % (st, cl))
        lmp.command("compute %s all coord/atom cutoff %.17g" % (co, grid_cut))
        with limit(180, "the evaluations of compute cluster/atom " + name):
            ms = [lmp.nbr_cost(cl) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
            rounds = lmp.cluster_rounds(cl)
        with limit(120, "the evaluations of compute coord/atom at the cutoff of " + name):
            cms = [lmp.nbr_cost(co) for _ in range(args.reps + 1)][1:]
        with limit(60, "compute cluster/stats of " + name):
            stats = lmp.compute_global(st).tolist()
        out = {"grid_cutoff": grid_cut, "verify_rounds": rounds, "clusters": stats[0], "largest": stats[1], "atoms": stats[2]}
        for j, part in enumerate(("grid", "cluster")):
            out[part + "_gpu_ms"] = statistics.median(m[j] for m in ms)
            out[part + "_gpu_ms_min_max"] = (min(m[j] for m in ms), max(m[j] for m in ms))
        out["coord_walk_gpu_ms"] = statistics.median(m[1] for m in cms)
        out["coord_walk_gpu_ms_min_max"] = (min(m[1] for m in cms), max(m[1] for m in cms))
        res[name] = out
        print(name, out, flush=True)
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
