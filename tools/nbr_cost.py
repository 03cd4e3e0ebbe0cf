"""Cost of the cutoff-grid walk on the headline bed, in one process: on the 1 M-grain Hertz bed after
settling, the GPU time from HIP events of (grid build, walk) for `compute rdf 100 cutoff 3 d` and for `compute coord/atom
cutoff 3 d` (median and spread of REPS evaluations after one that allocates), and `run STEPS` bare and with `fix ave/time 100 10
1000 c_rdf[2] mode vector`.  The yardstick to read the walk against is the rebuild's list build on the same bed (297 us,
DESIGN.md section 6 item 2): it walks the same kind of grid for a cutoff of about one diameter, and the rdf walk visits roughly
(3 d / list cutoff)^3 times as many candidates.

Every GPU step runs under a time limit of its own: a step that overruns it ends the process with status 124 and nothing more is
started on the GPU.

    python tools/nbr_cost.py [--particles 1000000] [--steps 1000] [--settle 2000] [--reps 5]
"""
import argparse
import contextlib
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextlib.contextmanager
def limit(seconds, what):
    # (a watchdog thread, not a signal: the main thread may sit in a library call that never returns)
    def overrun():
        print("nbr_cost: %s ran past its limit of %d s: stopping" % (what, seconds), flush=True)
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
    ap.add_argument("--steps", type=int, default=1000)
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
        lmp.step(args.settle)   # (settling: kernel choice, lists, the contacts of a bed that has moved)
        lmp.sync()
    d = float(bed["diameter"].max())
    lmp.command("compute rdf all rdf 100 cutoff %.17g" % (3.0 * d))
    lmp.command("compute coord all coord/atom cutoff %.17g" % (3.0 * d))
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps, "cutoff": 3.0 * d}
    for cid in ("rdf", "coord"):
        with limit(120, "the evaluations of compute " + cid):
            ms = [lmp.nbr_cost(cid) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
        for k, part in enumerate(("grid", "walk")):
            res["%s_%s_gpu_ms" % (cid, part)] = statistics.median(m[k] for m in ms)
            res["%s_%s_gpu_ms_min_max" % (cid, part)] = (min(m[k] for m in ms), max(m[k] for m in ms))
    with limit(60, "the counts of compute rdf"):
        res["rdf_pairs_counted"] = int(lmp.rdf_counts("rdf")["counts"].sum())

    def timed_run(what):
        with limit(300, what):
            t0 = time.perf_counter()
            lmp.step(args.steps)
            lmp.sync()
            return time.perf_counter() - t0

    res["run_bare_s"] = timed_run("the bare run")
    now = int(lmp.info().nsteps)
    assert now % 1000 == 0, now
    lmp.command("fix t all ave/time 100 10 1000 c_rdf[2] mode vector")
    before = lmp.nbr_launches()
    res["run_ave_time_s"] = timed_run("the run with fix ave/time mode vector")
    after = lmp.nbr_launches()
    res["ave_time_grid_builds"] = after["grid_builds"] - before["grid_builds"]
    res["ave_time_host_copies"] = after["host_copies"] - before["host_copies"]
    res["ave_time_overhead"] = res["run_ave_time_s"] / res["run_bare_s"] - 1.0
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
