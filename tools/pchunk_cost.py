"""Cost of the per-floc chain on the headline bed, in one process: on the 1 M-grain Hertz bed after
settling,

    compute cl all cluster/atom CUT
    compute cc all chunk/atom c_cl compress yes
    compute n  all property/chunk cc count id
    compute vc all vcm/chunk cc
    compute rg all gyration/chunk cc
    compute xc all com/chunk cc

at a cut that leaves every grain alone and at one that joins the bed into a percolating cluster: the GPU time from HIP events
of compute cluster/atom (grid build, everything after the grid) and of everything after it (the sort, the renumbering, the wait
for the 4 bytes of Nchunk, the segmented sums of the four per-chunk computes and their finish), median and spread of REPS
evaluations after one that allocates, Nchunk, the largest chunk and the launches of one evaluation.

Every GPU step runs under a time limit of its own: a step that overruns it ends the process with status 124 and nothing more is
started on the GPU.

    python tools/pchunk_cost.py [--particles 1000000] [--settle 2000] [--reps 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cluster_cost import limit   # noqa: E402


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
    d = float(bed["diameter"].max())
    cases = (("singlets_0.5d", 0.5 * d), ("percolating_1.1d", 1.1 * d))
    for k, (name, cut) in enumerate(cases):   # (before the setup: com and gyration count the periodic wraps from here)
        cl, cc = "cl%d" % k, "cc%d" % k
        lmp.command("compute %s all cluster/atom %.17g" % (cl, cut))
        lmp.command("compute %s all chunk/atom c_%s compress yes" % (cc, cl))
        lmp.command("compute n%d all property/chunk %s count id" % (k, cc))
        lmp.command("compute vc%d all vcm/chunk %s" % (k, cc))
        lmp.command("compute rg%d all gyration/chunk %s" % (k, cc))
        lmp.command("compute xc%d all com/chunk %s" % (k, cc))
    with limit(120, "setup and settling"):
        lmp.setup()
        lmp.step(args.settle)
        lmp.sync()
    res = {"n": int(bed["n"]), "reps": args.reps}
    for k, (name, cut) in enumerate(cases):
        cl, cc = "cl%d" % k, "cc%d" % k
        with limit(180, "the evaluations of compute cluster/atom " + name):
            cms = [lmp.nbr_cost(cl) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
        with limit(180, "the evaluations of the chain over " + name):
            before = lmp.chunk_info(cc)
            ms = [lmp.chunk_cost(cc) for _ in range(args.reps + 1)][1:]
            after = lmp.chunk_info(cc)
            count = lmp.compute_array("n%d" % k)[:, 0]
        out = {"cut": cut, "nchunk": after["nchunk"], "largest": float(count.max()) if len(count) else 0.0,
               "launches_per_evaluation": (after["launches"] - before["launches"]) // (args.reps + 1),
               "host_copies_per_evaluation": (after["host_copies"] - before["host_copies"]) // (args.reps + 1)}
        for j, part in enumerate(("grid", "cluster")):
            out[part + "_gpu_ms"] = statistics.median(m[j] for m in cms)
            out[part + "_gpu_ms_min_max"] = (min(m[j] for m in cms), max(m[j] for m in cms))
        out["chain_gpu_ms"] = statistics.median(ms)
        out["chain_gpu_ms_min_max"] = (min(ms), max(ms))
        res[name] = out
        print(name, out, flush=True)
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
