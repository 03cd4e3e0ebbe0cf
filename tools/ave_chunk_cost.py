"""Cost of binned profiles on the headline bed, in one process: on the 1 M-grain Hertz bed after
settling, the GPU time from HIP events of one sample of `fix ave/chunk` on a 1-D y profile of about 50 chunks -- assign, sort +
segment offsets, sums + fold; median and spread of REPS samples after one that allocates -- with `vx vy vz density/number`
and again with `c_s[1] .. c_s[6]` added (the evaluation of stress/atom itself is outside the time: tools/compute_atom_cost.py
has it), and `run STEPS` in three arms: bare; cut at every tenth step by pieces that write nothing (`step(10)` repeated); with
the fix sampling at every tenth step and writing one output at the end (`10 STEPS/10 STEPS`).  The second arm separates what
cutting the queued batch costs from what the kernels cost.

    python tools/ave_chunk_cost.py [--particles 1000000] [--steps 1000] [--settle 2000] [--reps 5] [--chunks 50]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=50)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    lmp = bench.build_engine(bed, script)
    lmp.setup()
    lmp.step(args.settle)   # (settling: kernel choice, lists, the contacts of a bed that has moved)
    lmp.sync()
    top = float(bed["x"][:, 1].max()) + 0.5 * float(bed["diameter"].max())
    delta = top / args.chunks
    lmp.command("compute s all stress/atom")
    lmp.command("compute cy all chunk/atom bin/1d y lower %r units box bound y lower %r" % (delta, top))
    few = "vx vy vz density/number"
    many = few + " " + " ".join("c_s[%d]" % k for k in range(1, 7))
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps}
    step0 = int(lmp.info().nsteps)
    far = 1000000 * (step0 // 1000000 + 1)   # (a schedule beyond every run here: the cost query samples on its own)
    for fid, vals in (("few", few), ("many", many)):
        lmp.command("fix %s all ave/chunk %d 1 %d cy %s" % (fid, far, far, vals))
        ms = [lmp.ave_chunk_cost(fid) for _ in range(args.reps + 1)][1:]   # (the first sample allocates)
        for k, part in enumerate(("assign", "sort", "sums")):
            col = [m[k] for m in ms]
            res["%s_%s_gpu_ms" % (fid, part)] = statistics.median(col)
            res["%s_%s_gpu_ms_min_max" % (fid, part)] = (min(col), max(col))
        lmp.command("unfix " + fid)
    t0 = time.perf_counter()
    lmp.step(args.steps)
    lmp.sync()
    res["run_bare_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(args.steps // 10):
        lmp.step(10)
    lmp.sync()
    res["run_cut_every_10_s"] = time.perf_counter() - t0
    now = int(lmp.info().nsteps)
    assert now % 10 == 0
    lmp.command("fix p all ave/chunk 10 %d %d cy %s" % (args.steps // 10, args.steps, many))
    before = lmp.ave_chunk_launches()
    t0 = time.perf_counter()
    lmp.step(args.steps)
    lmp.sync()
    res["run_with_fix_s"] = time.perf_counter() - t0
    res["fix_launches"] = lmp.ave_chunk_launches() - before
    try:
        res["fix_output_step"] = lmp.ave_chunk("p")["step"]
    except Exception as ex:   # (a step count that is no multiple of Nfreq: no output fell into the run)
        res["fix_output_step"] = str(ex)
    res["cut_overhead"] = res["run_cut_every_10_s"] / res["run_bare_s"] - 1.0
    res["fix_overhead"] = res["run_with_fix_s"] / res["run_bare_s"] - 1.0
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
