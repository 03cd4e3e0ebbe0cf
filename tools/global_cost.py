"""Cost of global computes and fix ave/time on the headline bed, in one process: on the 1 M-grain Hertz
bed after settling, the GPU time from HIP events of one fresh evaluation of `compute reduce sum vx vy vz fx fy fz` (six atom
columns: one gather over the velocity and force records, 64 B per atom, and one fold; median and spread of REPS evaluations
after one that allocates), of `compute ke` next to it, and `run STEPS` in three arms: bare; with `fix ave/time 1 10 10` (a
sample at every step, an output at every tenth); with `fix ave/time 10 10 100` (a sample at every tenth step).  The yardstick
to read the first figure against is thermo's k_thermo_reduce pair on the same bed (tools/thermo_cost.py), which reads the same
64 B per atom.

    python tools/global_cost.py [--particles 1000000] [--steps 1000] [--settle 2000] [--reps 5]
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
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    lmp = bench.build_engine(bed, script)
    lmp.setup()
    lmp.step(args.settle)   # (settling: kernel choice, lists, the contacts of a bed that has moved)
    lmp.sync()
    lmp.command("compute six all reduce sum vx vy vz fx fy fz")
    lmp.command("compute K all ke")
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps}
    for cid in ("six", "K"):
        ms = [lmp.global_cost(cid) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
        res["%s_gpu_ms" % cid] = statistics.median(ms)
        res["%s_gpu_ms_min_max" % cid] = (min(ms), max(ms))
    res["six_GB_per_s"] = 64.0 * res["n"] / (res["six_gpu_ms"] * 1.0e-3) / 1.0e9

    def timed_run():
        t0 = time.perf_counter()
        lmp.step(args.steps)
        lmp.sync()
        return time.perf_counter() - t0

    res["run_bare_s"] = timed_run()
    for name, sched in (("every_step", "1 10 10"), ("every_10", "10 10 100")):
        now = int(lmp.info().nsteps)
        assert now % 100 == 0, now
        lmp.command("fix t all ave/time %s c_six[1] c_six[2] c_six[3] c_six[4] c_six[5] c_six[6] c_K" % sched)
        before = lmp.global_launches()
        res["run_%s_s" % name] = timed_run()
        after = lmp.global_launches()
        res["%s_launches" % name] = after["launches"] - before["launches"]
        res["%s_host_copies" % name] = after["host_copies"] - before["host_copies"]
        res["%s_overhead" % name] = res["run_%s_s" % name] / res["run_bare_s"] - 1.0
        lmp.command("unfix t")
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
