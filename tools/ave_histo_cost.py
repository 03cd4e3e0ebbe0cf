"""Cost of fix ave/histo on the headline bed, in one process: on the 1 M-grain Hertz bed after settling,
the GPU time from HIP events of the binning of one sample (`sf_lammps_ave_histo_cost`; median and spread of REPS after one that
allocates) of `vx vy vz` into 100 bins (one pass over the velocity records and the masks, 36 B per atom); of the same on the
`force` column of a `compute pair/local` (the rows are built before the clock starts: tools/contact_cost.py times them); of the
same `vx vy vz` after `velocity all set 0 0 0`, the one-bin case in which every wave finds its lanes in one bin; and `run STEPS`
bare against `fix ave/histo 10 10 100`.  The yardstick to read the first figure against is thermo's k_thermo_reduce on the same
bed (tools/thermo_cost.py), which reads the same records.  The bed at rest is measured last: it changes the run.

    python tools/ave_histo_cost.py [--particles 1000000] [--steps 1000] [--settle 2000] [--reps 5]
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
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps}

    def cost(name, fid):
        ms = [lmp.ave_histo_cost(fid) for _ in range(args.reps + 1)][1:]   # (the first one allocates)
        res["%s_gpu_ms" % name] = statistics.median(ms)
        res["%s_gpu_ms_min_max" % name] = (min(ms), max(ms))

    def timed_run():
        t0 = time.perf_counter()
        lmp.step(args.steps)
        lmp.sync()
        return time.perf_counter() - t0

    lmp.command("compute pl all pair/local force")
    lmp.command("fix hv all ave/histo 10 10 100 -0.05 0.05 100 vx vy vz mode vector beyond end")
    lmp.command("fix hf all ave/histo 10 10 100 0 0.01 100 c_pl mode vector beyond end")
    cost("velocity", "hv")
    res["velocity_GB_per_s"] = 36.0 * res["n"] / (res["velocity_gpu_ms"] * 1.0e-3) / 1.0e9
    cost("pair_force", "hf")
    res["pair_rows"] = int(len(lmp.contacts()["tag1"]))
    lmp.command("unfix hf")
    lmp.command("unfix hv")
    res["run_bare_s"] = timed_run()
    now = int(lmp.info().nsteps)
    assert now % 100 == 0, now
    lmp.command("fix hv all ave/histo 10 10 100 -0.05 0.05 100 vx vy vz mode vector beyond end")
    before = lmp.ave_histo_launches()
    res["run_every_10_s"] = timed_run()
    after = lmp.ave_histo_launches()
    res["every_10_launches"] = after["launches"] - before["launches"]
    res["every_10_host_copies"] = after["host_copies"] - before["host_copies"]
    res["every_10_overhead"] = res["run_every_10_s"] / res["run_bare_s"] - 1.0
    out = lmp.ave_histo("hv")
    res["last_total_missing"] = (out["total"], out["missing"])
    lmp.command("velocity all set 0 0 0")
    cost("one_bin", "hv")
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
