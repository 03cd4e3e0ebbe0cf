"""Cost of thermo output on the headline bed (DESIGN.md, section "Thermo output"): `run 1000` with `thermo 100` against the
same run without a destination, and 20 x lammps_step(50) with and without output (two lines per step call), in one
process.  The kernel times of k_thermo_virial and k_thermo_reduce next to k_substep come from running this script under
`rocprofv3 --kernel-trace --stats`.

    python tools/thermo_cost.py [--particles 1000000] [--steps 1000] [--every 100] [--reps 2]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    log = os.path.join(tempfile.mkdtemp(prefix="sf_thermo_cost_"), "log.lammps")
    res = {"n": int(bed["n"]), "steps": args.steps, "every": args.every}
    times = {k: [] for k in ("plain", "thermo", "step_plain", "step_thermo")}
    for rep in range(args.reps):
        for mode in ("plain", "thermo"):
            lmp = bench.build_engine(bed, script)
            if mode == "thermo":
                lmp.commands("log %s\nthermo_style one\nthermo %d" % (log, args.every))
            lmp.setup()
            lmp.step(2 * args.steps - 1)   # (warm-up: kernel choice, lists, the thermo buffers)
            lmp.sync()
            t0 = time.perf_counter()
            lmp.step(args.steps)
            lmp.sync()
            times[mode].append(time.perf_counter() - t0)
            # the coupling loop's shape: lammps_step(50) twenty times, a line at the setup and the end of each
            t0 = time.perf_counter()
            for _ in range(20):
                lmp.step(50)
            lmp.sync()
            times["step_" + mode].append(time.perf_counter() - t0)
            if mode == "thermo":
                res["thermo_launches"] = lmp.thermo_launches()
            lmp.close()
    for k, v in times.items():
        res[k + "_s"] = min(v)
    res["thermo_overhead"] = res["thermo_s"] / res["plain_s"] - 1.0
    res["step_thermo_overhead"] = res["step_thermo_s"] / res["step_plain_s"] - 1.0
    lines = args.steps // args.every + 1
    res["per_line_ms"] = (res["thermo_s"] - res["plain_s"]) / lines * 1e3
    print(res)


if __name__ == "__main__":
    main()
