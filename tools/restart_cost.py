"""Cost of checkpoints on the headline bed: one `write_restart` (file size, GPU time of the pack from
HIP events, host time until the pinned copy has landed and until the file is renamed) and `run STEPS` with
`restart EVERY` against the same run without a `restart` line, interleaved in one process.  Run it under
`rocprofv3 --kernel-trace --stats` for the timeline: the k_substep launches that follow a pack start while the writer
thread still works on the file.

    python tools/restart_cost.py [--particles 1000000] [--steps 2000] [--every 1000] [--reps 2] [--dir DIR]
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
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import restart, synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    out = args.dir or tempfile.mkdtemp(prefix="sf_restart_cost_")
    res = {"n": int(bed["n"]), "steps": args.steps, "every": args.every}
    times = {"plain": [], "restart": [], "queued": []}
    for rep in range(args.reps):
        for mode in ("plain", "restart"):
            lmp = bench.build_engine(bed, script)
            lmp.setup()
            lmp.step(args.steps)   # (warm-up: kernel choice, lists)
            lmp.sync()
            if mode == "restart":
                if rep == 0:
                    lmp.restart_cost(timing=True)
                    f = os.path.join(out, "one.sfr")
                    t0 = time.perf_counter()
                    lmp.write_restart(f)
                    res["write_restart_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    res["pack_gpu_ms"], res["pinned_copy_landed_ms"], res["file_renamed_ms"] = lmp.restart_cost(timing=False)
                    h = restart.header(f)
                    res["file_bytes"] = os.path.getsize(f)
                    res["contacts"] = h["ncontacts"]
                    res["bytes_per_atom"] = res["file_bytes"] / h["natoms"]
                    res["restart_launches_one"] = lmp.restart_launches()
                lmp.command("restart %d %s/a %s/b" % (args.every, out, out))
            t0 = time.perf_counter()
            lmp.step(args.steps)
            t1 = time.perf_counter()   # (every sub-step queued and done; the last checkpoint may still be on its way)
            lmp.sync()
            t2 = time.perf_counter()
            times[mode].append(t2 - t0)
            if mode == "restart":
                times["queued"].append(t1 - t0)
            lmp.close()
    res["plain_s"] = min(times["plain"])
    res["restart_s"] = min(times["restart"])
    res["restart_steps_done_s"] = min(times["queued"])
    res["overhead"] = res["restart_s"] / res["plain_s"] - 1.0
    res["overhead_until_steps_done"] = res["restart_steps_done_s"] / res["plain_s"] - 1.0
    print(res)


if __name__ == "__main__":
    main()
