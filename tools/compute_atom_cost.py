"""Cost of the per-atom computes on the headline bed, in one process: on the 1 M-grain Hertz bed
after settling, the GPU time from HIP events of one fresh evaluation of stress/atom, contact/atom and ke/atom (median and
spread of REPS evaluations after one that allocates), and `run STEPS` without a dump against the same run with ONE frame of
`id x y z c_s[1] ... c_s[6] c_c` at its last step.  Thermo output is on (`thermo_style one`, a line every 100 steps), so
that under `rocprofv3 --kernel-trace --stats` the trace shows k_atom_virial<2> next to k_thermo_virial<2, false> -- the
same gathers and law, six block partials instead of 48 bytes per atom of stores -- and k_substep of the same process.

    python tools/compute_atom_cost.py [--particles 1000000] [--steps 1000] [--settle 2000] [--reps 5] [--dir DIR]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    out = args.dir or tempfile.mkdtemp(prefix="sf_compute_atom_cost_")
    lmp = bench.build_engine(bed, script)
    lmp.commands("log %s\nthermo_style one\nthermo 100" % os.path.join(out, "log.lammps"))
    lmp.command("compute s all stress/atom")
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    lmp.setup()
    lmp.step(args.settle)   # (settling: kernel choice, lists, the contacts of a bed that has moved)
    lmp.sync()
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps}
    for cid, name in (("s", "stress_atom"), ("c", "contact_atom"), ("k", "ke_atom")):
        ms = [lmp.compute_atom_cost(cid) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
        res[name + "_gpu_ms"] = statistics.median(ms)
        res[name + "_gpu_ms_min_max"] = (min(ms), max(ms))
    t0 = time.perf_counter()
    lmp.step(args.steps)
    lmp.sync()
    res["run_plain_s"] = time.perf_counter() - t0
    end = int(lmp.info().nsteps) + args.steps   # (a dump every `end` steps: one frame, at the last step of the run)
    lmp.command("dump d all custom %d %s id x y z %s c_c" % (
        end, os.path.join(out, "one.dump"), " ".join("c_s[%d]" % k for k in range(1, 7))))
    before = lmp.compute_atom_launches()
    t0 = time.perf_counter()
    lmp.step(args.steps)
    lmp.sync()
    res["run_one_frame_s"] = time.perf_counter() - t0
    res["frame_launches"] = lmp.compute_atom_launches() - before
    res["frame_bytes"] = os.path.getsize(os.path.join(out, "one.dump"))
    res["one_frame_overhead"] = res["run_one_frame_s"] / res["run_plain_s"] - 1.0
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
