"""Cost of the contact rows on the headline bed: on the 1 M-grain Hertz bed after settling, the GPU
time from HIP events of count + scan + rows and, separately, of the text of every column (lines + scan + compact), next to
the restart pack -- which enumerates the same contacts -- in the same process on the same state.  Each figure is the median
and the spread of REPS evaluations after one that warms the buffers up.  Run it under `rocprofv3 --kernel-trace --stats`
(in a run of its own) for the split per kernel.

    python tools/contact_cost.py [--particles 1000000] [--steps 2000] [--reps 5] [--dir DIR]
"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    out = args.dir or tempfile.mkdtemp(prefix="sf_contact_cost_")
    lmp = bench.build_engine(bed, script)
    lmp.setup()
    lmp.step(args.steps)   # (settling: kernel choice, lists, the contacts of a bed that has moved)
    lmp.sync()
    res = {"n": int(bed["n"]), "steps": args.steps, "reps": args.reps}
    rows_ms, text_ms, pack_ms = [], [], []
    lmp.restart_cost(timing=True)
    for rep in range(args.reps + 1):
        a, b, n = lmp.contact_cost()
        lmp.write_restart(os.path.join(out, "one.sfr"))
        p = lmp.restart_cost(timing=True)[0]
        if rep:   # (the first evaluation allocates)
            rows_ms.append(a)
            text_ms.append(b)
            pack_ms.append(p)
        res["rows"] = n
    for name, v in (("rows_gpu_ms", rows_ms), ("text_gpu_ms", text_ms), ("restart_pack_gpu_ms", pack_ms)):
        res[name] = statistics.median(v)
        res[name + "_min_max"] = (min(v), max(v))
    res["contact_launches"] = lmp.contact_launches()
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
