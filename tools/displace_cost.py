"""Cost of the unwrapped-coordinate computes on the headline bed, in one process: on the 1 M-grain
Hertz bed after settling, the GPU time from HIP events of one fresh evaluation of `compute com` (one launch, fold
included), of `compute displace/atom` (one launch, four stored columns) and of the mean squared displacement as `compute
reduce avesq c_d[1] c_d[2] c_d[3]` (gather + fold over the stored columns; displace/atom is evaluated before the clock
starts), next to `compute reduce sum vx` (the figure of section 15) for scale -- median and spread of REPS evaluations after
one that allocates.  For com the bytes the kernel must move per atom are 84 (two 32-byte records, mask and tag, the 12-byte
image row gathered by tag) and the line prints the fraction of the achievable HBM bandwidth (6.3 TB/s) the measured time
corresponds to.

    python tools/displace_cost.py [--particles 1000000] [--settle 2000] [--reps 7]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COM_BYTES_PER_ATOM = 32 + 32 + 4 + 4 + 12
HBM_ACHIEVABLE = 6.3e12   # bytes / s (a float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--settle", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    lmp = bench.build_engine(bed, script)
    # (before the first run: the image counts start with the first keyword that needs them)
    for line in ("compute c all com", "compute d all displace/atom", "compute m all reduce avesq c_d[1] c_d[2] c_d[3]",
                 "compute r all reduce sum vx"):
        lmp.command(line)
    lmp.setup()
    lmp.step(args.settle)   # (settling: kernel choice, lists, a bed that has moved and been re-sorted)
    lmp.sync()
    n = int(bed["n"])
    res = {"n": n, "reps": args.reps, "wrapped_atoms": int((lmp.images() != 0).any(axis=1).sum())}
    for cid, name in (("c", "com"), ("m", "msd_by_reduce"), ("r", "reduce_sum_vx")):
        ms = [lmp.global_cost(cid) for _ in range(args.reps + 1)][1:]   # (the first evaluation allocates)
        res[name + "_gpu_ms"] = statistics.median(ms)
        res[name + "_gpu_ms_min_max"] = (min(ms), max(ms))
    ms = [lmp.compute_atom_cost("d") for _ in range(args.reps + 1)][1:]
    res["displace_atom_gpu_ms"] = statistics.median(ms)
    res["displace_atom_gpu_ms_min_max"] = (min(ms), max(ms))
    res["com_bytes_per_atom"] = COM_BYTES_PER_ATOM
    res["com_fraction_of_hbm"] = COM_BYTES_PER_ATOM * n / (res["com_gpu_ms"] * 1.0e-3) / HBM_ACHIEVABLE
    print(res)
    lmp.close()


if __name__ == "__main__":
    main()
