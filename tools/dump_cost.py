"""Cost of `dump custom` on the headline bed (DESIGN.md, section "Particle snapshots"): `run 1000` with one frame of the
reference's ten columns against the same run without a dump, in one process, and the same frame formatted by a host
snprintf loop.  The formatter + compaction kernel times come from running this script under
`rocprofv3 --kernel-trace --stats`.

    python tools/dump_cost.py [--particles 1000000] [--steps 1000] [--reps 2]
"""
import argparse
import ctypes as C
import ctypes.util
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = "id type diameter mass x y z vx vy vz"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import bench
    from sedifoam_amd import synthetic
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(args.particles), seed=12345 + 3)
    script = synthetic.hertz_script(bed, **bench.KW)
    out = tempfile.mkdtemp(prefix="sf_dump_cost_")
    path = os.path.join(out, "snapshot")
    res = {"n": int(bed["n"]), "steps": args.steps}
    times = {"plain": [], "dump": []}
    for rep in range(args.reps):
        for mode in ("plain", "dump"):
            lmp = bench.build_engine(bed, script)
            if mode == "dump":
                # frames at 0 and `steps` before the timed run (they allocate the device scratch and both pinned
                # buffers); the timed run holds one frame, in the buffer of the frame at 0
                lmp.command("dump d all custom %d %s %s" % (args.steps, path, COLS))
            lmp.setup()
            lmp.step(2 * args.steps - 1)   # (warm-up: kernel choice, lists)
            lmp.sync()
            t0 = time.perf_counter()
            lmp.step(args.steps)
            lmp.sync()   # (the frame is in its file)
            times[mode].append(time.perf_counter() - t0)
            lmp.close()
    res["run_plain_s"] = min(times["plain"])
    res["run_dump_s"] = min(times["dump"])
    res["dump_overhead"] = res["run_dump_s"] / res["run_plain_s"] - 1.0
    data = open(path, "rb").read().split(b"ITEM: TIMESTEP\n")[-1]
    data = b"ITEM: TIMESTEP\n" + data
    res["frame_bytes"] = len(data)
    # the same rows through the host's snprintf, one thread
    rows = np.array([[float(t) for t in ln.split()] for ln in data.split(b"\n")[9:9 + 20000]])
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_double]
    buf = C.create_string_buffer(64)
    flat = rows[:, 2:].ravel().tolist()
    t0 = time.perf_counter()
    for v in flat:
        libc.snprintf(buf, 64, b"%g ", v)
    per_value_ctypes = (time.perf_counter() - t0) / len(flat)
    res["host_ctypes_snprintf_us_per_value"] = per_value_ctypes * 1e6
    # host C loop (the cost a host-formatted dump would pay): compiled on the fly when a C compiler is there
    res["host_c_snprintf_frame_s"] = host_c_loop(rows, int(bed["n"]))
    print(res)


def host_c_loop(rows, n):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        return None
    d = tempfile.mkdtemp()
    src = os.path.join(d, "f.c")
    open(src, "w").write(r"""
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
int main(int argc, char** argv) {
  long n = atol(argv[1]), m = atol(argv[2]);
  double* v = malloc(sizeof(double) * m * 8);
  FILE* f = fopen(argv[3], "rb");
  if (fread(v, sizeof(double), m * 8, f) != (size_t)(m * 8)) return 1;
  fclose(f);
  char* out = malloc((size_t)n * 160);
  struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
  size_t p = 0;
  for (long i = 0; i < n; i++) {
    const double* r = v + 8 * (i % m);
    p += sprintf(out + p, "%ld %d ", i + 1, 1);
    for (int k = 0; k < 8; k++) p += sprintf(out + p, "%g ", r[k]);
    out[p++] = '\n';
  }
  clock_gettime(CLOCK_MONOTONIC, &b);
  printf("%.6f %zu\n", (b.tv_sec - a.tv_sec) + 1e-9 * (b.tv_nsec - a.tv_nsec), p);
  return 0;
}
""")
    exe = os.path.join(d, "f")
    if subprocess.run([cc, "-O2", "-o", exe, src]).returncode:
        return None
    vals = os.path.join(d, "v.bin")
    np.ascontiguousarray(rows[:, 2:]).tofile(vals)
    r = subprocess.run([exe, str(n), str(rows.shape[0]), vals], capture_output=True, text=True)
    return float(r.stdout.split()[0])


if __name__ == "__main__":
    main()
