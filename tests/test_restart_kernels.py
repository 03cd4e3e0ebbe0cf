"""The checkpoint kernels (csrc/sf_restart.hip) compiled for gfx950 keep everything in registers: no scratch
(hipcc -Rpass-analysis=kernel-resource-usage, the table tests/kernel_resources.py prints for the sub-step kernels)."""
import os
import re
import subprocess

from sedifoam_amd import build


def test_restart_kernels_use_no_scratch(tmp_path):
    src = os.path.join(build.CSRC, "sf_restart.hip")
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "r.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {n: s for n, s in zip(names, scratch) if "k_rst_" in n}
    assert len(kernels) >= 8, names
    assert all(s == 0 for s in kernels.values()), kernels
