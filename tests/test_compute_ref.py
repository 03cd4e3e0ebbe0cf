"""What every reader of a `c_ID` / `c_ID[k]` word accepts of a compute of each kind (csrc/sf_compute_ref.h, host-only), compiled
into the stand-alone program tests/c_abi/compute_ref_check.cpp with -fsanitize=address,undefined and run once on the CPU: for
every kind and shape of compute, every index and every reader the text is the one the reader's own check gave before the
rules moved into that header, and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compute_reference_rules_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "compute_ref_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "compute_ref_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith(" 0 failures") and "FAIL" not in r.stdout
