"""The parsers of `compute chunk/atom c_CID` and of the per-chunk computes (csrc/sf_pchunk_parse.h, host-only), the checks of
the column behind c_CID and of CHUNKID, and the rows_vary rule of fix ave/time mode vector (csrc/sf_compute_ref.h) compiled into
the stand-alone program tests/c_abi/pchunk_parse_check.cpp with -fsanitize=address,undefined and run once on the CPU over every
accepted and every refused form: every case gives what is expected of it and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parsers_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "pchunk_parse_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "pchunk_parse_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("0 failures") and "FAIL" not in r.stdout
