"""The parser of `compute cluster/atom` (csrc/sf_nbr_parse.h, host-only), the by-name refusal of fragment/atom and
aggregate/atom, and the words of `compute cluster/stats` (csrc/sf_global_parse.h) compiled into the stand-alone program
tests/c_abi/cluster_parse_check.cpp with -fsanitize=address,undefined and run once on the CPU over every accepted form and
every illegal form: every case gives what is expected of it and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parsers_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "cluster_parse_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "cluster_parse_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("0 failures") and "FAIL" not in r.stdout
