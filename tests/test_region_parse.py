"""The parser and table of `region` (csrc/sf_region_parse.h, host-only) and the predicate region_match
(csrc/sf_region_match.h) compiled into the stand-alone program tests/c_abi/region_parse_check.cpp with
-fsanitize=address,undefined and -ffp-contract=off and run once on the CPU: well- and ill-formed lines of every style and
keyword, INF and EDGE, delete, the flattening of nested unions up to the 17-primitive overflow, and region_match at the
boundary points of every primitive.  Every case gives what is expected of it and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_and_predicate_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "region_parse_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "c_abi", "region_parse_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("0 failures") and "FAIL" not in r.stdout
