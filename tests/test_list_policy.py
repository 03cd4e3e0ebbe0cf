"""The rules that turn the statistics of a neighbour list into a choice (csrc/sf_list_policy.h: the three hysteresis bands and
who reads each in which direction, the env pins, the near-a-band predicate and the measure schedule, the non-temporal policy)
compiled into the stand-alone program tests/c_abi/list_policy_check.cpp with -fsanitize=address,undefined and run once on the
CPU: for every prior state, pin and fraction -- a sweep of thousandths, every band edge and near-a-band edge with the doubles
on both sides, a drift through each band and back -- the header decides what the engine's former if / else if ladders, written
out in the program with their literals, decide; and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_policy_header_agrees_with_the_written_out_ladders_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "list_policy_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "list_policy_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith(" 0 failures") and "FAIL" not in r.stdout
