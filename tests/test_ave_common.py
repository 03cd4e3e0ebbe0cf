"""What fix ave/chunk, fix ave/time and fix ave/histo share on the host (csrc/sf_ave_common.h: the sample schedule, the output
file, the file / ave / start keywords and the c_ID[k] parser) compiled into the stand-alone program
tests/c_abi/ave_common_check.cpp with -fsanitize=address,undefined and run once on the CPU: the schedule agrees with a
brute-force statement of the LAMMPS rule for every Nevery Nrepeat Nfreq with Nfreq <= 12, the files hold the bytes expected of
them, and neither sanitizer reports anything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_file_and_keywords_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ave_common_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "ave_common_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith(" 0 failures") and "FAIL" not in r.stdout
