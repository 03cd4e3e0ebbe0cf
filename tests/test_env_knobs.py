"""sedifoam_amd/csrc/sf_env.h, the one reader of the SF_* knobs: every idiom gives what the spelling it replaced gave,
for an unset variable, "0", "1", the empty string, a non-numeric word and a few numbers.  Host only: a stand-alone
program against the header, built with the host compiler."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one line per idiom: "<name> <sf_env.h> <the old expression, written out>"
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sf_env.h"
#define X "SF_TEST_KNOB"
int main()
{
  using namespace sf;
  printf("flag_on %d %d\n", (int)env_flag(X, true), (int)!(getenv(X) && !atoi(getenv(X))));
  printf("flag_off %d %d\n", (int)env_flag(X, false), (int)(getenv(X) && atoi(getenv(X))));
  printf("flag_off_ne0 %d %d\n", (int)env_flag(X, false), (int)(getenv(X) && atoi(getenv(X)) != 0));
  printf("flag_on_eq0 %d %d\n", (int)env_flag(X, true), (int)!(getenv(X) && atoi(getenv(X)) == 0));
  { const char* e = getenv(X); printf("flag_on_tern %d %d\n", (int)env_flag(X, true), (int)(e ? atoi(e) != 0 : true)); }
  for (int d = 0; d < 2; d++) {   // an override of a bool member that holds d
    bool old = d != 0;
    if (const char* e = getenv(X)) old = atoi(e) != 0;
    printf("flag_member%d %d %d\n", d, (int)env_flag(X, d != 0), (int)old);
  }
  printf("int %d %d\n", env_int(X, 8), getenv(X) ? atoi(getenv(X)) : 8);
  printf("int_neg %d %d\n", env_int(X, -1), getenv(X) ? atoi(getenv(X)) : -1);
  {
    int old = 5;   // an override of an int member that holds 5
    if (const char* e = getenv(X)) old = atoi(e);
    printf("int_member %d %d\n", env_int(X, 5), old);
  }
  printf("double %.17g %.17g\n", env_double(X, 20.0), getenv(X) ? atof(getenv(X)) : 20.0);
  printf("set %d %d\n", (int)env_set(X), (int)(getenv(X) != nullptr));
  printf("not_set %d %d\n", (int)!env_set(X), (int)!getenv(X));
  {
    const char *a = env_str(X), *b = getenv(X);
    printf("str [%s]%d [%s]%d\n", a ? a : "", a != nullptr, b ? b : "", b != nullptr);
  }
  {
    int out = 2, old = 2;
    bool given = env_override(X, out), old_given = false;
    if (const char* e = getenv(X)) {
      old = atoi(e);
      old_given = true;
    }
    printf("override %d/%d %d/%d\n", out, (int)given, old, (int)old_given);
  }
  return 0;
}
"""

VALUES = [None, "0", "1", "", "abc", "7", "-3", "2.5", "4x"]

# what the idioms give, from the definition of atoi / atof (not from running either spelling)
EXPECTED = {
    None: {"flag_on": "1", "flag_off": "0", "int": "8", "double": "20", "set": "0", "str": "[]0", "override": "2/0"},
    "0": {"flag_on": "0", "flag_off": "0", "int": "0", "double": "0", "set": "1", "str": "[0]1", "override": "0/1"},
    "1": {"flag_on": "1", "flag_off": "1", "int": "1", "double": "1", "set": "1", "str": "[1]1", "override": "1/1"},
    "": {"flag_on": "0", "flag_off": "0", "int": "0", "double": "0", "set": "1", "str": "[]1", "override": "0/1"},
    "abc": {"flag_on": "0", "flag_off": "0", "int": "0", "double": "0", "set": "1", "str": "[abc]1", "override": "0/1"},
    "2.5": {"flag_on": "1", "flag_off": "1", "int": "2", "double": "2.5", "set": "1", "str": "[2.5]1", "override": "2/1"},
}


@pytest.fixture(scope="module")
def knob_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build the sf_env.h program with")
    d = tmp_path_factory.mktemp("env_knobs")
    src = d / "knobs.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "knobs")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sedifoam_amd", "csrc"), str(src),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("value", VALUES, ids=["unset" if v is None else repr(v) for v in VALUES])
def test_every_idiom_reads_what_its_old_spelling_read(knob_program, value):
    env = {k: v for k, v in os.environ.items() if k != "SF_TEST_KNOB"}
    if value is not None:
        env["SF_TEST_KNOB"] = value
    r = subprocess.run([knob_program], capture_output=True, text=True, env=env, timeout=30)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, new, old = line.split(" ")
        assert new == old, "%s: sf_env.h gives %s, the old spelling %s" % (name, new, old)
        got[name] = new
    assert len(got) == 15
    for name, want in EXPECTED.get(value, {}).items():
        assert got[name] == want, name


def test_the_engine_sources_read_the_environment_through_the_header_only():
    csrc = os.path.join(ROOT, "sedifoam_amd", "csrc")
    hits = [f for f in sorted(os.listdir(csrc))
            if f.endswith((".h", ".hip")) and "getenv" in open(os.path.join(csrc, f)).read()]
    assert hits == ["sf_env.h"]
