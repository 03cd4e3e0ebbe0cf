"""The one ID space of the computes (csrc/sf_compute_ids.hip) and what every reader of `c_ID` accepts of each kind
(csrc/sf_compute_ref.h), on the GPU: one compute of each kind -- pair/local, ke/atom, chunk/atom, ke, rdf -- on the 108-grain bed
of tests/test_global_gpu.py (the smallest of its beds that has contacts) after `run 0`.

Reuse of an ID across the kinds; each reader's exact text for every wrong kind, and the right kind accepted; the order of the
refusals of `uncompute`; a state change at an unchanged step reaching the per-atom, the global and the array computes and
the cutoff grid (computes_invalidate), measured with the launch counters; and the files of every output kind complete after the
engine is closed with all of them open (the order in which SfLammps lets its members go, csrc/sf_handles.h)."""
import re

import numpy as np
import pytest

from sedifoam_amd import SfError
from tests import dem_cases as dc
from tests.test_ave_chunk_gpu import Y1
from tests.test_contacts_gpu import _inputs, _small
from tests.test_dump_gpu import frames
from tests.test_global_gpu import _third

pytestmark = pytest.mark.gpu

# one compute of each kind: ID -> (kind, the words behind `compute ID all`)
COMPUTES = {"pl": ("local", "pair/local force"), "ka": ("atom", "ke/atom"), "ch": ("chunk", "chunk/atom " + Y1),
            "K": ("global", "ke"), "g": ("array", "rdf 10 cutoff 1.3e-3")}


def _engine():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 0")
    for cid, (_, words) in COMPUTES.items():
        lmp.command("compute %s all %s" % (cid, words))
    return bed, lmp


def _refused(text):
    return pytest.raises(SfError, match=re.escape(text) + "$")


@pytest.fixture(scope="module")
def five():
    bed, lmp = _engine()
    yield lmp
    lmp.close()


def test_an_id_of_one_kind_is_taken_for_every_other(five):
    for cid, (kind, _) in COMPUTES.items():
        for other, words in COMPUTES.values():
            if other != kind:
                with _refused("Reuse of compute ID"):
                    five.command("compute %s all %s" % (cid, words))
    assert five.compute_global("K").shape == (1,) and five.compute_array("g").shape == (10, 3)   # (all five still stand)
    assert five.compute_atom("ka").shape == five.compute_atom("ch").shape == (108,) and five.contacts()["force"].size > 0


NOT_ATOM = "Dump custom compute does not compute per-atom info: "
NOT_LOCAL = "Dump local compute does not compute local info: "
NOT_GLOBAL = "compute %s does not calculate a global scalar or vector (sf_lammps_compute_atom and sf_lammps_get_contacts return " \
             "per-atom and local values)"
# reader -> (the line, with {id} and {p}; how to take back what an accepted line made; per kind the text, None: accepted)
READERS = {
    "dump custom": ("dump x all custom 10 {p} id c_{id}", "undump x", {
        "local": NOT_ATOM + "{id} is a compute pair/local (dump local prints its rows)", "atom": None, "chunk": None,
        "global": NOT_ATOM + "{id} is a global compute (fix ave/time and thermo print it)",
        "array": NOT_ATOM + "{id} is a global array (fix ave/time mode vector prints it)"}),
    "dump local": ("dump x all local 10 {p} index c_{id}", "undump x", {
        "local": None, "atom": NOT_LOCAL + "{id} is a per-atom compute (dump custom prints it)",
        "chunk": NOT_LOCAL + "{id} is a per-atom compute (dump custom prints it)",
        "global": NOT_LOCAL + "{id} is a global compute (fix ave/time and thermo print it)",
        "array": NOT_LOCAL + "{id} is a global array (fix ave/time mode vector prints it)"}),
    "compute reduce": ("compute x all reduce sum c_{id}", "uncompute x", {
        "local": None, "atom": None, "chunk": None,
        "global": "Compute reduce compute calculates global values (c_{id} is a global compute: per-atom and local ones are reduced)",
        "array": "Compute reduce compute calculates global values (c_{id} is a global array: per-atom and local ones are reduced)"}),
    "fix ave/chunk value": ("fix x all ave/chunk 2 3 10 ch c_{id}", "unfix x", {
        "local": "Fix ave/chunk compute does not calculate per-atom values", "atom": None, "chunk": None,
        "global": "Fix ave/chunk compute does not calculate per-atom values",
        "array": "Fix ave/chunk compute does not calculate per-atom values"}),
    "fix ave/chunk chunk ID": ("fix x all ave/chunk 2 3 10 {id} vx", "unfix x", {
        "local": "Fix ave/chunk does not use chunk/atom compute", "atom": "Fix ave/chunk does not use chunk/atom compute",
        "chunk": None, "global": "Fix ave/chunk does not use chunk/atom compute",
        "array": "Fix ave/chunk does not use chunk/atom compute"}),
    "fix ave/time scalar": ("fix x all ave/time 2 3 10 c_{id}", "unfix x", {
        "local": "Fix ave/time compute does not calculate a scalar", "atom": "Fix ave/time compute does not calculate a scalar",
        "chunk": "Fix ave/time compute does not calculate a scalar", "global": None,
        "array": "Fix ave/time compute does not calculate a scalar"}),
    "fix ave/time vector": ("fix x all ave/time 2 3 10 c_{id}[2] mode vector", "unfix x", {
        "local": "Fix ave/time compute does not calculate an array", "atom": "Fix ave/time compute does not calculate an array",
        "chunk": "Fix ave/time compute does not calculate an array", "global": "Fix ave/time compute does not calculate an array",
        "array": None}),
    # (per-atom and local values are binned in mode vector only, a global scalar in mode scalar only: each kind in its mode)
    "fix ave/histo": ("fix x all ave/histo 1 1 1 0 1 10 c_{id} mode {mode}", "unfix x", {
        "local": None, "atom": None, "chunk": None, "global": None,
        "array": "Fix ave/histo compute does not calculate a global scalar or vector (c_{id} is a global array, which is not binned)"}),
    "thermo": ("thermo_style custom step c_{id}", "thermo_style one", {
        "local": "Thermo compute does not compute scalar", "atom": "Thermo compute does not compute scalar",
        "chunk": "Thermo compute does not compute scalar", "global": None, "array": "Thermo compute does not compute scalar"}),
}


@pytest.mark.parametrize("reader", sorted(READERS))
def test_a_script_reader_names_each_wrong_kind_and_takes_the_right_one(five, tmp_path, reader):
    line, undo, texts = READERS[reader]
    for cid, (kind, _) in COMPUTES.items():
        words = line.format(id=cid, p=tmp_path / "out.txt", mode="scalar" if kind == "global" else "vector")
        if texts[kind] is None:
            five.command(words)
            five.command(undo)
        else:
            with _refused(texts[kind].format(id=cid)):
                five.command(words)


def test_a_getter_names_each_wrong_kind_and_takes_the_right_one(five):
    getters = {
        "compute_atom": {"local": "Could not find compute ID {id}", "atom": None, "chunk": None,
                         "global": "compute {id} does not calculate per-atom values (it is a global compute)",
                         "array": "compute {id} does not calculate per-atom values (it is a global array: sf_lammps_compute_array "
                                  "returns it)"},
        "compute_global": {"local": NOT_GLOBAL % "{id}", "atom": NOT_GLOBAL % "{id}", "chunk": NOT_GLOBAL % "{id}", "global": None,
                           "array": "compute {id} does not calculate a global scalar or vector (it is a global array: "
                                    "sf_lammps_compute_array returns it)"},
        "compute_array": dict({k: "compute {id} does not calculate a global array (compute rdf does)"
                               for k in ("local", "atom", "chunk", "global")}, array=None),
        "compute_atom_cost": {"local": "Could not find compute ID {id}", "atom": None,
                              "chunk": "compute {id} is a chunk/atom compute: sf_lammps_ave_chunk_cost times its pass",
                              "global": "Could not find compute ID {id}", "array": "Could not find compute ID {id}"},
    }
    for name, texts in getters.items():
        for cid, (kind, _) in COMPUTES.items():
            if texts[kind] is None:
                getattr(five, name)(cid)
            else:
                with _refused(texts[kind].format(id=cid)):
                    getattr(five, name)(cid)
    with _refused("Could not find compute ID nope"):
        five.compute_array("nope")


def test_uncompute_refuses_in_its_order_down_to_success(tmp_path):
    """ka is named by a compute reduce and by a dump custom; the reduce by a fix ave/time and by thermo_style custom: of two
    reasons the earlier one in the order reduce, averaging fix, thermo / dump is the one given"""
    bed, lmp = _engine()
    lmp.command("compute r all reduce sum c_ka")
    lmp.command("fix t all ave/time 2 3 10 c_r")
    lmp.command("thermo_style custom step c_r")
    lmp.command("dump d all custom 10 %s id c_ka" % (tmp_path / "d.txt"))
    with _refused("uncompute ka: a compute reduce still uses this compute (uncompute it first)"):
        lmp.command("uncompute ka")
    with _refused("uncompute r: a fix ave/time still uses this compute (unfix it first)"):
        lmp.command("uncompute r")
    lmp.command("unfix t")
    with _refused("uncompute r: thermo_style custom still names this compute (give another thermo_style first)"):
        lmp.command("uncompute r")
    lmp.command("thermo_style one")
    lmp.command("uncompute r")
    with _refused("uncompute ka: a dump custom still uses this compute (undump it first)"):
        lmp.command("uncompute ka")
    lmp.command("undump d")
    lmp.command("uncompute ka")
    with _refused("Could not find compute ID to delete"):
        lmp.command("uncompute ka")
    # the other kinds: a dump local holds its pair/local; nothing holds the chunk/atom, the global and the array compute
    lmp.command("dump l all local 10 %s index c_pl" % (tmp_path / "l.txt"))
    with _refused("uncompute pl: a dump local still uses this compute (undump it first)"):
        lmp.command("uncompute pl")
    lmp.command("undump l")
    for cid in ("pl", "ch", "K", "g"):
        lmp.command("uncompute " + cid)
        with _refused("Could not find compute ID to delete"):
            lmp.command("uncompute " + cid)
    lmp.close()


def _counters(lmp):
    nbr = lmp.nbr_launches()
    return np.array([lmp.compute_atom_launches(), lmp.global_launches()["launches"], nbr["grid_builds"], nbr["launches"]])


def test_a_state_change_at_an_unchanged_step_reaches_every_owner():
    bed, lmp = _engine()
    _, _, mass = _inputs(bed)

    def ask():
        before = _counters(lmp)
        out = lmp.compute_atom("ka"), lmp.compute_global("K"), lmp.compute_array("g")
        return out, _counters(lmp) - before

    (ka0, K0, g0), first = ask()
    assert (first > 0).all(), first   # launches of the per-atom compute, of the global compute, a grid build, the rdf walk
    _, again = ask()
    assert (again == 0).all(), again   # nothing changed: every value is the one made at this step
    step = lmp.info().nsteps
    lmp.command("velocity all set 0.1 -0.2 0.3")
    assert lmp.info().nsteps == step
    (ka1, K1, g1), fresh = ask()
    print("launches: first %s again %s after velocity %s" % (first, again, fresh))
    assert (fresh == first).all(), (first, fresh)
    # 0.5 m |v|^2: a handful of roundings each (2^-53 relative); the sum of 108 such terms of one sign within 108 2^-53
    want = 0.5 * mass * (0.1 ** 2 + 0.2 ** 2 + 0.3 ** 2)
    assert np.abs(ka1 - want).max() <= 1e-14 * want.max() and np.abs(ka0 - want).max() > 1e-3 * want.max()
    assert abs(K1[0] - ka1.sum()) <= 1e-13 * ka1.sum() and abs(K0[0] - ka0.sum()) <= 1e-13 * ka0.sum()
    assert (g1 == g0).all()   # (the positions did not change)
    lmp.close()


def test_every_output_file_is_complete_after_close(tmp_path):
    """a dump custom and a dump local, a thermo log, one fix of each averaging kind (ave/time in both modes), a region with a
    dynamic group and a compute of each kind, all open when the engine is closed after `run 20`"""
    bed, lmp = _engine()
    p = {k: str(tmp_path / (k + ".txt")) for k in ("custom", "local", "log", "chunk", "time", "vector", "histo")}
    ymid = 0.5 * (float(bed["boxlo"][1]) + float(bed["boxhi"][1]))
    for line in ("region up block INF INF %.17g INF INF INF side in units box" % ymid,
                 "group up dynamic all region up every 5",
                 "compute Kup up ke",
                 "log " + p["log"],
                 "thermo_style custom step ke c_K c_Kup",
                 "thermo 10",
                 "dump dc all custom 10 %s id c_ka c_ch" % p["custom"],
                 "dump dl all local 10 %s index c_pl" % p["local"],
                 "fix fc all ave/chunk 2 3 10 ch vx c_ka file " + p["chunk"],
                 "fix ft all ave/time 2 3 10 c_K c_Kup file " + p["time"],
                 "fix fv all ave/time 2 3 10 c_g[2] mode vector file " + p["vector"],
                 "fix fh all ave/histo 2 3 10 0 1e-6 8 c_ka mode vector file " + p["histo"],
                 "run 20"):
        lmp.command(line)
    nchunk, nrows = lmp.ave_chunk("fc")["count"].size, lmp.ave_time("fv")["values"].shape[0]
    nlocal = lmp.contacts()["force"].size
    lmp.close()
    fr = frames(p["custom"])
    assert [f[0] for f in fr] == [0, 10, 20] and fr[-1][1] == 108
    local = open(p["local"]).read()
    assert local.endswith(" \n") and local.count("ITEM: TIMESTEP\n") == 3
    last = local.split("ITEM: TIMESTEP\n")[-1].splitlines()
    assert last[0] == "20" and int(last[2]) == len(last) - 8 and int(last[2]) == nlocal > 0
    log = open(p["log"]).read().splitlines()
    rows = [ln for ln in log if ln.split() and ln.split()[0] in ("0", "10", "20") and len(ln.split()) == 4]
    assert [int(r.split()[0]) for r in rows] == [0, 10, 20], rows
    assert any(ln.startswith("Loop time of ") for ln in log[-3:]), log[-3:]   # (what a run writes last)

    def blocks(path, ntitles, per_block):
        lines = open(path).read().splitlines()[ntitles:]
        assert open(path).read().endswith("\n") and len(lines) == 2 * (1 + per_block), (path, len(lines))
        return [int(ln.split()[0]) for ln in lines[::1 + per_block]]

    assert blocks(p["chunk"], 3, nchunk) == [10, 20]
    assert blocks(p["time"], 2, 0) == [10, 20]
    assert blocks(p["vector"], 3, nrows) == [10, 20] and nrows == 10
    assert blocks(p["histo"], 3, 8) == [10, 20]
