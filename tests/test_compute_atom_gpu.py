"""`compute ID group stress/atom | contact/atom | ke/atom | erotate/sphere/atom`, the `c_ID` / `c_ID[k]` columns of `dump
custom` and Lammps.compute_atom() (csrc/sf_compute_atom.hip): per-atom values evaluated on the GPU from the state at the
moment of the output.  stress/atom summed over the bed is thermo's pressure tensor, agrees atom by atom with the NumPy
statement (tests/atom_compute_model.py, itself held to the CPU oracle by tests/test_atom_compute_model.py) and with the half
shares of the contacts() rows after motion, under fix freeze, on a group and in the other list form; the one-column
computes are exact; the text is that of what compute_atom() returns; and the run is left as it was.

Gates: per atom 1e-12 (one force evaluation, tests/contact_model.GATE) against the largest magnitude of the same column over
the bed; a tensor summed over the bed 1e-10 against its largest component (tests/test_thermo_gpu.py).  The bed is the 108-grain
3 x 3 x 3 fcc bed of tests/test_contacts_gpu.py with its STYLES."""
import re

import numpy as np
import pytest

from sedifoam_amd import SfError
from tests import atom_compute_model as am
from tests import contact_model as cm
from tests import dem_cases as dc
from tests.test_contacts_gpu import STYLES, _small
from tests.test_dump_gpu import frames

pytestmark = pytest.mark.gpu

S6 = " ".join("c_s[%d]" % k for k in range(1, 7))
# Steps after which the list has been rebuilt at least once.  Chosen on the CPU oracle (OracleDem.nbuilds on this bed with
# the wall and gravity, one run): gran/hertzFix/history rebuilds first between steps 175 and 200, the Hookean styles have
# rebuilt three times by step 40 -- 250 and 60 leave a margin of 50 and of 20 steps (and two further rebuilds).  At these
# steps the oracle's state has 39 % / 32 % / 30 % of the contacts at the Coulomb cap and over a hundred pairs across a
# periodic face.
STEPS = {"hertz": 250, "hooke": 60, "hooke_plain": 60}


def _inputs(bed):
    r = 0.5 * np.asarray(bed["diameter"])
    return np.arange(1, len(r) + 1, dtype=np.int32), r, 4.0 * np.pi / 3.0 * r ** 3 * np.asarray(bed["density"])


def _model(bed, cfg, lmp, frozen=None):
    st = lmp.get_state()
    tag, r, m = _inputs(bed)
    assert (st["tag"] == tag).all()
    pp = cm.pair_params(cfg["pair"], cfg["kn"], None, cfg["gamman"], None, cfg["xmu"])
    return am.per_atom(bed["boxlo"], bed["boxhi"], bed["periodic"], tag, st["x"], r, m, st["v"], st["omega"], lmp.history(),
                       pp, frozen=frozen), st


def _assert_columns(got, want, what, gate=am.GATE):
    errs = am.column_errors(got, want)
    print("%s: rel per column %s" % (what, ["%.2e" % e for e in errs]))
    assert np.asarray(got).shape == np.asarray(want).shape
    assert (errs <= gate).all(), (what, errs)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the commands and the query exist

def test_computes_columns_and_query_are_known(tmp_path):
    bed, cfg = _small()
    n = len(bed["x"])
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute s all stress/atom")
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    lmp.command("compute e all erotate/sphere/atom")
    lmp.command("dump d all custom 10 %s id x %s c_c c_k c_e" % (tmp_path / "d.dump", S6))
    lmp.command("run 0")
    assert lmp.compute_atom_launches() == 4
    s, c, k, e = (lmp.compute_atom(i) for i in "scke")
    assert s.shape == (n, 6) and c.shape == k.shape == e.shape == (n,)
    assert lmp.compute_atom_launches() == 4   # (the frame of step 0 evaluated them; the queries reuse it)
    assert np.abs(s).max() > 0 and c.min() >= 3 and (c == np.round(c)).all() and k.min() > 0 and e.min() > 0
    fr = frames(str(tmp_path / "d.dump"))
    assert [f[0] for f in fr] == [0] and fr[0][1] == n
    assert fr[0][2][4] == ("ITEM: ATOMS id x %s c_c c_k c_e" % S6).encode()
    lmp.command("undump d")
    for i in "scke":
        lmp.command("uncompute " + i)
    with pytest.raises(SfError, match="Could not find compute ID to delete"):
        lmp.command("uncompute s")
    with pytest.raises(SfError, match="Could not find compute ID s"):
        lmp.compute_atom("s")
    lmp.close()
    # defined but never written or asked for: nothing is launched
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute s all stress/atom")
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    lmp.command("dump d all custom 10 %s id x" % (tmp_path / "plain.dump"))
    lmp.command("run 30")
    assert lmp.compute_atom_launches() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sum over the bed is thermo's pressure tensor

@pytest.mark.parametrize("style", sorted(STYLES))
def test_stress_summed_over_the_bed_is_thermos_pressure(style, tmp_path):
    """pair forces only, run 0: the virial of the line is the setup evaluation's (shearupdate = 0, the velocities the
    compute sees)"""
    bed, cfg = _small(style, wall=False)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("log %s" % (tmp_path / "log.lammps"))
    lmp.command("thermo_style custom step press pxx pyy pzz pxy pxz pyz")
    lmp.command("compute s all stress/atom")
    lmp.command("compute sn all stress/atom NULL")
    lmp.command("compute sp all stress/atom pair")
    lmp.command("compute sv all stress/atom NULL virial fix bond angle dihedral improper kspace")
    lmp.command("compute sk all stress/atom ke")
    lmp.command("run 0")
    vol = float(np.prod(np.asarray(bed["boxhi"], dtype=np.float64) - np.asarray(bed["boxlo"], dtype=np.float64)))
    p = np.array([lmp.get_thermo(k) for k in ("pxx", "pyy", "pzz", "pxy", "pxz", "pyz")])
    s, sp, sk = lmp.compute_atom("s"), lmp.compute_atom("sp"), lmp.compute_atom("sk")
    assert lmp.compute_atom("sn").tobytes() == s.tobytes() and lmp.compute_atom("sv").tobytes() == sp.tobytes()
    st = lmp.get_state()
    m = _inputs(bed)[2]
    K = np.array([np.sum(m * st["v"][:, a] * st["v"][:, b]) for a, b in am.PAIRS6])
    scale = float(np.max(np.abs(p)))
    e_all = float(np.max(np.abs(-s.sum(axis=0) / vol - p))) / scale
    e_pair = float(np.max(np.abs(-sp.sum(axis=0) / vol - (p - K / vol)))) / scale
    e_ke = float(np.max(np.abs(-sk.sum(axis=0) - K))) / float(np.max(np.abs(K)))
    print("sum rule (%s): ke + pair %.3e, pair %.3e, ke %.3e; |K| / |pV| = %.2e" % (
        style, e_all, e_pair, e_ke, float(np.max(np.abs(K))) / (scale * vol)))
    assert e_all <= am.SUM_GATE and e_pair <= am.SUM_GATE and e_ke <= am.SUM_GATE
    assert lmp.get_thermo("press") == pytest.approx(-(s[:, 0] + s[:, 1] + s[:, 2]).sum() / (3.0 * vol), rel=am.SUM_GATE)


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the model after motion (and 9. the same in the other list form)

def _after_motion(style):
    bed, cfg = _small(style)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute s all stress/atom")
    lmp.command("compute sp all stress/atom pair")
    lmp.command("compute c all contact/atom")
    lmp.command("run 0")
    builds0 = lmp.info().nbuilds
    lmp.command("run %d" % STEPS[style])
    assert lmp.info().nbuilds > builds0, "the list was never rebuilt: the mirrored history reads are not exercised"
    mod, st = _model(bed, cfg, lmp)
    s, sp = lmp.compute_atom("s"), lmp.compute_atom("sp")
    _assert_columns(s, am.stress(mod), "stress/atom after %d steps (%s)" % (STEPS[style], style))
    _assert_columns(sp, am.stress(mod, ke=False), "stress/atom pair after %d steps (%s)" % (STEPS[style], style))
    assert (lmp.compute_atom("c") == mod["contacts"]).all()
    # the identity that needs no model of the law: the half shares of the contacts() rows, summed per atom (del of a row
    # from the positions: the model's pair search)
    rows = lmp.contacts()
    delta = {(int(st["tag"][i]), int(st["tag"][j])): d for i, j, d in zip(mod["I"], mod["J"], mod["D"])}
    assert len(delta) == len(mod["I"]) == 2 * len(rows["tag1"])   # (no partner touches through two images)
    pos = {int(t): k for k, t in enumerate(st["tag"])}
    W = np.zeros((len(st["tag"]), 6))
    for a, b, F in zip(rows["tag1"].tolist(), rows["tag2"].tolist(), rows["f"] + rows["fs"]):
        d = delta[(a, b)]
        half = [0.5 * d[p] * F[q] for p, q in am.PAIRS6]
        W[pos[a]] += half   # (del and F both change sign on the other side)
        W[pos[b]] += half
    _assert_columns(sp, -W, "stress/atom pair against the rows of contacts() (%s)" % style)
    # what the input must exercise: sliding and sticking contacts, pairs across a periodic face, history
    fscale = float(np.max(np.abs(rows["force"])))
    capped = np.abs(rows["fsmag"] - cfg["xmu"] * np.abs(rows["force"])) <= cm.GATE * fscale
    assert 0.1 <= capped.mean() <= 0.9, capped.mean()
    assert mod["wrapped"].any() and not mod["wrapped"].all()
    if style != "hooke_plain":
        assert max(float(np.max(np.abs(h))) for h in lmp.history().values()) > 0.0


@pytest.mark.parametrize("style", sorted(STYLES))
def test_stress_after_motion_is_the_models(style):
    """the default list form on one domain: root + image code words, no ghost atoms"""
    _after_motion(style)


def test_stress_after_motion_with_ghost_atoms(monkeypatch):
    """SF_GHOST_FREE is read in the engine's constructor (docs/knobs.md): 0 makes the periodic images ghost atoms and the
    list words plain indices.  (info().nghost cannot tell the two forms apart: without ghost atoms it counts the images
    LAMMPS would have made)"""
    monkeypatch.setenv("SF_GHOST_FREE", "0")
    _after_motion("hooke")


# ---------------------------------------------------------------------------------------------------------------------
# 4. fix freeze

def test_partners_of_frozen_atoms_take_the_meff_override():
    """a frozen bottom layer, pair forces only, run 0: the model with meff = the free partner's mass
    (pair_gran_hertzFix_history.cpp:188-189); without the override the frozen atoms' neighbourhood differs"""
    bottom = lambda bed: (1 + (bed["x"][:, 1] < 0.8e-3)).astype(np.int32)
    bed, cfg = _small("hertz", wall=False, types=bottom, frozen_types=[2])
    frozen = bed["type"] == 2
    assert 10 <= frozen.sum() <= len(frozen) // 2
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute sp all stress/atom pair")
    lmp.command("run 0")
    mod, _ = _model(bed, cfg, lmp, frozen=frozen)
    sp = lmp.compute_atom("sp")
    _assert_columns(sp, am.stress(mod, ke=False), "fix freeze")
    plain, _ = _model(bed, cfg, lmp)
    touched = np.zeros(len(frozen), bool)
    touched[mod["I"][frozen[mod["I"]] | frozen[mod["J"]]]] = True
    assert touched.any() and not touched.all()
    diff = np.abs(am.stress(plain, ke=False) - sp).max(axis=1)
    assert diff[touched].max() > 1e-6 * np.abs(sp).max() and diff[~touched].max() <= am.GATE * np.abs(sp).max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a group selects the atoms that get a value; partners count whatever their group

def test_a_group_gets_the_bits_of_all_and_the_others_zero():
    every_third = lambda bed: (1 + (np.arange(len(bed["x"])) % 3 == 0)).astype(np.int32)
    bed, cfg = _small(types=every_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    for name, style in (("s", "stress/atom"), ("c", "contact/atom"), ("k", "ke/atom"), ("e", "erotate/sphere/atom")):
        lmp.command("compute %s all %s" % (name, style))
        lmp.command("compute %s2 two %s" % (name, style))
    lmp.command("run 25")
    inside = bed["type"] == 2
    assert 0 < inside.sum() < len(inside)
    for name in "scke":
        every, two = lmp.compute_atom(name), lmp.compute_atom(name + "2")
        assert not two[~inside].any(), name
        assert two[inside].tobytes() == every[inside].tobytes(), name
        assert every[~inside].any(), name   # (so the zeros are the group's doing)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the one-column computes

def test_counts_and_kinetic_energies():
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    lmp.command("compute e all erotate/sphere/atom")
    lmp.command("run 30")
    rows, st = lmp.contacts(), lmp.get_state()
    tag, r, m = _inputs(bed)
    want = np.bincount(np.concatenate([rows["tag1"], rows["tag2"]]) - 1, minlength=len(tag))
    c = lmp.compute_atom("c")
    assert c.dtype == np.float64 and (c == want).all() and want.sum() > 8 * len(tag)
    ke = 0.5 * m * np.sum(st["v"] * st["v"], axis=1)
    er = 0.5 * (0.4 * m * r * r) * np.sum(st["omega"] * st["omega"], axis=1)
    e_k = float(np.max(np.abs(lmp.compute_atom("k") - ke) / ke))
    e_e = float(np.max(np.abs(lmp.compute_atom("e") - er) / er))
    print("ke/atom rel %.2e, erotate/sphere/atom rel %.2e" % (e_k, e_e))
    assert e_k <= 1e-14 and e_e <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# 7. text

def test_dump_custom_columns_are_the_text_of_compute_atom(tmp_path):
    bed, cfg = _small()
    n = len(bed["x"])
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute s all stress/atom")
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    cols = "id %s c_c c_k" % S6
    lmp.command("dump a all custom 15 %s %s" % (tmp_path / "a.dump", cols))
    lmp.command("dump b all custom 15 %s %s" % (tmp_path / "b.dump", cols))
    lmp.command("dump_modify b sort id")
    lmp.command("run 0")
    seen = []
    for piece in range(3):
        if piece:
            lmp.step(15)
        seen.append((lmp.compute_atom("s"), lmp.compute_atom("c"), lmp.compute_atom("k")))
    lmp.sync()
    fa, fb = frames(str(tmp_path / "a.dump")), frames(str(tmp_path / "b.dump"))
    assert [f[0] for f in fa] == [f[0] for f in fb] == [0, 15, 30]
    for a, b, (s, c, k) in zip(fa, fb, seen):
        want = [("%d " % (i + 1) + "".join("%g " % v for v in s[i]) + "%g %g \n" % (c[i], k[i])).encode() for i in range(n)]
        assert a[2][4] == b[2][4] == ("ITEM: ATOMS " + cols).encode()
        assert b[3] == want                   # sorted by id: the order of compute_atom()
        assert sorted(a[3]) == sorted(want)   # the engine's order: the same lines
    assert not (seen[0][0] == seen[2][0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. passive and repeatable

def test_a_run_with_compute_output_ends_in_the_bits_of_the_run_without(tmp_path):
    """60 + 35 + 60 + 50 steps with `dump custom` every 37; the same with c_ columns in a second dump every 37 and
    queries between the pieces.  Both runs are cut at the same steps, so they end with the same rebuilds and bits"""
    bed, cfg = _small("hooke")   # (the style that rebuilds often on this bed: STEPS above)
    outs = []
    for with_computes in (False, True):
        lmp = dc.make_hip(bed, cfg)
        lmp.command("dump d all custom 37 %s id x y z fx fy fz" % (tmp_path / ("bed%d.dump" % with_computes)))
        if with_computes:
            lmp.command("compute s all stress/atom")
            lmp.command("compute c all contact/atom")
            lmp.command("compute k all ke/atom")
            lmp.command("dump x all custom 37 %s id %s c_c c_k" % (tmp_path / "bed.stress", S6))
        lmp.setup()
        for piece in (60, 35, 60, 50):
            lmp.step(piece)
            if with_computes:
                assert np.abs(lmp.compute_atom("s")).max() > 0 and lmp.compute_atom("c").max() > 0
        lmp.sync()
        outs.append((lmp.get_state(), lmp.history(), lmp.info().nbuilds, lmp.compute_atom_launches()))
    assert outs[0][2] == outs[1][2] >= 2
    for k in ("tag", "x", "v", "omega", "f", "torque"):
        assert outs[0][0][k].tobytes() == outs[1][0][k].tobytes(), k
    assert set(outs[0][1]) == set(outs[1][1])
    assert all(outs[0][1][p].tobytes() == outs[1][1][p].tobytes() for p in outs[0][1])
    assert (tmp_path / "bed0.dump").read_bytes() == (tmp_path / "bed1.dump").read_bytes()
    assert [f[0] for f in frames(str(tmp_path / "bed.stress"))] == [0, 37, 74, 111, 148, 185]
    # six frames of three computes, and the queries after the pieces ending at 60, 95, 155, 205 (none of them a frame's step)
    assert outs[0][3] == 0 and outs[1][3] == 6 * 3 + 4 * 2


def test_one_evaluation_per_step_and_the_same_bits_twice(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute s all stress/atom")
    lmp.command("dump a all custom 20 %s id c_s[1] c_s[4]" % (tmp_path / "a.dump"))
    lmp.command("dump b all custom 10 %s id c_s[2]" % (tmp_path / "b.dump"))
    lmp.command("run 20")
    # frames: a at 0 and 20, b at 0, 10 and 20 -- three steps, three evaluations
    assert lmp.compute_atom_launches() == 3
    s = lmp.compute_atom("s")
    assert lmp.compute_atom_launches() == 3
    lmp.command("compute t all stress/atom ke pair")   # a second evaluation of the same state
    assert lmp.compute_atom("t").tobytes() == s.tobytes()
    assert lmp.compute_atom_launches() == 4
    lmp.command("uncompute t")
    lmp.command("compute t all stress/atom")
    assert lmp.compute_atom("t").tobytes() == s.tobytes()
    # a command that changes the state at an unchanged step is seen
    lmp.command("compute k all ke/atom")
    k0 = lmp.compute_atom("k")
    lmp.command("velocity all set 0.0 0.0 0.25")
    _, _, m = _inputs(bed)
    assert np.abs(lmp.compute_atom("k") / (0.5 * m * 0.0625) - 1.0).max() <= 1e-14 and k0.max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals

def _with_lubrication():
    bed, cfg = _small(lub=(1.0e-3, 1, 0, 1.001e-3, 1.2e-3, 1, 1))
    return dc.make_hip(bed, cfg)


def _without_pair_style():
    from sedifoam_amd import Lammps
    bed, _ = _small()
    lmp = Lammps()
    lmp.set_box(bed["boxlo"], bed["boxhi"])
    lmp.create_atoms(bed["x"], bed["diameter"], bed["density"])
    return lmp


def _plain():
    return dc.make_hip(*_small())


def _decompose(lmp):
    """what a decomposed run sets on the engine (two slabs along x); nothing is run afterwards"""
    bed, _ = _small()
    half = 0.5 * (float(bed["boxlo"][0]) + float(bed["boxhi"][0]))
    assert lmp.L.sf_dem_set_subdomain(lmp.ptr, 0, 2, float(bed["boxlo"][0]), half) == 0


@pytest.mark.parametrize("make,before,line,msg", [
    (_without_pair_style, [], "compute s all stress/atom", "compute stress/atom: no granular pair style is defined"),
    (_without_pair_style, [], "compute c all contact/atom", "compute contact/atom: no pair style is defined"),
    (_with_lubrication, [], "compute s all stress/atom", "compute stress/atom: not with lubricate/poly"),
    (_plain, ["fix r all rigid/nve single"], "compute s all stress/atom", "not while fix rigid/nve exists"),
    (_plain, [_decompose], "compute s all stress/atom", "compute stress/atom: one rank only"),
    (_plain, [_decompose], "compute c all contact/atom", "compute contact/atom: one rank only"),
    (_plain, [_decompose], "compute k all ke/atom", "compute ke/atom: one rank only"),
    (_plain, ["compute k all ke/atom", _decompose], "dump d all custom 10 {p} id c_k", "c_ columns on one rank only"),
    (_plain, [], "compute s all stress/atom mytemp ke", "a temperature compute (mytemp) is not supported"),
    (_plain, [], "compute s all stress/atom ke what", "Illegal compute stress/atom command"),
    (_plain, [], "compute k all ke/atom extra", "Illegal compute ke/atom command"),
    (_plain, ["compute s all stress/atom"], "compute s all ke/atom", "Reuse of compute ID"),
    (_plain, ["compute s all pair/local dist"], "compute s all ke/atom", "Reuse of compute ID"),
    (_plain, ["compute s all ke/atom"], "compute s all pair/local dist", "Reuse of compute ID"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_9", "Could not find dump custom compute ID 9"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s",
     "Dump custom compute does not compute per-atom vector: c_s"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s[7]",
     "Dump custom compute vector is accessed out-of-range: c_s[7]"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s[0]", "Invalid attribute c_s[0] in dump custom"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s[2", "Invalid attribute c_s[2 in dump custom"),
    (_plain, ["compute c all contact/atom"], "dump d all custom 10 {p} id c_c[1]",
     "Dump custom compute does not compute per-atom array: c_c[1]"),
    (_plain, ["compute p all pair/local dist"], "dump d all custom 10 {p} id c_p",
     "Dump custom compute does not compute per-atom info: p is a compute pair/local"),
    (_plain, ["compute k all ke/atom"], "dump d all local 10 {p} index c_k",
     "Dump local compute does not compute local info: k is a per-atom compute"),
    (_plain, ["compute k all ke/atom", "dump d all custom 10 {p} id c_k"], "uncompute k",
     "a dump custom still uses this compute"),
    # (an index is digits and nothing else, at most 1000000, and nothing follows the `]`: parse_cref of sf_ave_common.h)
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s[+1]", "Invalid attribute c_s[+1] in dump custom"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s]", "Invalid attribute c_s] in dump custom"),
    (_plain, ["compute s all stress/atom"], "dump d all custom 10 {p} id c_s[1000001]",
     "Invalid attribute c_s[1000001] in dump custom"),
])
def test_refused_forms(make, before, line, msg, tmp_path):
    lmp = make()
    for b in before:
        if callable(b):
            b(lmp)
        else:
            lmp.command(b.format(p=tmp_path / "r.dump"))
    with pytest.raises(SfError, match=re.escape(msg)):
        lmp.command(line.format(p=tmp_path / "r.dump"))


def test_evaluations_before_the_first_run_and_under_changed_settings_are_refused():
    lmp = _plain()
    lmp.command("compute s all stress/atom")
    lmp.command("compute c all contact/atom")
    lmp.command("compute k all ke/atom")
    for i in "sc":
        with pytest.raises(SfError, match="no neighbour list yet"):
            lmp.compute_atom(i)
    assert lmp.compute_atom("k").min() > 0   # (needs no list)
    lmp.command("run 0")
    assert np.abs(lmp.compute_atom("s")).max() > 0
    lmp.command("fix r all rigid/nve single")   # the settings are checked again at every evaluation
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.compute_atom("s")
