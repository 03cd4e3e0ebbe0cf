"""`compute ID group pair/local ...` (gran/local), `dump ID group local N file index c_ID[k] ...` and Lammps.contacts()
(csrc/sf_contacts.hip): the contact network evaluated on the GPU from the state at the moment of the output.  The rows sum
to the engine's own pair forces, agree with the NumPy statement of a row (tests/contact_model.py, itself held to the CPU
oracle by tests/test_contact_model.py) after motion, under fix freeze and on a group, are written as the text of what
contacts() returns, and leave the run as it was.

Every numeric comparison uses the project's gate for one force evaluation, 1e-12 (tests/test_dem_gpu.py): per column
against that column's largest magnitude, p1 .. p4 against the largest magnitude of `force` (the tangential force is the
pair force minus its normal part)."""
import os
import re

import numpy as np
import pytest

from sedifoam_amd import SfError, synthetic
from tests import contact_model as cm
from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

VALUES = "dist eng force fx fy fz p1 p2 p3 p4 tag1 tag2".split()

# the three pair styles with parameters under which, after 40 steps of the 3 x 3 x 3 bed below, a good share of the contacts
# slides and a good share does not: chosen with the CPU oracle plus the model (seed 3, vmax 0.2: 53 %, 29 %, 26 % of the rows
# Coulomb-capped), and asserted on the rows the test gets
STYLES = {
    "hertz": dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.1),
    "hooke": dict(pair="hooke", kn=5.0e4, gamman=2.0e5, xmu=0.002),
    "hooke_plain": dict(pair="hooke_plain", kn=5.0e4, gamman=2.0e5, xmu=0.002),
}


def _small(style="hertz", wall=True, types=None, **over):
    """the 3 x 3 x 3 fcc bed of tests/test_dump_gpu.py (108 grains, periodic in x and z); wall = False: pair forces only
    (no wall, g = 0)"""
    bed = synthetic.fcc_bed((3, 3, 3), seed=3, vmax=0.2)
    bed["omega"] = np.random.default_rng(7).uniform(-50.0, 50.0, size=(len(bed["x"]), 3))
    if types is not None:
        bed["type"] = types(bed)
    cfg = dict(STYLES[style], g=9.81 if wall else 0.0, dt=1.0e-6, skin=0.25e-3,
               walls=[(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))] if wall else [])
    cfg.update(over)
    return bed, cfg


def _inputs(bed):
    r = 0.5 * np.asarray(bed["diameter"])
    return np.arange(1, len(r) + 1, dtype=np.int32), r, 4.0 * np.pi / 3.0 * r ** 3 * np.asarray(bed["density"])


def _by_tags(rows):
    o = np.lexsort((rows["tag2"], rows["tag1"]))
    return {k: v[o] for k, v in rows.items()}


def _model(bed, cfg, lmp, frozen=None, group=None):
    st = lmp.get_state()
    tag, r, m = _inputs(bed)
    assert (st["tag"] == tag).all()
    return cm.contact_rows(bed["boxlo"], bed["boxhi"], bed["periodic"], tag, st["x"], r, m, st["v"], st["omega"],
                           lmp.history(), cm.pair_params(cfg["pair"], cfg["kn"], None, cfg["gamman"], None, cfg["xmu"]),
                           frozen=frozen, group=group), st


def _assert_rows(got, want, what):
    got = _by_tags(got)
    assert got["tag1"].tolist() == want["tag1"].tolist() and got["tag2"].tolist() == want["tag2"].tolist(), what
    errs = cm.column_errors(got, want)
    print("%s: %d rows, rel %s" % (what, len(want["dist"]), {k: "%.2e" % e for k, e in errs.items()}))
    for k, e in errs.items():
        assert e <= cm.GATE, (what, k, e)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the commands and the query exist

def test_compute_dump_local_and_contacts_are_known(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute 1 all pair/local " + " ".join(VALUES))
    lmp.command("compute g all gran/local tag1 tag2 eng dist force fx fy fz")   # BL24-TH1/in.lammps:33, the reference's name
    lmp.command("dump contact all local 10 %s index c_1[1] c_1[3] c_1[11] c_1[12]" % (tmp_path / "dump.contact"))
    lmp.command("run 0")
    rows = lmp.contacts()
    assert set(rows) == {"tag1", "tag2", "dist", "force", "f", "fs", "fsmag"}
    assert len(rows["tag1"]) > 4 * len(bed["x"]) and (rows["tag1"] < rows["tag2"]).all()
    assert lmp.contact_launches() >= 3
    lmp.command("undump contact")
    lmp.command("uncompute 1")
    lmp.command("uncompute g")
    with pytest.raises(SfError, match="Could not find compute ID to delete"):
        lmp.command("uncompute g")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rows are the engine's pair forces

@pytest.mark.parametrize("style", sorted(STYLES))
def test_rows_summed_per_atom_are_the_engines_forces(style):
    """pair forces only, run 0: the setup evaluation has shearupdate = 0 and the velocities the rows see"""
    bed, cfg = _small(style, wall=False)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 0")
    rows, st = lmp.contacts(), lmp.get_state()
    err = dc.rel_err(cm.per_atom_sums(rows, st["tag"]), st["f"])
    print("sum rule (%s): %d rows, rel %.3e" % (style, len(rows["tag1"]), err))
    assert len(rows["tag1"]) > 4 * len(bed["x"])
    assert err <= cm.GATE


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the model after motion

@pytest.mark.parametrize("style", sorted(STYLES))
def test_rows_after_motion_are_the_models(style):
    bed, cfg = _small(style)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 40")
    want, st = _model(bed, cfg, lmp)
    hist = lmp.history()
    assert set(zip(want["tag1"].tolist(), want["tag2"].tolist())) == set(hist)
    got = _assert_rows(lmp.contacts(), want, "after 40 steps (%s)" % style)
    assert set(zip(got["tag1"].tolist(), got["tag2"].tolist())) == set(hist)
    # what the input must exercise: sliding and sticking contacts, and pairs across a periodic face
    fscale = float(np.max(np.abs(got["force"])))
    capped = np.abs(got["fsmag"] - cfg["xmu"] * np.abs(got["force"])) <= cm.GATE * fscale
    assert 0.1 <= capped.mean() <= 0.9, capped.mean()
    assert (capped == want["capped"]).mean() > 0.99   # (the model's branch; a contact exactly at the cap may fall either way)
    pos = {int(t): k for k, t in enumerate(st["tag"])}
    raw = np.abs(np.array([st["x"][pos[int(a)]] - st["x"][pos[int(b)]] for a, b in zip(got["tag1"], got["tag2"])]))
    far = (raw > 0.5 * (np.asarray(bed["boxhi"]) - np.asarray(bed["boxlo"]))).any(axis=1)
    assert far.any() and (far == want["wrapped"]).all()
    if style != "hooke_plain":
        assert max(float(np.max(np.abs(s))) for s in hist.values()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. fix freeze

def test_rows_of_frozen_atoms_take_the_partners_mass():
    """a frozen bottom layer, pair forces only, run 0: every row matches the model with meff = the free partner's mass
    (pair_gran_hertzFix_history.cpp:188-189), the rows of a frozen atom differ from those without the override, and the
    rows sum to the forces of the atoms that are not frozen (fix freeze zeroes the others')"""
    bottom = lambda bed: (1 + (bed["x"][:, 1] < 0.8e-3)).astype(np.int32)
    bed, cfg = _small("hertz", wall=False, types=bottom, frozen_types=[2])
    frozen = bed["type"] == 2
    assert 10 <= frozen.sum() <= len(frozen) // 2
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 0")
    want, st = _model(bed, cfg, lmp, frozen=frozen)
    got = _assert_rows(lmp.contacts(), want, "fix freeze")
    plain, _ = _model(bed, cfg, lmp)
    touches = frozen[got["tag1"] - 1] | frozen[got["tag2"] - 1]
    assert touches.any() and not touches.all()
    assert float(np.max(np.abs(plain["force"][touches] - got["force"][touches]))) > 1e-6 * float(np.max(np.abs(got["force"])))
    free = ~frozen
    err = dc.rel_err(cm.per_atom_sums(got, st["tag"])[free], st["f"][free])
    print("sum rule, unfrozen atoms: rel %.3e" % err)
    assert err <= cm.GATE
    assert not st["f"][frozen].any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. group

def test_rows_of_a_group_are_the_rows_of_all_between_its_atoms():
    every_third = lambda bed: (1 + (np.arange(len(bed["x"])) % 3 == 0)).astype(np.int32)
    bed, cfg = _small(types=every_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    lmp.command("run 25")
    rows_all, rows_two = lmp.contacts(), lmp.contacts("two")
    in_two = bed["type"] == 2
    keep = in_two[rows_all["tag1"] - 1] & in_two[rows_all["tag2"] - 1]
    assert 0 < keep.sum() < len(keep)
    for k in rows_all:
        assert rows_two[k].tobytes() == rows_all[k][keep].tobytes(), k   # the same rows, order and bits


# ---------------------------------------------------------------------------------------------------------------------
# 6. text

def local_frames(path):
    """[(step, rows, header lines, [line bytes])] of a dump local file"""
    out = []
    for blk in open(path, "rb").read().split(b"ITEM: TIMESTEP\n")[1:]:
        lines = blk.split(b"\n")
        step = int(lines[0])
        assert lines[1] == b"ITEM: NUMBER OF ENTRIES"
        n = int(lines[2])
        assert lines[3].startswith(b"ITEM: BOX BOUNDS ")
        assert lines[7].startswith(b"ITEM: ENTRIES ")
        rows = [ln + b"\n" for ln in lines[8:8 + n]]
        assert len(rows) == n and lines[8 + n:] == [b""]
        out.append((step, n, lines[3:8], rows))
    return out


def _lines(rows, cols):
    """the Python formatting of the rows contacts() returned: index and the tags "%d ", everything else "%g " """
    col = cm.columns(rows)
    out = []
    for r in range(len(rows["tag1"])):
        s = ""
        for c in cols:
            if c == "index":
                s += "%d " % (r + 1)
            elif c in ("tag1", "tag2"):
                s += "%d " % rows[c][r]
            else:
                s += "%g " % (0.0 if c == "eng" else col[c][r])
        out.append((s + "\n").encode())
    return out


def test_dump_local_is_the_text_of_contacts(tmp_path):
    one_lone = lambda bed: (1 + 2 * (np.arange(len(bed["x"])) == 40)).astype(np.int32)
    bed, cfg = _small(types=one_lone)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group lone type 3")   # one atom: in the group, and no pair
    lmp.command("compute 1 all pair/local " + " ".join(VALUES))
    lmp.command("compute 2 all pair/local force")
    lmp.command("compute 3 lone pair/local dist force")
    cols = "index " + " ".join("c_1[%d]" % (k + 1) for k in range(len(VALUES)))
    lmp.command("dump a all local 15 %s %s" % (tmp_path / "a.contact", cols))
    lmp.command("dump b all local 15 %s c_2 index" % (tmp_path / "b.*"))
    lmp.command("dump c all local 15 %s index c_3[1] c_3[2]" % (tmp_path / "c.contact"))
    lmp.command("run 0")
    seen = [lmp.contacts()]
    for _ in range(2):
        lmp.step(15)
        seen.append(lmp.contacts())
    lmp.sync()
    fr = local_frames(str(tmp_path / "a.contact"))
    assert [f[0] for f in fr] == [0, 15, 30]
    lo, hi = bed["boxlo"], bed["boxhi"]
    for f, rows in zip(fr, seen):
        assert f[1] == len(rows["tag1"]) > 4 * len(bed["x"])
        assert f[2][0] == b"ITEM: BOX BOUNDS pp ff pp" and f[2][1:4] == [(b"%g %g" % (lo[k], hi[k])) for k in range(3)]
        assert f[2][4] == ("ITEM: ENTRIES " + cols).encode()
        assert f[3] == _lines(rows, ["index"] + VALUES)
    assert sorted(os.listdir(tmp_path)) == ["a.contact", "b.0", "b.15", "b.30", "c.contact"]
    for s, rows in zip((0, 15, 30), seen):
        fb = local_frames(str(tmp_path / ("b.%d" % s)))
        assert len(fb) == 1 and fb[0][0] == s and fb[0][2][4] == b"ITEM: ENTRIES c_2 index"
        assert fb[0][3] == _lines(rows, ["force", "index"])
    assert (tmp_path / "c.contact").read_bytes().split(b"ITEM: TIMESTEP\n")[1:] == [
        (b"%d\nITEM: NUMBER OF ENTRIES\n0\nITEM: BOX BOUNDS pp ff pp\n%g %g\n%g %g\n%g %g\nITEM: ENTRIES index c_3[1] c_3[2]\n"
         % (s, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])) for s in (0, 15, 30)]
    assert len(lmp.contacts("lone")["tag1"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. passive

def test_a_run_with_contact_output_ends_in_the_bits_of_the_run_without(tmp_path):
    """the walled 5 k-grain Hertz bed of tests/test_dump_gpu.py, 60 + 35 + 60 + 50 steps with `dump custom` every 37; the same
    with a `dump local` every 37 and a contacts() call between the pieces.  Both runs are cut at the same steps, so they end
    with the same rebuilds and the same bits: the contact kernels only read"""
    bed = synthetic.fcc_bed((11, 11, 11), seed=5, vmax=0.8)
    bed["periodic"] = (0, 0, 0)
    bed["x"][:, 0] += 0.3e-3
    bed["x"][:, 2] += 0.3e-3
    bed["boxhi"][0] += 0.6e-3
    bed["boxhi"][2] += 0.6e-3
    walls = [(1, float(bed["boxlo"][1]), float(bed["boxhi"][1])), (0, float(bed["boxlo"][0]), float(bed["boxhi"][0])),
             (2, float(bed["boxlo"][2]), float(bed["boxhi"][2]))]
    cfg = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.04e-3, walls=walls)
    assert 4000 <= len(bed["x"]) <= 8000
    outs = []
    for with_contacts in (False, True):
        lmp = dc.make_hip(bed, cfg)
        lmp.command("dump d all custom 37 %s id x y z fx fy fz" % (tmp_path / ("bed%d.dump" % with_contacts)))
        if with_contacts:
            lmp.command("compute 1 all pair/local " + " ".join(VALUES))
            lmp.command("dump c all local 37 %s index c_1[1] c_1[3] c_1[7] c_1[11] c_1[12]" % (tmp_path / "bed.contact"))
        lmp.setup()
        nrows = []
        for n in (60, 35, 60, 50):
            lmp.step(n)
            if with_contacts:
                nrows.append(len(lmp.contacts()["tag1"]))
        lmp.sync()
        outs.append((lmp.get_state(), lmp.history(), lmp.info().nbuilds))
    assert outs[0][2] == outs[1][2] and outs[0][2] >= 3
    for k in ("tag", "x", "v", "omega", "f", "torque"):
        assert outs[0][0][k].tobytes() == outs[1][0][k].tobytes(), k
    assert set(outs[0][1]) == set(outs[1][1])
    assert all(outs[0][1][p].tobytes() == outs[1][1][p].tobytes() for p in outs[0][1])
    fr = local_frames(str(tmp_path / "bed.contact"))
    assert [f[0] for f in fr] == [0, 37, 74, 111, 148, 185]
    assert all(f[1] > 2 * len(bed["x"]) for f in fr) and min(nrows) > 2 * len(bed["x"])
    assert len(outs[1][1]) == nrows[-1]
    assert (tmp_path / "bed0.dump").read_bytes() == (tmp_path / "bed1.dump").read_bytes()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals

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


@pytest.mark.parametrize("make,before,line,msg", [
    (_with_lubrication, [], "compute 1 all pair/local dist", "Pair style does not support compute pair/local"),
    (_without_pair_style, [], "compute 1 all pair/local dist", "No pair style is defined for compute pair/local"),
    (_plain, ["fix r all rigid/nve single"], "compute 1 all pair/local dist", "not while fix rigid/nve exists"),
    (_plain, [], "compute 1 all pair/local dist fq", "Invalid keyword in compute pair/local command: fq"),
    (_plain, [], "compute 1 all pair/local dist p5",
     "Pair style does not have extra field requested by compute pair/local"),
    (_plain, [], "compute 1 all cohe/local dist", "compute cohe/local is not built"),
    (_plain, [], "compute 1 all temp", "Invalid compute style temp"),
    (_plain, ["compute 1 all pair/local dist force"], "dump d all local 10 {p} index c_1[3]",
     "Dump local compute vector is accessed out-of-range"),
    (_plain, ["compute 1 all pair/local dist force"], "dump d all local 10 {p} index c_1",
     "Dump local compute does not compute local vector"),
    (_plain, ["compute 1 all pair/local dist", "compute 2 all pair/local force"], "dump d all local 10 {p} c_1 c_2",
     "every c_ column must name the same compute"),
    (_plain, ["compute 1 all pair/local dist"], "dump d all local 10 {p} index c_9[1]",
     "Could not find dump local compute ID 9"),
    (_plain, ["compute 1 all pair/local dist"], "dump d all local 10 {p} index c_1 x", "Invalid attribute x in dump local"),
    (_plain, ["compute 1 all pair/local dist"], "dump d all local 10 {p}.gz index c_1", "compressed"),
    (_plain, ["compute 1 all pair/local dist"], "dump d all local 10 {p}.% index c_1", "one rank and one file only"),
    (_plain, ["compute 1 all pair/local dist", "dump d all local 10 {p} index c_1"], "dump_modify d sort id",
     "on a dump local is not supported"),
    (_plain, ["compute 1 all pair/local dist", "dump d all local 10 {p} index c_1"], "uncompute 1",
     "a dump local still uses this compute"),
    (_plain, ["compute 1 all pair/local dist"], "compute 1 all pair/local force", "Reuse of compute ID"),
])
def test_refused_forms(make, before, line, msg, tmp_path):
    lmp = make()
    for b in before:
        lmp.command(b.format(p=tmp_path / "r.contact"))
    with pytest.raises(SfError, match=re.escape(msg)):
        lmp.command(line.format(p=tmp_path / "r.contact"))


def test_contacts_before_the_first_run_and_with_a_rigid_fix_later_are_refused():
    lmp = _plain()
    with pytest.raises(SfError, match="no neighbour list yet"):
        lmp.contacts()
    lmp.command("compute 1 all pair/local dist")
    lmp.command("fix r all rigid/nve single")
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.contacts()
