"""`thermo N`, `thermo_style one | custom`, `thermo_modify`, `units`, `log`, `echo` and -log / -screen (csrc/sf_thermo.hip):
the LAMMPS schedule and columns, the kinetic terms from the state, the pair virial against sum_i (x_i - xbar) (x) f_i on beds
whose only forces are pair forces, runs cut at thermo steps that end where uncut runs end, and the refused settings."""
import os

import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError
from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

CUSTOM = "step atoms temp ke etotal press pxx pyy pzz pxy pxz pyz vol fmax fnorm time dt"


def _bed(periodic=True, seed=5, vmax=0.05, ncells=(4, 3, 4), pair="hertz"):
    import tests.test_dem_gpu as T
    bed = T._bed(ncells, periodic=periodic, seed=seed, vmax=vmax)
    cfg = dict(T.BASE, pair=pair)
    cfg["walls"] = T._walls(bed)
    return bed, cfg


def _blocks(path):
    """[(header, [value rows], loop line)] of a log, echoed input lines skipped"""
    out, cur = [], None
    for ln in open(path).read().split("\n"):
        if ln.startswith("Step ") and ln.endswith(" "):
            cur = (ln, [], None)
        elif cur is not None and ln.startswith("Loop time of "):
            out.append((cur[0], cur[1], ln))
            cur = None
        elif cur is not None and ln.strip() and ln.endswith(" "):
            cur[1].append(ln)
    return out


def _mass(bed):
    r = np.asarray(bed["diameter"]) / 2.0
    return 4.0 * np.pi / 3.0 * r * r * r * np.asarray(bed["density"])


def _kin(lmp, bed):
    st = lmp.get_state()
    m = _mass(bed)[st["tag"] - 1]
    v = st["v"]
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    return np.array([np.sum(m * v[:, a] * v[:, b]) for a, b in pairs]), st


def _virial(lmp, K):
    vol = lmp.get_thermo("vol")
    return np.array([lmp.get_thermo(k) for k in ("pxx", "pyy", "pzz", "pxy", "pxz", "pyz")]) * vol - K


def _xf(st):
    x = st["x"] - st["x"].mean(axis=0)
    f = st["f"]
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    return np.array([np.sum(x[:, a] * f[:, b]) for a, b in pairs])


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def test_schedule_columns_and_nothing_without_a_destination(tmp_path):
    """thermo 7: run 20, run 10, lammps_step(5) write lines at 0 7 14 20 | 20 21 28 30 | 30 35, a header before and a
    `Loop time` line after each run; the last line re-formatted from get_thermo is byte-identical; `run 0` writes one
    line; with no destination nothing is written and no thermo kernel is launched"""
    bed, cfg = _bed()
    log = str(tmp_path / "log.lammps")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("log " + log)
    lmp.commands("thermo_style custom %s\nthermo 7\nthermo_modify lost error flush yes" % CUSTOM)
    lmp.command("run 20")
    lmp.command("run 10")
    lmp.step(5)
    lmp.command("log none")
    assert lmp.thermo_launches() > 0
    bl = _blocks(log)
    assert [[int(r.split()[0]) for r in b[1]] for b in bl] == [[0, 7, 14, 20], [20, 21, 28, 30], [30, 35]]
    hdr = "Step Atoms Temp KinEng TotEng Press Pxx Pyy Pzz Pxy Pxz Pyz Volume Fmax Fnorm Time Dt "
    assert all(b[0] == hdr for b in bl)
    n = len(bed["x"])
    for b, steps in zip(bl, (20, 10, 5)):
        assert b[2].startswith("Loop time of ") and b[2].endswith(" on 1 procs for %d steps with %d atoms" % (steps, n))
    last = bl[-1][1][-1]
    want = ""
    for k in CUSTOM.split():
        v = lmp.get_thermo(k)
        want += ("%8ld " % int(v)) if k in ("step", "atoms") else ("%12.8g " % v)
    assert last == want
    assert lmp.get_thermo("time") == pytest.approx(35 * cfg["dt"], rel=1e-12)
    txt = open(log).read()
    assert "thermo 7\n" in txt and "run 20\n" in txt   # echo log (the default)
    lmp.close()

    # run 0: one line
    log0 = str(tmp_path / "log0")
    lmp = dc.make_hip(bed, cfg)
    lmp.commands("log %s\nthermo 7\nrun 0" % log0)
    bl = _blocks(log0)
    assert len(bl) == 1 and len(bl[0][1]) == 1 and int(bl[0][1][0].split()[0]) == 0
    assert bl[0][0] == "Step Temp E_pair E_mol TotEng Press "
    lmp.close()

    # no destination: nothing written, no kernel launched, get_thermo has nothing to return
    lmp = dc.make_hip(bed, cfg)
    lmp.commands("thermo_style one\nthermo 7\nrun 20")
    lmp.step(5)
    assert lmp.thermo_launches() == 0
    with pytest.raises(SfError, match="no thermo line"):
        lmp.get_thermo("temp")
    lmp.close()


def test_log_and_screen_from_arguments(tmp_path):
    """-log FILE and -screen FILE of sf_lammps_open; `echo none` keeps the input out of the log"""
    bed, cfg = _bed()
    log, scr = str(tmp_path / "a.log"), str(tmp_path / "a.screen")
    lmp = Lammps(args=["-log", log, "-screen", scr])
    lmp.set_box(bed["boxlo"], bed["boxhi"])
    lmp.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"])
    lmp.command("echo none")
    for line in dc.script_lines(bed, cfg):
        lmp.command(line)
    lmp.commands("thermo 5\nrun 10")
    lmp.close()
    a, b = open(log).read(), open(scr).read()
    assert [[int(r.split()[0]) for r in blk[1]] for blk in _blocks(log)] == [[0, 5, 10]]
    assert _blocks(log)[0][1] == _blocks(scr)[0][1]
    assert "pair_style" not in a and "pair_style" not in b


def test_kinetic_terms_and_norm(tmp_path):
    """temp, ke and the kinetic part of the pressure tensor from sum m v v of the state (a bed without contacts: W = 0);
    norm yes under lj, no under si, and thermo_modify norm flips it"""
    bed, cfg = _bed(periodic=True, vmax=0.3)
    # (the lattice spacing 0.98 d overlaps: spread it so that nothing touches)
    bed["x"] = bed["boxlo"] + (bed["x"] - bed["boxlo"]) * 1.1
    bed["boxhi"] = bed["boxlo"] + (bed["boxhi"] - bed["boxlo"]) * 1.1
    n = len(bed["x"])
    for units, norm in (("lj", True), ("si", False)):
        lmp = Lammps()
        lmp.command("units " + units)
        lmp.set_box(bed["boxlo"], bed["boxhi"])
        lmp.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"])
        for line in dc.script_lines(bed, dict(cfg, g=0.0, walls=[])):
            lmp.command(line)
        lmp.commands("log %s\nthermo_style custom %s\nthermo 10\nrun 10" % (tmp_path / ("k" + units), CUSTOM))
        K, st = _kin(lmp, bed)
        mv2 = K[0] + K[1] + K[2]
        boltz = 1.0 if units == "lj" else 1.3806504e-23
        assert lmp.get_thermo("temp") == pytest.approx(mv2 / ((3 * n - 3) * boltz), rel=1e-12)
        assert lmp.get_thermo("ke") == pytest.approx(0.5 * mv2 / (n if norm else 1), rel=1e-12)
        assert lmp.get_thermo("etotal") == lmp.get_thermo("ke")
        vol = lmp.get_thermo("vol")
        assert np.prod(bed["boxhi"] - bed["boxlo"]) == pytest.approx(vol, rel=1e-14)
        P = np.array([lmp.get_thermo(k) for k in ("pxx", "pyy", "pzz", "pxy", "pxz", "pyz")])
        assert _rel(P * vol, K) <= 1e-12
        assert lmp.get_thermo("press") == pytest.approx(mv2 / (3 * vol), rel=1e-12)
        assert lmp.get_thermo("fnorm") == pytest.approx(np.sqrt(np.sum(st["f"] ** 2)), rel=1e-12)
        assert lmp.get_thermo("fmax") == np.max(np.abs(st["f"]))
        lmp.commands("thermo_modify norm %s\nrun 0" % ("no" if norm else "yes"))
        K, _ = _kin(lmp, bed)
        mv2 = K[0] + K[1] + K[2]
        assert lmp.get_thermo("ke") == pytest.approx(0.5 * mv2 / (1 if norm else n), rel=1e-12)
        lmp.commands("thermo_style custom step ke\nrun 0")   # a new style: norm back to the units' default
        assert lmp.get_thermo("ke") == pytest.approx(0.5 * mv2 / (n if norm else 1), rel=1e-12)
        lmp.close()


def _pair_only(bed, pair):
    """a closed bed, pair forces only (no gravity, walls, drag)"""
    bed = dict(bed, boxlo=bed["boxlo"] - 1e-3, boxhi=bed["boxhi"] + 1e-3) if not any(bed["periodic"]) else bed
    style = {"hertz": "gran/hertzFix/history 1e7 NULL 0.5 NULL 0.4 1", "hooke": "gran/hooke/history 1e3 NULL 0.5 NULL 0.4 1",
             "lub": "lubricate/poly 1.0e-3 1 0 1.001e-3 1.1e-3 1 1"}[pair]
    lmp = Lammps()
    lmp.set_box(bed["boxlo"], bed["boxhi"])
    lmp.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"])
    lmp.commands("""atom_style sphere
        boundary %s %s %s
        newton off
        communicate single vel yes
        neighbor 0.25e-3 bin
        neigh_modify delay 0
        pair_style %s
        pair_coeff * *
        timestep 1e-6
        fix 1 all nve/sphere""" % (tuple("p" if q else "f" for q in bed["periodic"]) + (style,)))
    return lmp


@pytest.mark.parametrize("pair", ["hertz", "hooke", "lub"])
def test_virial_is_sum_of_x_times_f(tmp_path, pair):
    """non-periodic bed with initial overlaps and random velocities, pair forces only: W_ab = sum_i (x_i - xbar)_a f_i,b
    at the setup line and at a thermo step inside the run"""
    bed, _ = _bed(periodic=False, seed=9, vmax=0.05)
    lmp = _pair_only(bed, pair)
    lmp.commands("log %s\nthermo_style custom %s\nthermo 3\nrun 0" % (tmp_path / "v.log", CUSTOM))
    K, st = _kin(lmp, bed)
    W = _virial(lmp, K)
    assert np.max(np.abs(W)) > 0.0
    assert _rel(W, _xf(st)) <= 1e-10, (W, _xf(st))
    lmp.command("run 6")
    K, st = _kin(lmp, bed)
    assert lmp.get_thermo("step") == 6
    assert _rel(_virial(lmp, K), _xf(st)) <= 1e-10
    lmp.close()


def test_virial_across_a_periodic_face(tmp_path):
    """two grains touching across the periodic x face: W = del (x) f_i with the minimum image"""
    d = 1e-3
    bed = dict(x=np.array([[0.45e-3, 2e-3, 2e-3], [4e-3 - 0.5e-3, 2e-3, 2e-3]]), v=np.array([[0.01, 0.02, -0.01], [0, 0, 0.0]]),
               diameter=np.array([d, d]), density=np.array([2650.0, 2650.0]), boxlo=np.zeros(3),
               boxhi=np.array([4e-3, 4e-3, 4e-3]), periodic=(1, 0, 0))
    lmp = _pair_only(bed, "hertz")
    lmp.commands("log %s\nthermo_style custom %s\nrun 0" % (tmp_path / "p.log", CUSTOM))
    K, st = _kin(lmp, bed)
    W = _virial(lmp, K)
    i = 0
    dl = st["x"][0] - st["x"][1]
    dl[0] -= 4e-3 * np.round(dl[0] / 4e-3)
    f = st["f"][i]
    want = np.array([dl[0] * f[0], dl[1] * f[1], dl[2] * f[2], dl[0] * f[1], dl[0] * f[2], dl[1] * f[2]])
    assert abs(f[0]) > 0
    assert _rel(W, want) <= 1e-10


def test_fixes_leave_the_virial_unchanged(tmp_path):
    """walls and gravity (at the setup evaluation) and fix cohesive (at step 1) change forces, not the pair virial"""
    bed, _ = _bed(periodic=False, seed=11, vmax=0.05)
    got = []
    for extra in ([], ["fix g all gravity 9.81 vector 0 -1 0",
                       "fix w all wall/granFix 1e7 NULL 0.5 NULL 0.4 1 yplane %.17g %.17g" % (bed["boxlo"][1], bed["boxhi"][1])]):
        lmp = _pair_only(bed, "hertz")
        lmp.commands("\n".join(extra + ["log %s" % (tmp_path / "f.log"), "thermo_style custom %s" % CUSTOM, "run 0"]))
        got.append((_virial(lmp, _kin(lmp, bed)[0]), lmp.get_thermo("fnorm")))
        lmp.close()
    assert _rel(got[1][0], got[0][0]) <= 1e-12 and got[1][1] != got[0][1]
    got = []
    for extra in ([], ["fix c all cohesive 1e-13 1e-7 1e-7 1e-4 1"]):
        lmp = _pair_only(bed, "hertz")
        lmp.commands("\n".join(extra + ["log %s" % (tmp_path / "c.log"), "thermo_style custom %s" % CUSTOM, "run 1"]))
        got.append((_virial(lmp, _kin(lmp, bed)[0]), lmp.get_thermo("fnorm")))
        lmp.close()
    assert _rel(got[1][0], got[0][0]) <= 1e-12 and got[1][1] != got[0][1]


def test_cut_runs_match_and_logs_repeat(tmp_path):
    """run 200 with thermo 10 ends in the state of run 200 without thermo (1e-12); two identical runs write identical logs
    apart from the Loop time line; a line inside a run equals the last line of a twin run stopped at that step"""
    bed, cfg = _bed(periodic=True, seed=3, vmax=0.3)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 200")
    ref = lmp.get_state()
    lmp.close()
    logs = []
    for k in range(2):
        logs.append(str(tmp_path / ("r%d.log" % k)))
        lmp = dc.make_hip(bed, cfg)
        lmp.commands("log %s\nthermo_style custom %s\nthermo 10\nrun 200\nlog none" % (logs[-1], CUSTOM))
        st = lmp.get_state()
        lmp.close()
        for key in ("x", "v", "omega", "f"):
            assert dc.rel_err(st[key], ref[key]) <= 1e-12, key
    strip = [[ln for ln in open(p).read().split("\n") if not ln.startswith("Loop time") and not ln.startswith("log ")]
             for p in logs]
    assert strip[0] == strip[1]
    vals = {}
    for n in (20, 14):
        lmp = dc.make_hip(bed, cfg)
        lmp.commands("log %s\nthermo_style custom %s\nthermo 7\nrun %d" % (tmp_path / "t.log", CUSTOM, n))
        vals[n] = [r for r in _blocks(str(tmp_path / "t.log"))[0][1] if int(r.split()[0]) == 14][0]
        lmp.close()
    assert vals[20] == vals[14]


def test_refused_settings():
    bed, cfg = _bed()
    lmp = dc.make_hip(bed, cfg)
    for line, msg in (("thermo_style multi", "multi"), ("thermo_style custom step bogus", "bogus"),
                      ("thermo_modify lost ignore", "lost ignore"), ("thermo_modify format float %g", "format"),
                      ("thermo_modify norm maybe", "thermo_modify"), ("thermo -1", "thermo"), ("log", "log")):
        with pytest.raises(SfError, match=msg):
            lmp.command(line)
    with pytest.raises(SfError, match="unknown thermo keyword"):
        lmp.get_thermo("bogus")
    lmp.close()
