"""Checkpoints on the GPU: `write_restart` / `read_restart` / `restart N` against sedifoam_amd/restart.py (the format's
specification), continuation runs against the run that was not interrupted by a file, and the restart schedule.

Tolerances: what the engine writes and what restart.py reads are the same bits (array_equal, byte-equal files).  A
continued run performs the operations of the run it continues on the same state and may differ in summation order only
(atom order on arrival, list heuristics): rel <= 1e-9, the tol_x of tests/test_dem_gpu.py.  A run cut by `restart N`
against the uncut run: rel <= 1e-12, the bound of test_cut_runs_match_and_logs_repeat in tests/test_thermo_gpu.py."""
import os

import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError, restart
from tests import dem_cases as dc
from tests.test_dem_gpu import BASE, _bed, _walls

pytestmark = pytest.mark.gpu

TOL = 1e-9
HOT = dict(BASE, skin=0.03e-3)   # a thin skin: the hot bed below rebuilds every few dozen sub-steps


def _closed_bed(seed=5, **kw):
    return _bed((5, 5, 5), periodic=False, seed=seed, vmax=0.5, **kw)


def _sheared(bed, v=0.5):
    w = _walls(bed)
    w[0] = w[0] + ({"shear": (0, v)},)   # the floor and lid slide along x: wall history stays alive
    return w


def _resume(path, bed, cfg, groups=True):
    """a new engine that reads `path` and is then given the script's pair_style / neighbor / fix lines again"""
    lmp = Lammps()
    lmp.read_restart(path)
    for line in dc.script_lines(bed, cfg):
        # (box, periodicity and the timestep are the file's: neither line is given again)
        if line.startswith(("boundary", "timestep")) or (line.startswith("group") and not groups):
            continue
        lmp.command(line)
    return lmp


def _snapshot(lmp, nwalls):
    st = lmp.get_state()
    st["hist"] = lmp.history()
    st["wall"] = [lmp.wall_shear(w) for w in range(nwalls)]
    st["nbuilds"] = lmp.info().nbuilds
    st["nsteps"] = lmp.info().nsteps
    return st


def _worst(a, b, keys=("x", "v", "omega")):
    """largest relative difference of two snapshots (identical tags and contact pairs are asserted)"""
    assert np.array_equal(a["tag"], b["tag"])
    assert set(a["hist"]) == set(b["hist"])
    err = {k: dc.rel_err(a[k], b[k]) for k in keys}
    if a["hist"]:
        ks = sorted(a["hist"])
        err["hist"] = dc.rel_err(np.array([a["hist"][k] for k in ks]), np.array([b["hist"][k] for k in ks]))
    for w, (p, q) in enumerate(zip(a["wall"], b["wall"])):
        err["wall%d" % w] = dc.rel_err(p, q)
    return err


def test_file_matches_engine_state_bit_for_bit(tmp_path):
    bed = _closed_bed()
    cfg = dict(HOT, walls=_sheared(bed))
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 120")
    assert lmp.info().nbuilds >= 2
    F = str(tmp_path / "F.sfr")
    lmp.command("write_restart " + F)
    assert not os.path.exists(F + ".tmp")
    st, eng = restart.read(F), lmp.get_state()
    assert st["step"] == 120 and st["dt"] == cfg["dt"] and st["units"] == "lj"
    assert np.array_equal(st["boxlo"], bed["boxlo"]) and np.array_equal(st["boxhi"], bed["boxhi"])
    assert tuple(st["periodic"]) == tuple(bed["periodic"]) and st["groups"] == [("all", 1)]
    assert np.array_equal(st["tag"], eng["tag"])
    for k in ("x", "v", "omega"):
        assert np.array_equal(st[k], eng[k]), k
    r = 0.5 * np.asarray(bed["diameter"])
    assert np.array_equal(st["radius"], r) and (st["type"] == 1).all() and (st["mask"] == 1).all()
    assert np.array_equal(st["rmass"], 4.0 * np.pi / 3.0 * r * r * r * np.asarray(bed["density"]))
    hist, saved = lmp.history(), restart.contacts(st)
    nonzero = sum(1 for s in saved.values() if np.any(s != 0.0))
    print("contacts in the file: %d, with non-zero shear: %d" % (len(saved), nonzero))
    assert nonzero >= 100
    assert set(saved) == set(hist)
    assert all(np.array_equal(saved[k], hist[k]) for k in hist)
    assert [w["id"] for w in st["walls"]] == ["w0", "w1", "w2"]
    touching = 0
    for w in range(3):
        dense = restart.wall_rows(st, w)
        assert np.array_equal(dense, lmp.wall_shear(w))
        touching += int((np.abs(dense).sum(axis=1) > 0).sum())
    print("wall rows with non-zero shear: %d" % touching)
    assert touching >= 10

    # a fresh engine reads F, is given the fixes and writes G without running: the same bytes
    fresh = Lammps()
    fresh.read_restart(F)   # (before any script line: what the file itself restores)
    assert fresh.get_timestep() == cfg["dt"] and fresh.info().nsteps == 120 and fresh.get_local_n() == len(st["tag"])
    B = _resume(F, bed, cfg)
    G = str(tmp_path / "G.sfr")
    B.write_restart(G)
    assert open(G, "rb").read() == open(F, "rb").read()
    assert B.info().nsteps == 120 and B.get_timestep() == cfg["dt"]

    # ... and so does a file restart.py made from hand-built arrays
    n = len(st["tag"])
    rng = np.random.default_rng(3)
    hand = dict(st)
    hand["step"] = 7
    for k in ("v", "omega", "fdrag", "DuDt", "vOld"):
        hand[k] = rng.normal(size=(n, 3))
    hand["foamCpuId"] = rng.integers(0, 4, n).astype(np.int32)
    hand["contact_shear"] = rng.normal(size=st["contact_shear"].shape)
    hand["walls"] = [dict(id=w["id"], tag=w["tag"], shear=rng.normal(size=w["shear"].shape)) for w in st["walls"]]
    H1, H2 = str(tmp_path / "H1.sfr"), str(tmp_path / "H2.sfr")
    restart.write(H1, hand)
    C = _resume(H1, bed, cfg)
    C.write_restart(H2)
    assert open(H2, "rb").read() == open(H1, "rb").read()


def _frozen_bed():
    bed = _closed_bed(seed=9)
    y = bed["x"][:, 1]
    bed["type"] = np.where(y < y.min() + 0.3e-3, 2, 1).astype(np.int32)   # the lowest layer is the fixed one
    return bed


CASES = {
    "hertz_plane_walls": lambda: (_closed_bed(), dict(HOT), None, True),
    "sheared_wall": lambda: (_closed_bed(seed=7), dict(HOT), "shear", True),
    "hooke_history": lambda: (_closed_bed(seed=8), dict(HOT, pair="hooke", kn=2.0e5), None, True),
    "freeze_without_group_lines": lambda: (_frozen_bed(), dict(HOT, frozen_types=[2], freeze_first=True), None, False),
    "overlay_lubricate_cohesive": lambda: (
        _bed((5, 5, 5), periodic=True, seed=11, poly=(0.85e-3, 1.0e-3), spacing=0.95, vmax=0.3),
        dict(HOT, cohesive=(1.0e-13, 1.0e-7, 1.0e-7, 1.0e-4, 1), lub=(1.0e-3, 1, 1, 1.001e-3, 1.1e-3, 1, 1)), None, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_continuation_matches_the_run_it_continues(case, tmp_path):
    """A: run k, write_restart F, setup(), run m.  B: new engine, read_restart F, the same lines, run m.  Measured on an
    MI355X (worst relative difference over x, v, omega, history, wall shear): hertz 3.0e-16, sheared wall 3.0e-16,
    hooke/history 3.8e-12, fix freeze 0, overlay with lubricate/poly and fix cohesive 2.7e-14; the control leg misses by
    1.6e-1; the uninterrupted run differs from the continued one by 9.3e-7 (x), 9.8e-5 (v), 2.3e-4 (omega)."""
    bed, cfg, motion, groups = CASES[case]()
    cfg["walls"] = _sheared(bed) if motion == "shear" else _walls(bed)
    nw = len(cfg["walls"])
    k, m = 100, 100
    A = dc.make_hip(bed, cfg)
    A.command("log %s" % (tmp_path / "A.log"))   # (a thermo destination: get_thermo needs a line)
    A.command("thermo 50")
    A.command("run %d" % k)
    F = str(tmp_path / "F.sfr")
    A.command("write_restart " + F)
    builds_k = A.info().nbuilds
    A.setup()
    A.step(m)
    a = _snapshot(A, nw)
    assert a["nbuilds"] >= builds_k + 2   # (the setup's own build and at least one more during run m)
    B = _resume(F, bed, cfg, groups=groups)
    B.command("log %s" % (tmp_path / "B.log"))
    B.command("thermo 50")
    B.step(m)
    b = _snapshot(B, nw)
    assert b["nbuilds"] >= 2 and a["nsteps"] == b["nsteps"] == k + m
    assert A.get_thermo("step") == B.get_thermo("step") == k + m
    assert A.get_thermo("time") == B.get_thermo("time") == (k + m) * cfg["dt"]
    err = _worst(a, b)
    print("continuation %s: %s" % (case, " ".join("%s=%.3e" % kv for kv in sorted(err.items()))))
    assert max(err.values()) <= TOL, err
    if case != "hertz_plane_walls":
        return
    # control: a checkpoint without its contact and wall sections must miss A by far, or the bed does not exercise history
    C0 = str(tmp_path / "C.sfr")
    restart.write(C0, restart.without_history(restart.read(F)))
    C = _resume(C0, bed, cfg)
    C.step(m)
    c = C.get_state()
    miss = max(dc.rel_err(c["v"], a["v"]), dc.rel_err(c["omega"], a["omega"]))
    print("control leg without history misses A by %.3e" % miss)
    assert miss >= 100 * TOL
    # the uninterrupted run differs by design (setup evaluation: shearupdate = 0, fix cohesive skipped): measured only
    U = dc.make_hip(bed, cfg)
    U.command("run %d" % (k + m))
    u = U.get_state()
    print("uninterrupted run %d vs continued: x %.3e v %.3e omega %.3e" % (
        k + m, dc.rel_err(u["x"], b["x"]), dc.rel_err(u["v"], b["v"]), dc.rel_err(u["omega"], b["omega"])))


def test_restart_schedule_and_files(tmp_path):
    bed = _closed_bed()
    cfg = dict(HOT, walls=_sheared(bed))

    def drive(lmp):
        lmp.command("run 25")
        lmp.command("run 10")
        lmp.step(5)

    d = str(tmp_path)
    R = dc.make_hip(bed, cfg)
    R.command("restart 10 %s/r.*" % d)
    drive(R)
    R2 = dc.make_hip(bed, cfg)
    R2.command("restart 10 %s/a %s/b" % (d, d))
    drive(R2)
    R.sync(); R2.sync()   # (lammps_step does not wait for the writer: sync does)
    # the same run without `restart`, cut by hand at the same steps: write_restart at each
    P = dc.make_hip(bed, cfg)
    for n, step in ((10, 10), (10, 20), (5, None), (5, 30), (5, None), (5, 40)):
        P.command("run %d" % n) if step != 40 else P.step(n)
        if step:
            P.write_restart("%s/p.%d" % (d, step))
    plain = dc.make_hip(bed, cfg)
    drive(plain)
    assert plain.restart_launches() == 0 and R.restart_launches() > 0
    plain.command("restart 0")
    plain.step(10)
    assert plain.restart_launches() == 0
    names = sorted(f for f in os.listdir(d) if f.startswith("r."))
    assert names == ["r.10", "r.20", "r.30", "r.40"]
    assert restart.header(d + "/a")["step"] == 40 and restart.header(d + "/b")["step"] == 30
    # each file against write_restart at that step of the same run without `restart` (cut by hand at the same steps)
    for step in (10, 20, 30, 40):
        assert open("%s/r.%d" % (d, step), "rb").read() == open("%s/p.%d" % (d, step), "rb").read(), step
    assert open(d + "/a", "rb").read() == open(d + "/r.40", "rb").read()
    assert open(d + "/b", "rb").read() == open(d + "/r.30", "rb").read()
    plain2 = dc.make_hip(bed, cfg)
    drive(plain2)
    a, b = R.get_state(), plain2.get_state()
    for k in ("x", "v", "omega", "f"):
        assert dc.rel_err(a[k], b[k]) <= 1e-12, k
    R.close(); R2.close()
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]


def test_step_numbering_goes_on_after_read_restart(tmp_path):
    bed = _closed_bed()
    cfg = dict(HOT, walls=_walls(bed))
    A = dc.make_hip(bed, cfg)
    A.command("run 30")
    F = str(tmp_path / "F.sfr")
    A.write_restart(F)
    B = _resume(F, bed, cfg)
    dump = str(tmp_path / "d.txt")
    B.command("dump 1 all custom 10 %s id x y z" % dump)
    B.command("restart 20 %s/c.*" % tmp_path)
    log = str(tmp_path / "B.log")
    B.command("log " + log)
    B.command("thermo_style custom step time ke")
    B.command("thermo 10")
    B.command("run 25")
    B.close()
    rows = [l.split() for l in open(log).read().splitlines() if l.split() and l.split()[0].isdigit()]
    assert [int(r[0]) for r in rows] == [30, 40, 50, 55]
    assert np.allclose([float(r[1]) for r in rows], [q * cfg["dt"] for q in (30, 40, 50, 55)], rtol=1e-5, atol=0)   # (print precision)
    text = open(dump).read().split("ITEM: TIMESTEP\n")[1:]
    assert [int(t.split("\n", 1)[0]) for t in text] == [30, 40, 50]
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("c.")) == ["c.40"]
    assert restart.header(str(tmp_path / "c.40"))["step"] == 40


def test_refusals(tmp_path):
    bed = _closed_bed()
    cfg = dict(HOT, walls=_walls(bed))
    empty = Lammps()
    with pytest.raises(SfError, match="Write_restart command before simulation box is defined"):
        empty.command("write_restart %s/x" % tmp_path)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 5")
    F = str(tmp_path / "F.sfr")
    lmp.write_restart(F)
    with pytest.raises(SfError, match="Cannot read_restart after simulation box is defined"):
        lmp.command("read_restart " + F)
    for bad in ("restart", "restart -1 x", "restart ten x", "restart 10", "restart 10 a b c", "restart 0 x"):
        with pytest.raises(SfError, match="Illegal restart command"):
            lmp.command(bad)
    with pytest.raises(SfError, match="%"):
        lmp.command("restart 10 %s/x.%%" % tmp_path)
    with pytest.raises(SfError, match="%"):
        lmp.command("write_restart %s/x.%%" % tmp_path)
    with pytest.raises(SfError, match="Cannot open restart file"):
        lmp.command("write_restart %s/no/such/dir/x" % tmp_path)
    # under lammps_step the writer's error arrives at the next point that waits for the files
    lmp.command("restart 5 %s/no/such/dir/y.*" % tmp_path)
    lmp.step(5)
    with pytest.raises(SfError, match="Cannot open restart file"):
        lmp.sync()
    lmp.command("restart 0")
    lmp.command("run 0")   # the engine stays usable
    lmp.write_restart(F)
    assert restart.header(F)["step"] == 10 and lmp.info().nsteps == 10
    cut = open(F, "rb").read()[:-40]
    open(F + ".cut", "wb").write(cut)
    with pytest.raises(SfError, match="is truncated"):
        Lammps().read_restart(F + ".cut")
    raw = bytearray(open(F, "rb").read())
    raw[restart.header(F)["sections"][4][1] + 5] ^= 0x10
    open(F + ".bad", "wb").write(bytes(raw))
    with pytest.raises(SfError, match="is corrupted"):
        Lammps().read_restart(F + ".bad")
    # the header refusals, through the engine
    good = open(F, "rb").read()
    for name, data, msg in (("magic", b"LAMMPS  " + good[8:], "not a sedifoam_amd restart file"),
                            ("version", good[:8] + b"\x02" + good[9:], "format version 2, this code reads up to version 1"),
                            ("order", good[:12] + good[12:16][::-1] + good[16:], "other byte order"),
                            ("header", good[:70] + bytes([good[70] ^ 4]) + good[71:], "is corrupted")):
        open(F + "." + name, "wb").write(data)
        with pytest.raises(SfError, match=msg):
            Lammps().read_restart(F + "." + name)
    # files restart.py refuses on reading are refused by the engine too: a partner that is not above the atom's own tag
    st = restart.read(F)
    st["contact_partner"] = st["contact_partner"].copy()
    st["contact_partner"][0] = st["tag"][np.nonzero(st["contact_count"])[0][0]]
    bad_bytes = restart.to_bytes(st, check=False)
    open(F + ".partner", "wb").write(bad_bytes)
    with pytest.raises(restart.RestartError, match="is corrupted"):
        restart.read(F + ".partner")
    with pytest.raises(SfError, match="is corrupted"):
        Lammps().read_restart(F + ".partner")
    # a wall whose saved ID no fix claims: dropped at the first run, the run goes on
    B = Lammps()
    B.read_restart(F)
    for line in dc.script_lines(bed, cfg):
        if not line.startswith("boundary"):
            B.command(line.replace("fix w0 ", "fix floor "))
    B.step(5)
    assert B.info().nsteps == 15


def test_second_setup_keeps_the_pair_history_like_the_oracle():
    """sf_dem_setup on an engine that has a list (the setup of a second run): the rebuild re-injects the shear history,
    as FixShearHistory does and as orc_dem_setup does -- forces and history of the setup evaluation against the oracle's."""
    bed = _closed_bed()
    cfg = dict(HOT, walls=_sheared(bed))
    lmp, orc = dc.make_hip(bed, cfg), dc.make_oracle(bed, cfg)
    lmp.setup(); orc.setup()
    lmp.step(60); orc.run(60)
    lmp.setup(); orc.setup()
    a, b = lmp.get_state(), orc.get()
    ha, hb = lmp.history(), orc.history()
    assert set(ha) == set(hb) and sum(1 for s in hb.values() if np.any(s != 0.0)) >= 100
    ks = sorted(ha)
    assert dc.rel_err(np.array([ha[k] for k in ks]), np.array([hb[k] for k in ks])) <= 1e-9
    assert dc.rel_err(a["f"], b["f"]) <= 1e-9 and dc.rel_err(a["torque"], b["torque"]) <= 1e-9
    lmp.step(40); orc.run(40)
    a, b = lmp.get_state(), orc.get()
    assert dc.rel_err(a["v"], b["v"]) <= 1e-9 and dc.rel_err(a["omega"], b["omega"]) <= 1e-9
