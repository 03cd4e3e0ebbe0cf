"""`dump ID group custom N file attr...`, `dump_modify ID sort id`, `undump ID` (csrc/sf_dump.hip): the reference's one
particle output, written from GPU-formatted bytes.  The reference's own post-processing (`grep "^i 1"` per particle of
multiParticlesCollide*/particle{Position,Velocity}.py) applied to our file gives its golden rows; a run with dumps ends in
the state of the same run without them; and the LAMMPS rules of the command (group, `*`, sort, steps) hold."""
import os
import re

import numpy as np
import pytest

from sedifoam_amd import SfError, synthetic
from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def frames(path):
    """[(step, natoms, header lines, [row bytes])] of a dump file"""
    data = open(path, "rb").read()
    out = []
    for blk in data.split(b"ITEM: TIMESTEP\n")[1:]:
        lines = blk.split(b"\n")
        step = int(lines[0])
        assert lines[1] == b"ITEM: NUMBER OF ATOMS"
        n = int(lines[2])
        assert lines[3].startswith(b"ITEM: BOX BOUNDS ")
        assert lines[7].startswith(b"ITEM: ATOMS ")
        rows = [ln + b"\n" for ln in lines[8:8 + n]]
        assert len(rows) == n and all(r.endswith(b" \n") for r in rows)
        assert lines[8 + n:] == [b""]
        out.append((step, n, lines[3:8], rows))
    return out


def row_g(*vals):
    return ("".join(("%d " % v) if isinstance(v, (int, np.integer)) else ("%g " % v) for v in vals) + "\n").encode()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's cases and post-processing

@pytest.mark.parametrize("case,ds,rhos,x0", [
    ("Rho", [1.5e-3] * 4, [4650.0, 3650.0, 2650.0, 1650.0],
     [[5e-2, 7.5e-2, 5e-2], [9e-2, 8.5e-2, 5e-2], [9.1e-2, 8.5e-2, 5e-2], [1.7e-1, 7.5e-2, 5e-2]]),
    ("Dia", [3.5e-3, 3.0e-3, 2.5e-3, 2.0e-3], [2650.0] * 4,
     [[5e-2, 7.5e-2, 5e-2], [9e-2, 8.5e-2, 5e-2], [9.2e-2, 8.5e-2, 5e-2], [1.7e-1, 6.5e-2, 5e-2]]),
])
def test_multi_particles_collide_dump_gives_the_golden_rows(case, ds, rhos, x0, tmp_path):
    """multiParticlesCollide{Rho,Dia} as tests/test_cloud_gpu.py runs them, plus the reference's dump line.  `^i 1` of
    the file: row 0 byte-identical to the golden row 0, later rows within the gates of the cloud test, and every row
    byte-identical to "%d %d %g ..." of the state sampled through lammps_get_local_info at the same step."""
    from sedifoam_amd import Lammps, enhancedCloud
    snap = str(tmp_path / "snapshot.bubblemd")
    lmp = Lammps()
    lmp.set_box([0, 0, 0], [0.2, 0.1, 0.1])
    lmp.create_atoms(x0, ds, rhos)
    lmp.commands("""
        atom_style sphere
        atom_modify map array
        boundary ff ff ff
        newton off
        communicate single vel yes
        neighbor 0.02 bin
        neigh_modify delay 0
        pair_style gran/hooke/history 4910.0 NULL 0 NULL 0.15 0
        pair_coeff * *
        timestep 1e-5
        velocity all set 0.0 0.0 0.0 units box
        fix 1 all nve/sphere
        fix 2 all gravity 9.8 vector 0 -1 0
        fix 3 all fdrag
        fix xwall all wall/gran 4910.0 NULL 0 NULL 0 0 xplane 0.00 0.20
        fix ywall all wall/gran 4910.0 NULL 0 NULL 0 0 yplane 0.00 0.10
        fix zwall all wall/gran 4910.0 NULL 0 NULL 0 0 zplane 0.00 0.10
        thermo_style one
        thermo 2000
        thermo_modify lost error
    """)
    lmp.command("dump id all custom 1000 %s id type diameter mass x y z vx vy vz" % snap)
    mesh_n = [40, 20, 1]
    cloud = enhancedCloud(lmp, [0, 0, 0], [0.2 / 40, 0.1 / 20, 0.1], mesh_n,
                          dict(dragModel="SyamlalOBrien", subCycles=2, g=(0, -9.8, 0)),
                          dict(rhob=1000.0, nub=1e-6), deltaT=1e-3)
    nc = int(np.prod(mesh_n))
    cloud.setFluid(Uf=np.zeros((nc, 3)), gradp=np.tile([0.0, -9.8 * 1000.0, 0.0], (nc, 1)))
    states = [(0, lmp.get_local_info())]
    for it in range(200):
        cloud.evolve()
        if (it + 1) % 10 == 0:
            states.append((lmp.info().nsteps, lmp.get_local_info()))
    lmp.sync()
    fr = frames(snap)
    assert [f[0] for f in fr] == [s for s, _ in states] == [1000 * k for k in range(21)]
    init = lmp.get_initial_info()
    lines = open(snap, "rb").read().split(b"\n")
    for pid in (1, 2, 3, 4):
        rows = [ln + b"\n" for ln in lines if re.match(rb"^%d 1" % pid, ln)]   # particlePosition.py: grep "^i 1"
        assert len(rows) == len(fr)
        gold_rows = open(os.path.join(GOLD, "multiParticlesCollide%s_p%d.dat" % (case, pid)), "rb").read().split(b"\n")
        assert rows[0] == gold_rows[0] + b"\n"
        gold = np.loadtxt(os.path.join(GOLD, "multiParticlesCollide%s_p%d.dat" % (case, pid)))
        ours = np.array([[float(t) for t in r.split()] for r in rows])
        for k in range(2, min(len(gold), len(ours))):
            assert ours[k, 8] == pytest.approx(gold[k, 8], rel=0.05), (pid, k)
            assert ours[k, 5] == pytest.approx(gold[k, 5], abs=1.0e-3), (pid, k)
            assert ours[k, 4] == pytest.approx(gold[k, 4], abs=3.5e-3), (pid, k)
        for k, (step, st) in enumerate(states):
            i = int(np.nonzero(st["tag"] == pid)[0][0])
            j = int(np.nonzero(init["tag"] == pid)[0][0])
            want = row_g(pid, 1, float(init["diam"][j]), 0.0, *st["x"][i], *st["v"][i])
            # (mass: the bits of row 0, which is the golden row, in every row)
            head = rows[k].split(b" ")[:4]
            assert head[:3] == want.split(b" ")[:3]
            assert head[3] == rows[0].split(b" ")[3]
            assert rows[k].split(b" ")[4:] == want.split(b" ")[4:], (pid, k)


# ---------------------------------------------------------------------------------------------------------------------
# the dump is passive

def _walled_bed(seed=5):
    bed = synthetic.fcc_bed((11, 11, 11), seed=seed, vmax=0.8)
    bed["periodic"] = (0, 0, 0)
    bed["x"][:, 0] += 0.3e-3
    bed["x"][:, 2] += 0.3e-3
    bed["boxhi"][0] += 0.6e-3
    bed["boxhi"][2] += 0.6e-3
    walls = [(1, float(bed["boxlo"][1]), float(bed["boxhi"][1])), (0, float(bed["boxlo"][0]), float(bed["boxhi"][0])),
             (2, float(bed["boxlo"][2]), float(bed["boxhi"][2]))]
    return bed, dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.04e-3, walls=walls)


def test_a_run_with_dumps_ends_in_the_state_of_the_run_without(tmp_path):
    """A 5 k-grain walled Hertz bed with rebuilds, stepped 60 + 35 + 60 + 50 sub-steps with `dump every 37` (frames
    inside queued batches and next to rebuilds) and without: the same rebuilds and contacts, and x v omega f torque and
    the contact history within the gate of the kernel-policy tests (tests/test_dem_gpu.py): a run cut at a frame ends the
    fused sub-step there (final integrate of step s, then the initial integrate of s + 1 in the next launch), which
    rounds differently from the fused pair in the last bits.  The dump kernels only read."""
    bed, cfg = _walled_bed()
    assert 4000 <= len(bed["x"]) <= 8000
    outs = []
    for with_dump in (False, True):
        lmp = dc.make_hip(bed, cfg)
        if with_dump:
            lmp.command("dump d all custom 37 %s id type x y z vx vy vz fx fy fz omegax tqz" % (tmp_path / "bed.dump"))
        lmp.setup()
        for n in (60, 35, 60, 50):
            lmp.step(n)
        lmp.sync()
        outs.append((lmp.get_state(), lmp.history(), lmp.info().nbuilds))
    assert outs[0][2] == outs[1][2] and outs[0][2] >= 3
    assert (outs[0][0]["tag"] == outs[1][0]["tag"]).all()
    dx = float(np.max(np.abs(outs[1][0]["x"] - outs[0][0]["x"])))
    errs = {k: dc.rel_err(outs[1][0][k], outs[0][0][k]) for k in ("v", "omega", "f", "torque")}
    assert set(outs[0][1]) == set(outs[1][1])
    keys = sorted(outs[0][1])
    errs["history"] = dc.rel_err(np.array([outs[1][1][p] for p in keys]), np.array([outs[0][1][p] for p in keys]))
    print("dump passive: max|dx| %.3e m, rel %s, nbuilds %d" % (dx, errs, outs[0][2]))
    assert dx <= 1e-12 * 1e-3
    for k, e in errs.items():
        assert e <= 1e-12, (k, e)
    fr = frames(str(tmp_path / "bed.dump"))
    assert [f[0] for f in fr] == [0, 37, 74, 111, 148, 185]
    assert all(f[1] == len(bed["x"]) for f in fr)


# ---------------------------------------------------------------------------------------------------------------------
# semantics

def _small(types=None):
    bed = synthetic.fcc_bed((3, 3, 3), seed=3, vmax=0.2)
    if types is not None:
        bed["type"] = types(len(bed["x"]))
    cfg = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.25e-3,
               walls=[(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))])
    return bed, cfg


def test_group_filter_and_number_of_atoms(tmp_path):
    bed, cfg = _small(types=lambda n: (1 + (np.arange(n) % 3 == 0)).astype(np.int32))
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    lmp.command("dump d two custom 10 %s id type x" % (tmp_path / "g.dump"))
    lmp.command("run 20")
    fr = frames(str(tmp_path / "g.dump"))
    want = int((bed["type"] == 2).sum())
    assert [f[0] for f in fr] == [0, 10, 20]
    assert all(f[1] == want and all(r.split(b" ")[1] == b"2" for r in f[3]) for f in fr)
    assert fr[0][2][0] == b"ITEM: BOX BOUNDS pp ff pp" and fr[0][2][4] == b"ITEM: ATOMS id type x"
    lo, hi = bed["boxlo"], bed["boxhi"]
    assert fr[0][2][1:4] == [(b"%g %g" % (lo[k], hi[k])) for k in range(3)]


def test_star_writes_one_file_per_frame(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 5 %s id x y z" % (tmp_path / "snap.*"))
    lmp.command("run 12")
    assert sorted(os.listdir(tmp_path)) == ["snap.0", "snap.10", "snap.5"]
    for s in (0, 5, 10):
        fr = frames(str(tmp_path / ("snap.%d" % s)))
        assert len(fr) == 1 and fr[0][0] == s and fr[0][1] == len(bed["x"])


def test_sort_id_with_tag_holes(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 10 %s id x y z" % (tmp_path / "s.dump"))
    lmp.command("dump_modify d sort id")
    lmp.step(10)
    gone = [3, 4, 17, 50, 51]
    lmp.delete_particle(gone)
    lmp.step(10)
    lmp.sync()
    fr = frames(str(tmp_path / "s.dump"))
    keep = [t for t in range(1, len(bed["x"]) + 1) if t not in gone]
    assert [int(r.split(b" ")[0]) for r in fr[0][3]] == list(range(1, len(bed["x"]) + 1))
    assert [int(r.split(b" ")[0]) for r in fr[-1][3]] == keep
    st = lmp.get_state()
    assert fr[-1][3] == [row_g(int(t), *x) for t, x in zip(st["tag"], st["x"])]


def test_create_particle_between_runs_changes_the_next_frame(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 10 %s id x" % (tmp_path / "c.dump"))
    lmp.step(10)
    n0 = len(bed["x"])
    lmp.create_particle([[float(bed["boxhi"][0]) * 0.5, float(bed["boxhi"][1]) * 0.9, float(bed["boxhi"][2]) * 0.5]],
                        [n0 + 1], 1.0e-3, 2500.0, 1, [0.0, 0.0, 0.0])
    lmp.step(10)
    lmp.sync()
    fr = frames(str(tmp_path / "c.dump"))
    assert [(f[0], f[1]) for f in fr] == [(0, n0), (10, n0), (20, n0 + 1)]


def test_undump_stops_the_frames(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 5 %s id" % (tmp_path / "u.dump"))
    lmp.command("run 5")
    lmp.command("undump d")
    lmp.command("run 10")
    assert [f[0] for f in frames(str(tmp_path / "u.dump"))] == [0, 5]
    with pytest.raises(SfError, match="Could not find undump ID"):
        lmp.command("undump d")


def test_step_zero_once_and_no_repeat_at_run_boundaries(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 10 %s id x" % (tmp_path / "b.dump"))
    lmp.command("run 0")
    lmp.step(5)
    lmp.step(5)
    lmp.command("run 10")
    lmp.command("run 3")
    assert [f[0] for f in frames(str(tmp_path / "b.dump"))] == [0, 10, 20]
    # a dump defined later starts at the next multiple of its N, and the file is truncated by the command
    (tmp_path / "late.dump").write_bytes(b"old")
    lmp.command("dump e all custom 4 %s id" % (tmp_path / "late.dump"))
    lmp.command("run 5")
    assert (tmp_path / "late.dump").read_bytes().startswith(b"ITEM: TIMESTEP\n24\n")
    assert [f[0] for f in frames(str(tmp_path / "late.dump"))] == [24, 28]


def test_forces_torques_and_omega_are_those_of_get_forces(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 7 %s id fx fy fz tqx tqy tqz omegax omegay omegaz radius diameter mass" %
                (tmp_path / "f.dump"))
    lmp.command("dump_modify d sort id")
    lmp.command("run 21")
    st = lmp.get_state()
    init = lmp.get_initial_info()
    o = np.argsort(init["tag"])
    d = init["diam"][o]
    m = init["rho"][o] * 4.0 / 3.0 * 3.14159265358979323846 * (0.5 * d) ** 3
    last = frames(str(tmp_path / "f.dump"))[-1]
    assert last[0] == 21
    for k, r in enumerate(last[3]):
        w = row_g(int(st["tag"][k]), *st["f"][k], *st["torque"][k], *st["omega"][k], 0.5 * d[k], d[k])
        assert r.split(b" ")[:12] == w.split(b" ")[:12], k
        assert float(r.split(b" ")[12]) == pytest.approx(m[k], rel=1e-5)


@pytest.mark.parametrize("line,msg", [
    ("dump d all atom 10 {p}", "Invalid dump style atom"),
    ("dump d all xyz 10 {p}", "Invalid dump style xyz"),
    ("dump d all local 10 {p} index", "Invalid dump style local"),
    ("dump d all custom 10 {p}.gz id x", "compressed"),
    ("dump d all custom 10 {p}.bin id x", "binary"),
    ("dump d all custom 10 {p} id xu", "Invalid attribute xu in dump custom command"),
    ("dump d all custom 10 {p} id ix", "Invalid attribute ix in dump custom command"),
    ("dump d all custom 0 {p} id", "Illegal dump command"),
    ("dump d all custom 10 {p}", "Illegal dump custom command"),
    ("dump d nogroup custom 10 {p} id", "Could not find group ID"),
])
def test_refused_dump_forms(line, msg, tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    with pytest.raises(SfError, match=re.escape(msg)):
        lmp.command(line.format(p=tmp_path / "r.dump"))


def test_refused_dump_modify_forms(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lmp.command("dump d all custom 10 %s id x" % (tmp_path / "m.dump"))
    with pytest.raises(SfError, match="Reuse of dump ID"):
        lmp.command("dump d all custom 10 %s id x" % (tmp_path / "m2.dump"))
    for line, msg in (("dump_modify d first yes", "dump_modify first is not supported"),
                      ("dump_modify d sort 3", "dump_modify sort 3 is not supported"),
                      ("dump_modify e sort id", "Could not find dump_modify ID e")):
        with pytest.raises(SfError, match=re.escape(msg)):
            lmp.command(line)


def test_xiaocase3_dump_grep_gives_the_golden_curve(tmp_path):
    """cases/auto-testing/test-cases/xiaocase3 as tests/test_cloud_gpu.py runs it, with a dump line; the reference's
    postprocessing.py filter (`grep "1 1" snapshot.bubblemd`) on our file: one row per frame, byte-identical to
    "%d %d %g ..." of the state sampled at the same step, and the velocity column on the golden curve
    (xiaocase3_lammps08.dat) within the gates of the cloud test."""
    from sedifoam_amd import Lammps, enhancedCloud
    snap = str(tmp_path / "snapshot.bubblemd")
    lmp = Lammps()
    lmp.set_box([0, 0, 0], [4e-3, 4e-3, 5e-4])
    lmp.create_atoms([[2e-3, 1.9e-3, 2.5e-4]], [8.3e-5], [2000.0])
    lmp.commands("""
        atom_style sphere
        atom_modify map array
        boundary ff ff ff
        newton off
        communicate single vel yes
        neighbor 5.0e-4 bin
        neigh_modify delay 0
        pair_style gran/hooke/history 5000.0 NULL 11200 NULL 0.1 0
        pair_coeff * *
        timestep 2e-7
        velocity all set 0.0 0.0 0.0 units box
        fix 1 all nve/sphere
        fix 2 all gravity 0.0 vector 0 -1 0
        fix 3 all fdrag
        fix xwall all wall/gran 5000.0 NULL 11200 NULL 0.1 0 xplane 0.00 0.004
        fix ywall all wall/gran 5000.0 NULL 11200 NULL 0.1 0 yplane 0.00 0.004
        fix zwall all wall/gran 5000.0 NULL 11200 NULL 0.1 0 zplane 0.00 0.0005
        thermo_style one
        thermo 2000
        thermo_modify lost error
    """)
    lmp.command("dump id all custom 2500 %s id type diameter mass x y z vx vy vz" % snap)
    cloud = enhancedCloud(lmp, [0, 0, 0], [4e-4, 4e-4, 5e-4], [10, 10, 1],
                          dict(dragModel="SyamlalOBrien", subCycles=1, g=(0, 0, 0)),
                          dict(rhob=1000.0, nub=1e-6), deltaT=2e-5)
    cloud.setFluid(Uf=np.tile([0.0, 0.05, 0.0], (100, 1)))
    states = [lmp.get_local_info()]
    for it in range(250):
        cloud.evolve()
        if lmp.info().nsteps % 2500 == 0:
            states.append(lmp.get_local_info())
    lmp.sync()
    rows = [ln + b"\n" for ln in open(snap, "rb").read().split(b"\n") if b"1 1" in ln]
    assert len(rows) == len(states) == len(frames(snap)) == 11
    m = rows[0].split(b" ")[3]
    for k, st in enumerate(states):
        want = row_g(1, 1, 8.3e-5, 0.0, *st["x"][0], *st["v"][0]).split(b" ")
        got = rows[k].split(b" ")
        assert got[:3] == want[:3] and got[3] == m and got[4:] == want[4:], k
    gold = np.loadtxt(os.path.join(GOLD, "xiaocase3_lammps08.dat"))
    t = np.arange(len(rows)) * 2500 * 2e-7
    vy = np.array([float(r.split()[8]) for r in rows])
    assert t[-1] == pytest.approx(5e-3)
    for row in gold[1:]:
        if row[0] <= t[-1] + 1e-12:
            assert np.interp(row[0], t, vy) == pytest.approx(row[2], rel=0.25 if row[0] < 1e-3 else 0.04), row
