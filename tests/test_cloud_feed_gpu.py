"""The cloud's particle add / delete schedules (cloudProperties addParticle, deleteParticle, deleteBeforeAdd; DESIGN.md
section 19), decided on the GPU, against tests/feed_model.py, against the host-driven route bit for bit, and against the
CPU oracle's coupled loop.

Bed: synthetic.fcc_bed((9, 6, 6)) -- 1 296 grains (six blocks of 256 lanes, the last one a single wave 16 lanes wide),
the two bottom layers (108 grains) of type 2 and frozen as in the reference's bed cases, over a y wall, on a 4x5x4 mesh
whose two upper cell layers (iy = 3, 4) are free of grains.  Of the FCC beds of 1 250-1 650 grains this one keeps the
centre-counted solid fraction of every cell lowest (0.81; tests/test_cloud_gpu.py::_coupled_case asks for < 0.85: the drag
closures diverge as a cell fills up).  Grains are added in layer iy = 4 and fall at 8 m/s."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ob
from sedifoam_amd import SfError, _lib
from tests import dem_cases as dc
from tests import feed_model as fm
import tests.test_inject_remove_gpu as IR

pytestmark = pytest.mark.gpu

DELTA_T = 50e-6
MESH_N = (4, 5, 4)
D_NEW, RHO_NEW, V_NEW = 0.6e-3, 2000.0, (0.0, -8.0, 0.0)
ACTIVE_BIT = 4                                   # group bottom type 2 -> bit 2, group active subtract all bottom -> bit 4
TRANS = dict(rhob=1000.0, nub=1.0e-6)
FORCES = dict(particleAddedMass=True, particleHistoryForce=True)


@pytest.fixture(scope="module")
def bed():
    from sedifoam_amd import synthetic
    b = synthetic.fcc_bed((9, 6, 6), seed=21, vmax=0.05)
    assert b["n"] == 1296 and b["n"] > 256 and b["n"] % 64 != 0
    b["type"] = np.where(b["x"][:, 1] < 0.8e-3, 2, 1).astype(np.int32)
    assert (b["type"] == 2).sum() == 108
    origin, dxm, n = _mesh(b)
    c = np.floor((b["x"] - origin) / dxm).astype(int)
    count = np.bincount(c[:, 0] + n[0] * (c[:, 1] + n[1] * c[:, 2]), minlength=int(np.prod(n)))
    assert (count * np.pi / 6.0 * 1.0e-9 / np.prod(dxm)).max() < 0.85
    for k in ("x", "v", "type"):
        b[k].setflags(write=False)
    return b


def _cfg(bed):
    return dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.25e-3, frozen_types=[2],
                walls=[(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))])


def _mesh(bed):
    n = np.array(MESH_N, np.int32)
    return bed["boxlo"].copy(), (bed["boxhi"] - bed["boxlo"]) / n, n


def _fields(ncells):
    rng = np.random.default_rng(3)
    Uf = np.tile([0.0, 0.05, 0.0], (ncells, 1)) + 0.01 * np.sin(rng.uniform(0, 6, size=(ncells, 3)))
    DDtUf = rng.normal(scale=0.5, size=(ncells, 3))
    gradp = np.tile([0.0, -9810.0, 0.0], (ncells, 1)) + rng.normal(scale=50.0, size=(ncells, 3))
    curlU = rng.normal(scale=5.0, size=(ncells, 3))
    return dict(Uf=Uf, DDtUf=DDtUf, gradp=gradp, curlU=curlU)


def _cloud(lmp, bed, keys, sub_cycles=1, flags=None, **mesh_kw):
    from sedifoam_amd import enhancedCloud
    origin, dxm, n = _mesh(bed)
    cd = dict(dragModel="ErgunWenYu", subCycles=sub_cycles, g=(0.0, -9.81, 0.0), maxPossibleAlpha=0.65, **(flags or {}))
    cd.update(keys)
    cloud = enhancedCloud(lmp, origin, dxm, n, cd, TRANS, DELTA_T, **mesh_kw)
    cloud.setFluid(**_fields(int(np.prod(n))))
    return cloud


def _boxes(bed):
    """addParticleBox: the cell layer iy = 4; clearInitialBox: a corner of the bed's two top layers; deleteParticleBox: a
    slab that begins 0.2 mm under the add cells' centres -- under every created position (randomPerturb / 2 = 0.15 mm), so
    that only falling grains reach it, 0.4 mm further down after one CFD step; nowhere: outside the domain"""
    lo, hi = bed["boxlo"], bed["boxhi"]
    dy = (hi[1] - lo[1]) / MESH_N[1]
    cy = lo[1] + 4.5 * dy
    ytop = float(bed["x"][:, 1].max())
    return dict(add=(lo[0], hi[0], lo[1] + 4 * dy, hi[1], lo[2], hi[2], 0.0, 0.0, 0.0),
                clear=(lo[0], lo[0] + 2.5e-3, ytop - 1.0e-3, ytop + 1.0e-3, lo[2], lo[2] + 2.5e-3, 0.0, 0.0, 0.0),
                delete=(lo[0], hi[0], cy - 1.8e-3, cy - 0.2e-3, lo[2], hi[2], 0.0, 0.0, 0.0),
                nowhere=(-2.0, -1.0, -2.0, -1.0, -2.0, -1.0, 0.0, 0.0, 0.0))


def _keys(bed, **over):
    b = _boxes(bed)
    k = dict(addParticle=1, deleteParticle=1, deleteBeforeAdd=1, addParticleTimeStep=2 * DELTA_T, randomPerturb=0.3e-3,
             addParticleBox=b["add"], clearInitialBox=b["clear"], deleteParticleBox=b["delete"],
             addParticleInfo=(D_NEW, RHO_NEW, 1), addParticleVelocity=V_NEW, reduceNumberFactor=2)
    k.update(over)
    return k


def _types(lmp):
    """(tag, type) of the owned atoms sorted by tag"""
    ii = lmp.get_initial_info()
    o = np.argsort(ii["tag"], kind="stable")
    return ii["tag"][o], ii["type"][o], ii["diam"][o]


def _centres(bed, **kw):
    origin, dxm, n = _mesh(bed)
    return fm.cell_centres(origin, dxm, n, **kw)


# ---- 1: the add cells -------------------------------------------------------------------------------------------------------

def _graded(lo, hi, n, expansion):
    r = expansion ** (1.0 / (n - 1))
    w = r ** np.arange(n)
    f = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(w) / w.sum()])
    f[-1] = hi
    return f


@pytest.mark.parametrize("mesh", ["uniform", "graded", "labels"])
def test_add_cells_equal_the_model(bed, mesh):
    origin, dxm, n = _mesh(bed)
    lo, hi = bed["boxlo"], bed["boxhi"]
    kw, mkw = {}, {}
    if mesh == "graded":
        faces = (None, _graded(lo[1], hi[1], n[1], 0.4), _graded(lo[2], hi[2], n[2], 2.5))
        kw, mkw = dict(mesh_faces=faces), dict(faces=faces)
    elif mesh == "labels":
        lab = np.random.default_rng(5).permutation(int(np.prod(n))).astype(np.int32)
        kw, mkw = dict(mesh_labels=lab), dict(labels=lab)
    centres = fm.cell_centres(origin, dxm, n, **mkw)
    cx = 0.5 * (lo[0] + hi[0])
    cy = float(centres[:, 1].max())                                   # the centre of the top cell layer
    cyl = (cx, cx, cy, cy, lo[2], hi[2], 0.5e-3, 2.0e-3, 0.0)         # hollow cylinder along z: the two middle columns
    box = (lo[0], hi[0], cy - 1.0e-3, hi[1], lo[2], hi[2], 0.0, 0.0, 0.0)
    lmp = dc.make_hip(bed, _cfg(bed))
    seen = set()
    for option, region in ((1, box), (2, cyl)):
        for factor in (1, 2, 3):
            keys = _keys(bed, addParticle=option, addParticleBox=region, reduceNumberFactor=factor, deleteParticle=0,
                         deleteBeforeAdd=0, eccentricity=(0.1e-3, 0.0, 0.0))
            cloud = _cloud(lmp, bed, keys, **kw)
            got = cloud.addParticleCells()
            want = fm.add_cells(option, region, keys["eccentricity"], centres, factor)
            assert np.array_equal(got, want), (option, factor)
            assert cloud.feedInfo()["nAddCells"] == len(want) > 0
            seen.add((option, len(want)))
            cloud.close()
    assert {(1, 16), (2, 8)} <= seen                                  # all of the layer; the two middle columns of it


# ---- 2: one add event -------------------------------------------------------------------------------------------------------

def test_one_add_event(bed):
    """The timer starts at 0: the first sub-cycle adds.  clearInitialBox holds the grain with the highest tag alone, so its
    tag is handed out again; that grain had been wrapped around the periodic box once, the new holder of its tag has not"""
    b = dict(bed)
    x = bed["x"].copy()
    last = b["n"] - 1
    lx = float(bed["boxhi"][0] - bed["boxlo"][0])
    x[last, 0] += lx                                                  # one box length outside: the first rebuild wraps it
    b["x"] = x
    lmp = dc.make_hip(b, _cfg(bed))
    lmp.command("compute d all displace/atom")
    lmp.command("compute m all property/atom mass")
    p = bed["x"][last]
    w = 0.3e-3
    clear = (p[0] - w, p[0] + w, p[1] - w, p[1] + w, p[2] - w, p[2] + w, 0.0, 0.0, 0.0)
    keys = _keys(bed, addParticleTimeStep=0.0, clearInitialBox=clear, deleteParticleBox=_boxes(bed)["nowhere"])
    cloud = _cloud(lmp, bed, keys)
    tag0 = lmp.get_local_info()["tag"]
    assert lmp.images()[tag0 == b["n"]].tolist() == [[1, 0, 0]]
    before = lmp.get_state()
    tags_t, types_t, _ = _types(lmp)
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    assert model.time_to_add == 0.0
    want = model.sub_cycle(before["x"], tags_t, types_t)
    assert want["clear"].tolist() == [b["n"]] and want["delete"].size == 0
    assert want["add"]["tags"].tolist() == list(range(b["n"], b["n"] + 4))      # the cleared grain's tag is handed out again
    nb = lmp.info().nbuilds
    cloud._phase(7)                                                   # the schedules of one sub-cycle, nothing else
    assert lmp.info().nbuilds == nb + 2                               # one rebuild behind the clearing, one behind the add
    info = cloud.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (4, 0, 1)
    assert (info["lastAdd"], info["lastDelete"], info["lastDeleteBeforeAdd"]) == (4, 0, 1)
    assert info["timeToAddParticle"] == 0.0 and lmp.get_local_n() == b["n"] + 3
    after = lmp.get_state()
    new = np.isin(after["tag"], want["add"]["tags"])
    assert new.sum() == 4 and np.array_equal(after["tag"][new], want["add"]["tags"])
    assert np.array_equal(after["x"][new], want["add"]["pos"])        # the same doubles
    assert np.all(np.abs(after["x"][new] - _centres(bed)[model.cells]) <= 0.15e-3)
    assert np.all(after["v"][new] == np.asarray(V_NEW))
    for k in ("omega", "f", "torque"):
        assert np.all(after[k][new] == 0.0)
    tags_a, types_a, diam_a = _types(lmp)
    assert np.array_equal(tags_a, after["tag"])
    assert np.all(types_a[new] == 1) and np.all(diam_a[new] == D_NEW)
    assert np.all(lmp.compute_atom("m")[new] == fm.created_mass(D_NEW, RHO_NEW))
    order = lmp.get_local_info()["tag"]
    is_new = np.isin(order, want["add"]["tags"])
    assert np.all(lmp.group_mask("active")[is_new]) and np.all(lmp.group_mask("all")[is_new])
    assert not np.any(lmp.group_mask("bottom")[is_new])
    assert np.all(lmp.images()[is_new] == 0)                          # the reused tag among them
    assert np.all(lmp.compute_atom("d")[new] == 0.0)                  # displacement of a new grain at its creation
    # everybody else is carried bit for bit
    old = ~np.isin(before["tag"], want["clear"])
    for k in IR.KEYS:
        assert np.array_equal(after[k][~new], before[k][old]), k


# ---- 3: removal ---------------------------------------------------------------------------------------------------------------

def test_removal_by_box_and_exact_carry_over(bed):
    cfg = _cfg(bed)
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    st = lmp.get_state()
    tags_t, types_t, _ = _types(lmp)
    lo, hi = bed["boxlo"], bed["boxhi"]
    # A box over the whole height, a third of the bed wide in x and z, with faces THROUGH grains: x1 and z2 are
    # coordinates of type-1 grains (product 0 < 1e-150: inside), y1 = the wall (the type-2 layers lie inside)
    one = np.nonzero(types_t == 1)[0]
    # (ga: x nearest 3 mm among the grains with z in 4.5 +- 1 mm; gb: z nearest 6 mm among those with x in 4.5 +- 1 mm: the
    # lattice planes lie 0.69 mm apart, so x1 <= 3.35 mm, x1 + 3 mm >= 5.65 mm and each lies between the other's faces)
    ga = one[np.argmin(np.abs(st["x"][one, 0] - 3.0e-3) + 1.0e3 * (np.abs(st["x"][one, 2] - 4.5e-3) > 1.0e-3))]
    gb = one[np.argmin(np.abs(st["x"][one, 2] - 6.0e-3) + 1.0e3 * (np.abs(st["x"][one, 0] - 4.5e-3) > 1.0e-3))]
    x1, z2 = float(st["x"][ga, 0]), float(st["x"][gb, 2])
    box = (x1, x1 + 3.0e-3, lo[1], hi[1], z2 - 3.0e-3, z2, 0.0, 0.0, 0.0)
    keys = _keys(bed, addParticle=1, addParticleTimeStep=1.0e9, deleteBeforeAdd=0, deleteParticleBox=box)
    cloud = _cloud(lmp, bed, keys)
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    want = model.sub_cycle(st["x"], tags_t, types_t)
    dead = want["delete"]
    inside = fm.in_region(1, box, (0, 0, 0), st["x"])
    assert int(tags_t[ga]) in dead and int(tags_t[gb]) in dead        # the grains on the faces go
    assert 40 <= len(dead) < 400 and (inside & (types_t == 2)).sum() >= 4
    # (a grain one ulp beyond a face would stay: the model says so in tests/test_feed_model.py; here the faces' grains)
    before = IR._snap(lmp, cfg)
    nb = lmp.info().nbuilds
    cloud._phase(7)
    assert lmp.info().nbuilds == nb + 1
    after = IR._snap(lmp, cfg)
    assert sorted(after["tag"].tolist()) == sorted(set(before["tag"].tolist()) - set(dead.tolist()))
    t_after, ty_after, _ = _types(lmp)
    assert (ty_after == 2).sum() == 108                               # type-2 grains inside the box stay
    live, dropped = IR._assert_carried(before, after, dead.tolist(), "feed removal")
    assert live >= 100 and dropped >= len(dead)
    info = cloud.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (0, len(dead), 0)
    assert info["lastDelete"] == len(dead)
    nb = lmp.info().nbuilds
    cloud._phase(7)                                                   # nobody is left inside: the mark launch and nothing else
    assert lmp.info().nbuilds == nb and cloud.feedInfo()["lastDelete"] == 0
    assert cloud.feedInfo()["totalDelete"] == len(dead)


def test_add_due_without_add_cells_still_removes(bed):
    """The drain-only configuration: deleteParticle needs addParticle > 0 (the region kind), and an addParticleBox that
    holds no cell centre gives no add cell.  With the timer due, the sub-cycle is an add of nothing followed by the delete:
    the grains inside deleteParticleBox go, one rebuild, everybody else carried exactly, and the timer restarts."""
    cfg = _cfg(bed)
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    st = lmp.get_state()
    tags_t, types_t, _ = _types(lmp)
    lo, hi = bed["boxlo"], bed["boxhi"]
    ytop = float(bed["x"][:, 1].max())
    nowhere = _boxes(bed)["nowhere"]
    dele = (lo[0], lo[0] + 2.6e-3, ytop - 0.35e-3, ytop + 1.0e-3, hi[2] - 2.6e-3, hi[2], 0.0, 0.0, 0.0)
    keys = _keys(bed, addParticleTimeStep=0.0, addParticleBox=nowhere, clearInitialBox=nowhere, deleteParticleBox=dele)
    cloud = _cloud(lmp, bed, keys)
    assert cloud.feedInfo()["nAddCells"] == 0 and cloud.addParticleCells().size == 0
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    assert model.time_to_add == 0.0 and len(model.cells) == 0
    want = model.sub_cycle(st["x"], tags_t, types_t)
    dead = want["delete"]
    assert want["add"] is None and want["clear"].size == 0 and len(dead) >= 4
    before = IR._snap(lmp, cfg)
    nb = lmp.info().nbuilds
    cloud._phase(7)
    assert lmp.info().nbuilds == nb + 1
    after = IR._snap(lmp, cfg)
    assert sorted(after["tag"].tolist()) == sorted(set(before["tag"].tolist()) - set(dead.tolist()))
    IR._assert_carried(before, after, dead.tolist(), "drain-only removal")
    info = cloud.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (0, len(dead), 0)
    assert (info["lastAdd"], info["lastDelete"], info["lastDeleteBeforeAdd"]) == (0, len(dead), 0)
    assert info["timeToAddParticle"] == 0.0                           # due again at once
    nb = lmp.info().nbuilds
    cloud._phase(7)                                                   # due, no cell, nobody inside: nothing is rebuilt
    assert lmp.info().nbuilds == nb and cloud.feedInfo()["totalDelete"] == len(dead)
    cloud.evolve()                                                    # and the engine goes on
    assert lmp.get_local_n() == bed["n"] - len(dead)


# ---- 4: the same bits as the host-driven route ------------------------------------------------------------------------------

def _host_feed(lmp, model):
    """what a host shim does in front of evolve(): the lists of the model from the engine's own state, through
    lammps_delete_particle / lammps_create_particle.  Returns (cleared, added, deleted)"""
    st = lmp.get_state()
    tags_t, types_t, _ = _types(lmp)
    w = model.sub_cycle(st["x"], tags_t, types_t)
    if len(w["clear"]):
        lmp.delete_particle(w["clear"])
    if w["add"] is not None:
        k = model.k
        lmp.create_particle(w["add"]["pos"], w["add"]["tags"], k["addParticleInfo"][0], k["addParticleInfo"][1],
                            int(k["addParticleInfo"][2]), k["addParticleVelocity"])
    if len(w["delete"]):
        lmp.delete_particle(w["delete"])
    return len(w["clear"]), 0 if w["add"] is None else len(w["add"]["tags"]), len(w["delete"])


def test_fed_run_equals_host_driven_run_bit_for_bit(bed):
    cfg = _cfg(bed)
    keys = _keys(bed)
    la, lb = dc.make_hip(bed, cfg), dc.make_hip(bed, cfg)
    ca, cb = _cloud(la, bed, keys, flags=FORCES), _cloud(lb, bed, {}, flags=FORCES)
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    events = []
    for it in range(8):
        events.append(_host_feed(lb, model))
        ca.evolve(); cb.evolve()
        info = ca.feedInfo()
        assert (info["lastDeleteBeforeAdd"], info["lastAdd"], info["lastDelete"]) == events[-1], it
        a, b = la.get_state(), lb.get_state()
        for k in ("tag",) + IR.KEYS:
            assert np.array_equal(a[k], b[k]), (it, k)
        ha, hb = la.history(), lb.history()
        assert set(ha) == set(hb) and all(np.array_equal(ha[k], hb[k]) for k in ha), it
        assert np.array_equal(la.wall_shear(0), lb.wall_shear(0)), it
        pa, pb = ca.particles(), cb.particles()
        for k in ("tag", "cell", "pDrag", "Jd"):
            assert np.array_equal(pa[k], pb[k]), (it, k)
        assert np.array_equal(ca.gamma(), cb.gamma()) and np.array_equal(ca.Ue(), cb.Ue()), it
    print("events (cleared, added, deleted) per CFD step:", events)
    assert sum(1 for e in events if e[1]) >= 2 and sum(1 for e in events if e[0]) >= 1
    assert sum(1 for e in events if e[2]) >= 2
    info = ca.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (
        model.totalAdd, model.totalDelete, model.totalDeleteBeforeAdd)
    assert info["timeToAddParticle"] == model.time_to_add
    assert sum(1 for v in ha.values() if np.any(v != 0.0)) >= 100     # the comparison had live history to carry


# ---- 5: held to the oracle -------------------------------------------------------------------------------------------------

def _reindex(old_tags, new_tags, arr, init):
    """rows of `arr` (by old_tags, sorted) carried to new_tags by tag; a new tag takes `init` (a row or a function of tag)"""
    out = np.empty((len(new_tags),) + arr.shape[1:], arr.dtype)
    pos = {int(t): i for i, t in enumerate(old_tags)}
    for i, t in enumerate(new_tags):
        out[i] = arr[pos[int(t)]] if int(t) in pos else init
    return out


def test_fed_coupled_run_against_the_oracle(bed):
    """The coupled loop of tests/test_cloud_gpu.py::_coupled_case with the schedules in it: the oracle side creates and
    deletes through OracleDem, the per-particle rows the loop owns (diameter, type, UOld, sumFb, n0) follow their tags.
    Gates as there: 1e-12, cell owners exact, positions 1e-12 m, velocities 1e-9."""
    cfg = _cfg(bed)
    keys = _keys(bed)
    sub_cycles = 2
    origin, dxm, mesh_n = _mesh(bed)
    ncells = int(np.prod(mesh_n))
    F = _fields(ncells)
    Uf, DDtUf, gradp, curlU = F["Uf"], F["DDtUf"], F["gradp"], F["curlU"]
    lmp = dc.make_hip(bed, cfg)
    cloud = _cloud(lmp, bed, keys, sub_cycles=sub_cycles, flags=FORCES)
    L = ob.lib()
    orc = dc.make_oracle(bed, cfg)
    dtadj = C.c_double(); steps = C.c_int(); sc = C.c_int(); ss = C.c_int()
    assert L.orc_adjust_timestep(DELTA_T, cfg["dt"], sub_cycles, C.byref(dtadj), C.byref(steps), C.byref(sc), C.byref(ss)) == 0
    orc.timestep(dtadj.value)
    orc.setup()
    V = np.full(ncells, float(np.prod(dxm)))
    fl = ob.CloudFlags()
    fl.particleDrag = 1; fl.particlePressureGrad = 1; fl.particleBuoyancy = 0; fl.particleAddedMass = 1
    fl.particleLift = 0; fl.lubricationForce = 0
    fl.gravity = (C.c_double * 3)(0.0, -9.81, 0.0); fl.rhob = 1000.0; fl.nub = 1e-6; fl.deltaT = DELTA_T
    gamma = np.zeros(ncells); Ue = np.zeros((ncells, 3))
    st = orc.get()
    d = bed["diameter"].copy(); typ = bed["type"].copy()
    sumFb = np.zeros((orc.nlocal, 3)); n0 = np.zeros(orc.nlocal)
    UOld = st["v"].copy()

    def scatter(st, d):
        n = len(d)
        cell = np.zeros(n, np.int32)
        L.orc_cell_owner(n, ob.P(st["x"]), ob.P(origin), ob.P(dxm), ob.P(mesh_n), ob.P(cell))
        L.orc_particle_to_eulerian_smooth(n, ob.P(cell), ob.P(d), ob.P(st["v"]), ncells, ob.P(V), None, ob.P(gamma), ob.P(Ue))
    scatter(st, d)
    assert dc.rel_err(cloud.gamma(), gamma) <= 1e-12
    UfS = np.zeros((ncells, 3))
    L.orc_uf_smoothed(ncells, ob.P(Uf), ob.P(gamma), None, ob.P(UfS))
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    events = []
    for it in range(6):
        cloud.evolve()
        UfS_old = UfS.copy()
        L.orc_uf_smoothed(ncells, ob.P(Uf), ob.P(gamma), None, ob.P(UfS))
        for k in range(sc.value):
            w = model.sub_cycle(st["x"], st["tag"], typ)
            if len(w["clear"]):
                assert orc.delete_particle(w["clear"]) == len(w["clear"])
            if w["add"] is not None:
                orc.create_particle(w["add"]["pos"], w["add"]["tags"], D_NEW, RHO_NEW, 1, V_NEW, active_bit=ACTIVE_BIT)
            if len(w["delete"]):
                assert orc.delete_particle(w["delete"]) == len(w["delete"])
            events.append((len(w["clear"]), 0 if w["add"] is None else len(w["add"]["tags"]), len(w["delete"])))
            if any(events[-1]):
                old_tags, st = st["tag"], orc.get()
                new_v = {int(t): st["v"][i] for i, t in enumerate(st["tag"])}
                d = _reindex(old_tags, st["tag"], d, D_NEW)
                typ = _reindex(old_tags, st["tag"], typ, 1)
                sumFb = _reindex(old_tags, st["tag"], sumFb, 0.0)      # the registered initial values: 0, 0 ...
                n0 = _reindex(old_tags, st["tag"], n0, 0.0)
                uo = np.empty((len(st["tag"]), 3))                     # ... and NaN = "UOld is U" (softParticle.C:74)
                pos = {int(t): i for i, t in enumerate(old_tags)}
                for i, t in enumerate(st["tag"]):
                    uo[i] = UOld[pos[int(t)]] if int(t) in pos else new_v[int(t)]
                UOld = uo
            n = orc.nlocal
            assert n == len(d) == len(UOld)
            cell = np.zeros(n, np.int32)
            Uri = np.zeros((n, 3)); mag = np.zeros(n); Jd = np.zeros(n); pDrag = np.zeros((n, 3)); pDuDt = np.zeros((n, 3))
            L.orc_cell_owner(n, ob.P(st["x"]), ob.P(origin), ob.P(dxm), ob.P(mesh_n), ob.P(cell))
            L.orc_drag_on_particles_hist(C.byref(fl), 0, n, ob.P(cell), ob.P(st["x"]), ob.P(d), ob.P(st["v"]), ob.P(UOld),
                                         ob.P(gamma), ob.P(UfS), ob.P(gradp), ob.P(DDtUf), ob.P(curlU), it + 1,
                                         ob.P(UfS_old), ob.P(sumFb), ob.P(n0), ob.P(Uri), ob.P(mag), ob.P(Jd), ob.P(pDrag),
                                         ob.P(pDuDt))
            cell_before, pDrag_before, Jd_before = cell.copy(), pDrag.copy(), Jd.copy()
            orc.put_fdrag(pDrag, st["tag"])
            orc.run(ss.value)
            UOld = st["v"]
            st = orc.get()
            if k == 0:
                scatter(st, d)
        P = cloud.particles()
        assert np.array_equal(P["tag"], st["tag"]), it
        assert np.array_equal(P["cell"], cell_before), it
        ej, ep = dc.rel_err(P["Jd"], Jd_before), dc.rel_err(P["pDrag"], pDrag_before)
        a = lmp.get_state()
        ex, ev = float(np.max(np.abs(a["x"] - st["x"]))), dc.rel_err(a["v"], st["v"])
        eg, eu = dc.rel_err(cloud.gamma(), gamma), dc.rel_err(cloud.Ue(), Ue)
        print("step %d n=%d: Jd %.2e pDrag %.2e x %.2e v %.2e gamma %.2e Ue %.2e" % (it, len(d), ej, ep, ex, ev, eg, eu))
        assert ej <= 1e-12 and ep <= 1e-12 and ex <= 1e-12 and ev <= 1e-9 and eg <= 1e-12 and eu <= 1e-11
    info = cloud.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (
        model.totalAdd, model.totalDelete, model.totalDeleteBeforeAdd)
    print("events per sub-cycle:", events)
    assert model.totalAdd >= 8 and model.totalDeleteBeforeAdd >= 1 and model.totalDelete >= 1
    assert len(st["tag"]) != bed["n"]


# ---- 6: the schedule with two sub-cycles ------------------------------------------------------------------------------------

def test_schedule_with_two_sub_cycles(bed):
    """The timer falls by deltaT per SUB-CYCLE, as in the reference: with addParticleTimeStep = 2 deltaT the adds come on
    sub-cycles 3, 6, 9 (counted from 1), i.e. in the first sub-cycle of evolve 2, the second of evolve 3, the first of
    evolve 5.  deleteParticleBox holds a fixed set of bed grains (its faces lie in the gaps between lattice planes, the grains
    move by microns): they all go on sub-cycle 1; clearInitialBox likewise at the first add."""
    cfg = _cfg(bed)
    lo, hi = bed["boxlo"], bed["boxhi"]
    ytop = float(bed["x"][:, 1].max())
    dele = (lo[0], lo[0] + 2.6e-3, ytop - 0.35e-3, ytop + 1.0e-3, hi[2] - 2.6e-3, hi[2], 0.0, 0.0, 0.0)
    keys = _keys(bed, deleteParticleBox=dele)
    lmp = dc.make_hip(bed, cfg)
    cloud = _cloud(lmp, bed, keys, sub_cycles=2)
    model = fm.Schedule(keys, _centres(bed), DELTA_T)
    x = bed["x"].copy(); tag = np.arange(1, bed["n"] + 1); typ = bed["type"].copy()
    appeared, want_appeared = [], []
    for it in range(5):
        per_cycle = []
        for k in range(2):
            w = model.sub_cycle(x, tag, typ)
            gone = np.isin(tag, np.concatenate([w["clear"], w["delete"]]))
            x, tag, typ = x[~gone], tag[~gone], typ[~gone]
            if w["add"] is not None:
                x = np.vstack([x, w["add"]["pos"]]); tag = np.append(tag, w["add"]["tags"])
                typ = np.append(typ, np.ones(len(w["add"]["tags"]), typ.dtype))
                want_appeared.append(2 * it + k + 1)
            per_cycle.append((len(w["clear"]), 0 if w["add"] is None else 4, len(w["delete"])))
        t0 = cloud.feedInfo()["totalAdd"]
        cloud.evolve()
        info = cloud.feedInfo()
        assert (info["lastDeleteBeforeAdd"], info["lastAdd"], info["lastDelete"]) == per_cycle[1], it
        if info["totalAdd"] > t0:
            appeared.append(2 * it + (2 if info["lastAdd"] else 1))
        assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (
            model.totalAdd, model.totalDelete, model.totalDeleteBeforeAdd), it
        assert info["timeToAddParticle"] == model.time_to_add
        assert sorted(lmp.get_local_info()["tag"].tolist()) == sorted(tag.tolist()), it
    assert appeared == want_appeared == [3, 6, 9]
    assert model.totalDelete >= 4 and model.totalDeleteBeforeAdd >= 4 and model.totalAdd == 12


# ---- 7: passive ---------------------------------------------------------------------------------------------------------------

def test_idle_schedules_change_no_bit(bed):
    cfg = _cfg(bed)
    nowhere = _boxes(bed)["nowhere"]
    keys = _keys(bed, addParticleTimeStep=1.0e9, deleteParticleBox=nowhere, clearInitialBox=nowhere)
    la, lb = dc.make_hip(bed, cfg), dc.make_hip(bed, cfg)
    ca, cb = _cloud(la, bed, keys, sub_cycles=2, flags=FORCES), _cloud(lb, bed, {}, sub_cycles=2, flags=FORCES)
    for it in range(3):
        ca.evolve(); cb.evolve()
    a, b = la.get_state(), lb.get_state()
    for k in ("tag",) + IR.KEYS:
        assert np.array_equal(a[k], b[k]), k
    ha, hb = la.history(), lb.history()
    assert set(ha) == set(hb) and all(np.array_equal(ha[k], hb[k]) for k in ha)
    assert np.array_equal(ca.gamma(), cb.gamma()) and np.array_equal(ca.Ue(), cb.Ue())
    assert np.array_equal(ca.particles()["pDrag"], cb.particles()["pDrag"])
    assert la.info().nbuilds == lb.info().nbuilds
    info = ca.feedInfo()
    assert (info["totalAdd"], info["totalDelete"], info["totalDeleteBeforeAdd"]) == (0, 0, 0)
    timer = 1.0e9
    for _ in range(6):
        timer -= DELTA_T                                              # once per sub-cycle, rounded each time
    assert info["timeToAddParticle"] == timer and info["nAddCells"] == 4
    none = cb.feedInfo()                                              # a cloud without the keys: nothing configured
    assert none["nAddCells"] == 0 and cb.addParticleCells().size == 0 and none["timeToAddParticle"] > 1e149


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------

def _set_feed(cloud, keys):
    from sedifoam_amd import enhancedCloud
    f = enhancedCloud._feed_keys(keys)
    _lib.check(cloud.L.sf_cloud_set_feed(cloud.ptr, C.byref(f)))


def test_refusals(bed):
    cfg = _cfg(bed)
    lmp = dc.make_hip(bed, cfg)
    b = _boxes(bed)
    top = b["add"]
    cases = [
        (dict(addParticle=3), "addParticle 3 is not 0, 1 or 2"),
        (dict(addParticle=-1), "addParticle -1 is not 0, 1 or 2"),
        (dict(addParticleOption=2), "addParticle 1 and addParticleOption 2 differ"),
        (dict(reduceNumberFactor=0), "reduceNumberFactor 0 < 1"),
        # type 1, deleteParticle > 0 and the add layer inside deleteParticleBox
        (dict(deleteParticleBox=(top[0], top[1], top[2] - 1.0e-3, top[3], top[4], top[5], 0, 0, 0)),
         "created and deleted in the same step"),
        # the top layer's centres lie 1.4 mm under the lid: +- 2 mm leaves the box along y, which is not periodic
        (dict(randomPerturb=4.0e-3), "leaves the box .* along axis 1, which is not periodic"),
    ]
    for over, msg in cases:
        with pytest.raises(SfError, match=msg):
            _cloud(lmp, bed, _keys(bed, **over))
    # the same add layer with type 2, or without deleteParticle: no grain is made and deleted at once
    inside = dict(deleteParticleBox=(top[0], top[1], top[2] - 1.0e-3, top[3], top[4], top[5], 0, 0, 0))
    _cloud(lmp, bed, _keys(bed, addParticleInfo=(D_NEW, RHO_NEW, 2), **inside)).close()
    _cloud(lmp, bed, _keys(bed, deleteParticle=0, **inside)).close()
    # x and z are periodic: a perturbation that leaves the box there is wrapped by the rebuild, not refused
    lo, hi = bed["boxlo"], bed["boxhi"]
    dy = (hi[1] - lo[1]) / MESH_N[1]
    mid = (lo[0], hi[0], lo[1] + 3 * dy, lo[1] + 4 * dy, lo[2], hi[2], 0, 0, 0)
    _cloud(lmp, bed, _keys(bed, addParticleBox=mid, randomPerturb=3.4e-3, deleteParticle=0)).close()
    with pytest.raises(SfError, match="required|undefined"):
        k = _keys(bed); del k["addParticleInfo"]
        _cloud(lmp, bed, k)
    # a driver
    with pytest.raises(SfError, match="one rank"):
        from sedifoam_amd import enhancedCloud
        origin, dxm, n = _mesh(bed)
        enhancedCloud(lmp, origin, dxm, n, dict(_keys(bed), dragModel="ErgunWenYu"), TRANS, DELTA_T, driver=object())
    # a slab mesh
    L = _lib.lib()
    origin, dxm, n = _mesh(bed)
    m = _lib.CloudMesh()
    m.origin = (C.c_double * 3)(*origin); m.dx = (C.c_double * 3)(*dxm); m.n = (C.c_int * 3)(*[int(q) for q in n])
    m.slab_nx_global = 8
    pr = _lib.CloudProps()
    pr.subCycles = 1; pr.particleDrag = 1; pr.rhob = 1000.0; pr.nub = 1e-6; pr.smoothDirection = (C.c_double * 3)(1, 1, 1)
    h = C.c_void_p()
    _lib.check(L.sf_cloud_create(lmp.ptr, C.byref(m), C.byref(pr), DELTA_T, C.byref(h)))
    from sedifoam_amd import enhancedCloud
    f = enhancedCloud._feed_keys(_keys(bed))
    assert L.sf_cloud_set_feed(h, C.byref(f)) < 0 and "one rank" in L.sf_last_error().decode()
    _lib.check(L.sf_cloud_destroy(h))
    # after the first evolve
    cloud = _cloud(lmp, bed, {})
    cloud.evolve()
    with pytest.raises(SfError, match="after the first evolve"):
        _set_feed(cloud, _keys(bed))
    cloud.close()
    # the C entry's own check (enhancedCloud refuses in Python before it gets there): a cloud made with the override alone.
    # A C struct cannot leave a field out, so there 0 is "not given": addParticle 0 beside addParticleOption 2 passes
    cloud = _cloud(lmp, bed, dict(addParticleOption=2))
    with pytest.raises(SfError, match=r"sf_cloud_set_feed: addParticle 1 and addParticleOption 2 differ"):
        _set_feed(cloud, _keys(bed))
    _set_feed(cloud, dict(addParticle=0, deleteParticle=1))
    cloud.close()
    # a caller that steps through the phases cannot leave the schedules out unnoticed
    cloud = _cloud(lmp, bed, _keys(bed, addParticleTimeStep=1.0e9))
    cloud._phase(0)
    with pytest.raises(SfError, match="phase 7 runs them"):
        cloud._phase(1)
    cloud._phase(7)
    cloud._phase(1)
    cloud.close()
    # fix rigid/nve: the first two grains (neighbours) as one body in the place of the frozen layer
    from sedifoam_amd import Lammps
    two = np.ones(bed["n"], np.int32)
    two[:2] = 2
    lr = Lammps()
    lr.set_box(bed["boxlo"], bed["boxhi"])
    lr.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"], type_=two)
    for line in dc.script_lines(bed, cfg):
        lr.command("fix 4 bottom rigid/nve single" if line == "fix 4 bottom freeze" else line)
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        _cloud(lr, bed, _keys(bed))
    # a decomposed engine
    ld = dc.make_hip(bed, cfg)
    cloud = _cloud(ld, bed, {})
    assert ld.L.sf_dem_set_subdomain(ld.ptr, 0, 2, float(lo[0]), 0.5 * float(lo[0] + hi[0])) == 0
    with pytest.raises(SfError, match="one rank"):
        _set_feed(cloud, _keys(bed))
    cloud.close()
