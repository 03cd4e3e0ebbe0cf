"""Particle injection and removal (lammps_create_particle / lammps_delete_particle, library.cpp:406-621;
DemEngine::create_particles / delete_particles) across a live neighbour list, contact history, wall history and the
per-atom fix rows.

Two kinds of check:
  * the carry-over across the call is EXACT: the call moves rows and copies history, it computes nothing, so every
    survivor's record, stored force, wall history and pair history is compared with `==` (np.array_equal);
  * the run that continues is held to the CPU oracle's restatement of the same contract (oracle/orc_dem.c,
    orc_dem_add_atoms / orc_dem_delete_atoms: history by partner tag, lists rebuilt at the call) within the gates of the
    other parity tests (tests/test_dem_gpu.py::_compare: forces, torques, history 1e-12, states 1e-9), plus wall history,
    atom counts and the number of list builds.

Beds are FCC lattices of 256-500 grains, hot (0.3-0.5 m/s) so that contacts slide, with a thin skin so that lists are
also rebuilt on their own after the call.  No atom of these beds comes within 0.3 mm of a periodic face, so the forced
rebuild wraps nobody and positions are comparable bit for bit."""
import numpy as np
import pytest

from tests import dem_cases as dc
import tests.test_dem_gpu as T

pytestmark = pytest.mark.gpu

KEYS = ("x", "v", "omega", "f", "torque")
COHE_LUB = dict(cohesive=(1.0e-13, 1.0e-7, 1.0e-7, 1.0e-4, 1), lub=(1.0e-3, 1, 1, 1.001e-3, 1.1e-3, 1, 1))
D_NEW, RHO_NEW = 0.8e-3, 2000.0          # created grains: another size and density than the bed's
# fdrag rows: 1e-6 N on a 1.4e-6 kg grain changes v by F dt / m = 7e-7 m/s per sub-step; the velocity gate of _compare is
# 1e-9 of max |v| (below 1e-8 m/s here), so a survivor that integrates a neighbour's row fails after one sub-step
FDRAG_SCALE = 1.0e-6

FORMS = [{"SF_HIST_IN_PLACE": "0"}, {"SF_HIST_IN_PLACE": "1"}, {"SF_GHOST_FREE": "0"}, {"SF_GHOST_FREE": "1"},
         {"SF_BUILD_LDS": "0"}, {"SF_BUILD_QUAD": "0"}, {"SF_HIST_COPIES": "2"},
         {"SF_LDS": "1", "SF_TILE": "4", "SF_SUB": "1"}]
FORM_IDS = ["-".join("%s=%s" % kv for kv in sorted(f.items())) for f in FORMS]


def _case(name):
    """(bed, cfg): (a) periodic x/z over a y wall, Hertz; (b) closed box, three walls, Hooke with history; (c) polydisperse
    periodic (d in [0.9, 1.0] mm on a 0.95 mm lattice: half of the neighbours touch) with fix cohesive and lubricate/poly;
    (d) bed (a) with a carrier density, i.e. with the DuDt / vOld rows"""
    if name in ("a", "d"):
        bed = T._bed((5, 5, 5), periodic=True, seed=61, vmax=0.5)
        cfg = dict(T.BASE, skin=0.05e-3)
        if name == "d":
            cfg["carrier_rho"] = 1000.0
    elif name == "b":
        bed = T._bed((4, 4, 4), periodic=False, seed=62, vmax=0.5)
        cfg = dict(T.BASE, pair="hooke", kn=2.0e3, gamman=50.0, skin=0.05e-3)
    elif name == "c":
        bed = T._bed((5, 5, 5), periodic=True, seed=11, poly=(0.9e-3, 1.0e-3), spacing=0.95, vmax=0.3)
        cfg = dict(T.BASE, skin=0.08e-3, **COHE_LUB)
    else:
        raise KeyError(name)
    cfg["walls"] = T._walls(bed)
    return bed, cfg


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _snap(lmp, cfg):
    st = lmp.get_state()
    st["hist"] = lmp.history()
    st["wsh"] = [lmp.wall_shear(w) for w in range(len(cfg["walls"]))]
    st["order"] = lmp.get_local_info()["tag"].copy()          # engine order, unsorted
    return st


def _inside(bed, st):
    lo, hi = np.asarray(bed["boxlo"]), np.asarray(bed["boxhi"])
    return all(np.all((st["x"][:, k] >= lo[k]) & (st["x"][:, k] < hi[k])) for k in range(3) if bed["periodic"][k])


def _pick_dead(st, extra=2):
    """first, middle and last atom in ENGINE order (a compaction that goes wrong behind the first hole shows on all that
    follow it), plus the atoms at the quartiles"""
    o = st["order"]
    n = len(o)
    idx = [0, n // 2, n - 1] + [n // 4, (3 * n) // 4][:extra]
    return sorted({int(o[i]) for i in idx})


def _assert_carried(before, after, dead, label=""):
    """the exact statement: survivors matched by tag keep x, v, omega, f, torque and wall history bit for bit; the history
    is the one before minus every pair that holds a dead tag, each value bit for bit (the rebuild only copies; an owner
    flip negates exactly; both read-outs orient by tag).  Returns (surviving pairs with live shear, pairs dropped)."""
    dead = np.asarray(sorted(dead), dtype=np.int64)
    keep = ~np.isin(before["tag"], dead)
    sel = np.isin(after["tag"], before["tag"][keep])
    assert np.array_equal(after["tag"][sel], before["tag"][keep]), label
    for k in KEYS:
        bad = np.nonzero(np.any(after[k][sel] != before[k][keep], axis=1))[0]
        assert bad.size == 0, "%s %s: %d of %d survivors changed, first tag %d" % (
            label, k, bad.size, int(keep.sum()), int(before["tag"][keep][bad[0]]))
    for w, (wa, wb) in enumerate(zip(after["wsh"], before["wsh"])):
        bad = np.nonzero(np.any(wa[sel] != wb[keep], axis=1))[0]
        assert bad.size == 0, "%s wall %d history: %d survivors changed" % (label, w, bad.size)
    ds = set(dead.tolist())
    want = {k: s for k, s in before["hist"].items() if k[0] not in ds and k[1] not in ds}
    got = after["hist"]
    lost, new = set(want) - set(got), set(got) - set(want)
    changed = [k for k in want if k in got and not np.array_equal(got[k], want[k])]
    assert not lost and not new and not changed, "%s history: %d of %d surviving pairs lost, %d changed, %d new" % (
        label, len(lost), len(want), len(changed), len(new))
    live = sum(1 for s in want.values() if np.any(s != 0.0))
    return live, len(before["hist"]) - len(want)


def _check_delete(lmp, bed, cfg, dead=None, label=""):
    """A1 for a removal on the engine as it stands (between two runs); returns (snapshot after, dead tags)"""
    before = _snap(lmp, cfg)
    assert _inside(bed, before)
    if dead is None:
        dead = _pick_dead(before)
    o = before["order"]
    assert {int(o[0]), int(o[len(o) // 2]), int(o[-1])} <= set(dead)
    for t in dead:   # removed mid-contact
        assert any(t in k for k in before["hist"]), "dead tag %d touches nobody" % t
    n0, nb0 = lmp.get_local_n(), lmp.info().nbuilds
    lmp.delete_particle(dead)
    assert lmp.get_local_n() == lmp.get_global_n() == n0 - len(dead)
    assert lmp.info().nbuilds == nb0 + 1
    after = _snap(lmp, cfg)
    live, dropped = _assert_carried(before, after, dead, label)
    print("%s delete: %d surviving pairs with live shear, %d pairs dropped with %d atoms" % (label, live, dropped, len(dead)))
    assert live >= 100 and dropped >= len(dead)
    return after, dead


def _drop_sites(st, radius, count):
    """Where to create grains: one created diameter above the plane of the bed's top layer, over hollows of that
    layer (between four of its grains), and the common downward velocity that brings the slowest of them into contact
    within 25 sub-steps of 1 us.  `st`: tag-sorted state, `radius`: radii in the same order."""
    x = st["x"]
    ytop = x[:, 1].max()
    top = np.nonzero(x[:, 1] > ytop - 0.3e-3)[0]
    y0 = float(np.mean(x[top, 1])) + D_NEW
    ctr = 0.5 * (x[top][:, [0, 2]].min(axis=0) + x[top][:, [0, 2]].max(axis=0))
    sites, drops = [], []
    # hollows: midpoints of pairs of top-layer grains that are second neighbours (one lattice edge apart)
    order = np.argsort(np.hypot(x[top, 0] - ctr[0], x[top, 2] - ctr[1]))
    for i in top[order]:
        for j in top:
            h = np.hypot(x[i, 0] - x[j, 0], x[i, 2] - x[j, 2])
            if j <= i or not (1.25e-3 < h < 1.5e-3):
                continue
            p = np.array([0.5 * (x[i, 0] + x[j, 0]), y0, 0.5 * (x[i, 2] + x[j, 2])])
            if any(np.hypot(p[0] - q[0], p[2] - q[2]) < 1.2 * D_NEW for q in sites):
                continue
            hh = np.hypot(x[:, 0] - p[0], x[:, 2] - p[2])
            reach = radius + 0.5 * D_NEW
            near = hh < reach
            land = np.max(x[near, 1] + np.sqrt(reach[near] ** 2 - hh[near] ** 2)) if near.any() else -1.0
            if land < 0 or np.any(np.sqrt(hh ** 2 + (x[:, 1] - y0) ** 2) < reach + 0.02e-3):
                continue                          # nothing underneath, or too close to a grain already
            sites.append(p)
            drops.append(y0 - land)
            if len(sites) == count:
                return np.array(sites), -max(drops) / 25.0e-6
    raise AssertionError("no %d hollows in the top layer" % count)


def _check_create(lmp, bed, cfg, pos, tags, vel, label=""):
    """A1 for an injection; returns the snapshot after"""
    before = _snap(lmp, cfg)
    assert _inside(bed, before)
    n0, nb0 = lmp.get_local_n(), lmp.info().nbuilds
    lmp.create_particle(pos, tags, D_NEW, RHO_NEW, 1, vel)
    assert lmp.get_local_n() == lmp.get_global_n() == n0 + len(tags)
    assert lmp.info().nbuilds == nb0 + 1
    after = _snap(lmp, cfg)
    live, dropped = _assert_carried(before, after, [], label)       # new atoms start without contacts
    assert dropped == 0
    print("%s create: %d pairs with live shear carried, %d atoms created" % (label, live, len(tags)))
    new = np.isin(after["tag"], tags)
    assert new.sum() == len(tags)
    srt = np.argsort(np.asarray(tags))
    assert np.array_equal(after["x"][new], np.asarray(pos, dtype=np.float64)[srt])
    assert np.all(after["v"][new] == np.asarray(vel, dtype=np.float64))
    for k in ("omega", "f", "torque"):
        assert np.all(after[k][new] == 0.0), k
    assert all(np.all(w[new] == 0.0) for w in after["wsh"])
    return after


def _radius_by_tag(bed, st):
    r = np.full(len(st["tag"]), 0.5 * D_NEW)
    old = st["tag"] <= bed["n"]
    r[old] = 0.5 * np.asarray(bed["diameter"])[st["tag"][old] - 1]
    return r


def _parity(lmp, orc, cfg, tol_f):
    T._compare(lmp, orc, tol_f=tol_f)
    for w in range(len(cfg["walls"])):
        assert dc.rel_err(lmp.wall_shear(w), orc.wall_shear(w)) <= 1e-9, "wall %d" % w
    assert lmp.get_local_n() == lmp.get_global_n() == orc.nlocal
    assert lmp.info().nbuilds == orc.nbuilds


def _sequence(name, tol_f=1e-12, label=""):
    """A2: setup, seeded fdrag rows in shuffled order, 20 steps, delete, 40 steps, create, 40 steps -- engine and oracle
    side by side, compared after every piece; the exact carry-over is checked at both calls on the way"""
    bed, cfg = _case(name)
    lmp, orc = dc.make_hip(bed, cfg), dc.make_oracle(bed, cfg)
    lmp.setup(); orc.setup()
    _parity(lmp, orc, cfg, tol_f)
    rng = np.random.default_rng(7)
    st = orc.get()
    fd = rng.normal(scale=FDRAG_SCALE, size=st["x"].shape)
    perm = rng.permutation(len(fd))
    lmp.put_local_info(fd[perm], st["tag"][perm])
    orc.put_fdrag(fd[perm], st["tag"][perm])
    lmp.step(20); orc.run(20)
    _parity(lmp, orc, cfg, tol_f)
    _, dead = _check_delete(lmp, bed, cfg, label=label)
    assert orc.delete_particle(dead) == len(dead)
    _parity(lmp, orc, cfg, tol_f)              # (stored forces: the ones of the last evaluation, dead atoms' share included)
    lmp.step(40); orc.run(40)
    _parity(lmp, orc, cfg, tol_f)
    st = orc.get()
    pos, vy = _drop_sites(st, _radius_by_tag(bed, st), 4)
    tags = [bed["n"] + 1 + k for k in range(len(pos))]
    vel = [0.0, vy, 0.0]
    _check_create(lmp, bed, cfg, pos, tags, vel, label=label)
    orc.create_particle(pos, tags, D_NEW, RHO_NEW, 1, vel)
    _parity(lmp, orc, cfg, tol_f)
    lmp.step(40); orc.run(40)
    _parity(lmp, orc, cfg, tol_f)
    h = lmp.history()
    landed = [k for k in h if k[0] in tags or k[1] in tags]
    print("%s: %d contacts of created grains after 40 steps (vy = %.2f m/s), %d builds" % (label, len(landed), vy, orc.nbuilds))
    assert landed, "no created grain touches the bed"
    assert any(np.any(h[k] != 0.0) for k in landed)       # ... with history
    assert orc.nbuilds >= 5                               # setup, the two calls, and rebuilds of their own


# ---- A1: exact carry-over across the call, no oracle -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_removal_carries_every_survivor_bit_for_bit(name):
    bed, cfg = _case(name)
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    _check_delete(lmp, bed, cfg, label="bed " + name)
    lmp.step(5)
    assert np.isfinite(lmp.get_state()["x"]).all()


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_injection_leaves_every_old_atom_bit_for_bit(name):
    bed, cfg = _case(name)
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    st = lmp.get_state()
    pos, vy = _drop_sites(st, _radius_by_tag(bed, st), 4)
    after = _check_create(lmp, bed, cfg, pos, [bed["n"] + 1 + k for k in range(4)], [0.0, vy, 0.0], label="bed " + name)
    assert sum(1 for s in after["hist"].values() if np.any(s != 0.0)) >= 100


# ---- A2: the run that continues, against the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_run_through_removal_and_injection_against_oracle(name):
    _sequence(name, label="bed " + name)


# ---- A3: the forms of the rebuild the call can meet ---------------------------------------------------------------------

@pytest.mark.parametrize("env", FORMS, ids=FORM_IDS)
def test_removal_exact_in_every_form_of_the_rebuild(env, monkeypatch):
    """Every knob of FORMS is read when the engine is constructed (docs/knobs.md), so each case really runs its own form
    whatever ran before it in the process.  The form that used to lose history here is the default, SF_HIST_IN_PLACE=1:
    the old list was read in place at compacted indices (half of the surviving pairs lost, a quarter given another
    pair's shear); a removal now always stages the rows by partner tag."""
    _setenv(monkeypatch, env)
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    _check_delete(lmp, bed, cfg, label=FORM_IDS[FORMS.index(env)])


@pytest.mark.parametrize("env", FORMS, ids=FORM_IDS)
def test_injection_exact_in_every_form_of_the_rebuild(env, monkeypatch):
    _setenv(monkeypatch, env)
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    st = lmp.get_state()
    pos, vy = _drop_sites(st, _radius_by_tag(bed, st), 4)
    _check_create(lmp, bed, cfg, pos, [bed["n"] + 1 + k for k in range(4)], [0.0, vy, 0.0],
                  label=FORM_IDS[FORMS.index(env)])


@pytest.mark.parametrize("env", FORMS, ids=FORM_IDS)
def test_run_through_both_calls_in_every_form_of_the_rebuild(env, monkeypatch):
    """The LDS-staged form (list words index ghost slots) is the one only this run can judge: created atoms used to take
    the first ghosts' slots before the history was staged, and the copy of an owned-ghost pair on the higher tag's side
    -- which history() does not report -- lost its shear: forces 1e-3 off forty steps later."""
    _setenv(monkeypatch, env)
    _sequence("a", label=FORM_IDS[FORMS.index(env)])


# ---- A4: edges ------------------------------------------------------------------------------------------------------------

def test_capacity_grows_under_a_live_list():
    """One create_particle call with more grains than the per-atom arrays have room for: ensure_capacity re-strides every
    [rows][capacity] array -- the list and both history buffers among them -- while the old list is still needed.  The new
    grains are a lattice above the bed (they touch neither each other nor the bed at the call), falling at 8 m/s: the lowest
    layer reaches the bed within the 20 steps."""
    bed = T._bed((4, 4, 4), periodic=True, seed=63, vmax=0.5, y_gap_top=0.2)
    cfg = dict(T.BASE, skin=0.05e-3)
    cfg["walls"] = T._walls(bed)
    lmp, orc = dc.make_hip(bed, cfg), dc.make_oracle(bed, cfg)
    lmp.setup(); orc.setup()
    lmp.step(25); orc.run(25)
    cap0, n0 = lmp.info().capacity, lmp.get_local_n()
    st = orc.get()
    per_side = 6
    lx, lz = float(bed["boxhi"][0]), float(bed["boxhi"][2])
    assert lx / per_side > D_NEW + 0.05e-3 and lz / per_side > D_NEW + 0.05e-3
    need = cap0 - n0 + 64                                   # well past what is left of the capacity
    layers = -(-need // (per_side * per_side))
    ylo = float(st["x"][:, 1].max()) + 0.5e-3 + 0.5 * D_NEW + 0.05e-3      # clear of every bed grain
    dy = D_NEW + 0.05e-3
    assert ylo + layers * dy < float(bed["boxhi"][1]) - D_NEW
    g = np.arange(per_side)
    pos = np.array([[(i + 0.5) * lx / per_side, ylo + l * dy, (k + 0.5) * lz / per_side]
                    for l in range(layers) for i in g for k in g])
    tags = np.arange(n0 + 1, n0 + 1 + len(pos))
    vel = [0.0, -8.0, 0.0]
    after = _check_create(lmp, bed, cfg, pos, tags, vel, label="capacity")
    cap1 = lmp.info().capacity
    print("capacity %d -> %d for %d + %d atoms" % (cap0, cap1, n0, len(pos)))
    assert cap1 > cap0
    assert sum(1 for s in after["hist"].values() if np.any(s != 0.0)) >= 100
    orc.create_particle(pos, tags, D_NEW, RHO_NEW, 1, vel)
    lmp.step(20); orc.run(20)
    _parity(lmp, orc, cfg, 1e-12)
    assert any(k[1] > n0 for k in lmp.history())           # the lowest layer has landed


def test_unknown_tags_change_nothing():
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    before = _snap(lmp, cfg)
    nb = lmp.info().nbuilds
    lmp.delete_particle([bed["n"] + 7, 10 ** 6])
    after = _snap(lmp, cfg)
    assert lmp.info().nbuilds == nb and lmp.get_local_n() == lmp.get_global_n() == bed["n"]
    assert np.array_equal(after["order"], before["order"])
    live, dropped = _assert_carried(before, after, [], "unknown tags")
    assert live >= 100 and dropped == 0


def test_duplicate_tags_remove_once():
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(25)
    before = _snap(lmp, cfg)
    dead = _pick_dead(before, extra=0)
    lmp.delete_particle([dead[0]] + dead + [dead[-1], dead[0]])
    assert lmp.get_local_n() == lmp.get_global_n() == bed["n"] - len(dead)
    after = _snap(lmp, cfg)
    assert sorted(after["tag"].tolist()) == sorted(set(before["tag"].tolist()) - set(dead))
    _assert_carried(before, after, dead, "duplicates")


def _two_grains():
    x = np.array([[2.0e-3, 0.6e-3, 2.0e-3], [2.7e-3, 0.9e-3, 2.1e-3]])      # 0.768 mm apart: overlapping; clear of the wall
    return x


def test_remove_all_then_refill():
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    lmp.step(10)
    lmp.delete_particle(lmp.get_local_info()["tag"])
    assert lmp.get_local_n() == lmp.get_global_n() == 0
    lmp.step(5)
    assert lmp.get_local_n() == 0 and lmp.history() == {}
    # two grains into the emptied engine, one call each (a velocity per call), against a fresh oracle of those two
    x = _two_grains()
    v = np.array([[0.3, -0.2, 0.0], [-0.3, 0.0, 0.1]])
    tags = [901, 902]
    for k in range(2):
        lmp.create_particle(x[k], [tags[k]], D_NEW, RHO_NEW, 1, v[k])
    r = 0.5 * D_NEW
    m = 4.0 * 3.14159265358917323846 / 3.0 * r * r * r * RHO_NEW
    # The fresh oracle takes the same road: a set-up driver emptied, then the two grains through its own create call.  (A
    # driver constructed from the two grains would weigh them with the true pi and, at its setup, evaluate the forces the
    # created grains do not have yet: no force is computed at the call, on either side.)
    two = dict(bed, x=x, v=v, diameter=np.full(2, D_NEW), density=np.full(2, RHO_NEW), n=2, tag=np.array(tags, np.int32))
    orc = dc.make_oracle(two, cfg)
    orc.setup()
    assert orc.delete_particle(tags) == 2 and orc.nlocal == 0
    for k in range(2):
        orc.create_particle(x[k], [tags[k]], D_NEW, RHO_NEW, 1, v[k])
    assert np.all(orc.mass() == m)
    lmp.step(30); orc.run(30)
    T._compare(lmp, orc)
    assert set(lmp.history()) == {(901, 902)} and lmp.get_local_n() == orc.nlocal == 2


def test_injection_and_removal_before_setup():
    bed, cfg = _case("a")
    lmp, orc = dc.make_hip(bed, cfg), dc.make_oracle(bed, cfg)
    n = bed["n"]
    dead = [1, n // 2, n]
    lmp.delete_particle(dead)
    assert orc.delete_particle(dead) == 3
    top = float(bed["x"][:, 1].max())
    pos = np.array([[1.0e-3, top + 1.2e-3, 1.0e-3], [3.0e-3, top + 1.2e-3, 2.0e-3]])
    tags = [n + 1, n + 2]
    lmp.create_particle(pos, tags, D_NEW, RHO_NEW, 1, [0.0, -8.0, 0.0])
    orc.create_particle(pos, tags, D_NEW, RHO_NEW, 1, [0.0, -8.0, 0.0])
    assert lmp.get_local_n() == lmp.get_global_n() == orc.nlocal == n - 1
    want = sorted((set(range(1, n + 1)) - set(dead)) | set(tags))
    assert sorted(lmp.get_local_info()["tag"].tolist()) == want and orc.get()["tag"].tolist() == want
    assert lmp.info().nbuilds == 0 and orc.nbuilds == 0
    lmp.setup(); orc.setup()
    _parity(lmp, orc, cfg, 1e-12)
    lmp.step(20); orc.run(20)
    _parity(lmp, orc, cfg, 1e-12)


def test_mass_of_a_created_grain_bit_for_bit():
    """rmass through `compute property/atom mass` against the double product of library.cpp:460, in its order and with its
    literal, which differs from pi in the 13th digit: a relative bound of 1e-12 cannot tell the two, == can"""
    bed, cfg = _case("a")
    lmp = dc.make_hip(bed, cfg)
    lmp.setup()
    n = bed["n"]
    top = float(bed["x"][:, 1].max())
    lmp.create_particle([[1.0e-3, top + 2.0e-3, 1.0e-3]], [n + 1], D_NEW, RHO_NEW, 1, [0.0, 0.0, 0.0])
    lmp.command("compute m all property/atom mass")
    mass = lmp.compute_atom("m")
    radtmp = 0.5 * D_NEW
    want = 4.0 * 3.14159265358917323846 / 3.0 * radtmp * radtmp * radtmp * RHO_NEW
    with_pi = 4.0 * np.pi / 3.0 * radtmp * radtmp * radtmp * RHO_NEW
    assert want != with_pi and abs(want / with_pi - 1.0) < 1e-12
    assert len(mass) == n + 1 and mass[n] == want
