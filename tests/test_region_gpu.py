"""`region`, `group ID region`, `group ID dynamic ... region ... every N` on the GPU (DESIGN.md section 18;
csrc/sf_region_match.h, sf_region_parse.h, sf_region.hip) against the NumPy statement tests/region_model.py (held to
hand-computed answers by tests/test_region_model.py).

Every comparison is ==: the kernel evaluates the model's own expressions, operation by operation, and membership is a bool.
The model is fed the engine's own bits (get_local_info()), in the engine's atom order, which is the order of group_mask().

The beds: the eight free-flight grains and the sheared 400-grain bed of tests/test_displace_gpu.py, the 108-grain bed of
tests/test_contacts_gpu.py, and 70 hand-placed atoms on a 2^-1 grid."""
import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError, restart
from tests import chunk_model as km
from tests import dem_cases as dc
from tests import global_model as gm
from tests import region_model as rm
from tests.test_compute_atom_gpu import _decompose
from tests.test_contacts_gpu import _small
from tests.test_displace_gpu import FF_V, FF_X, N_FLOW, _flow_bed, _flow_engine
from tests.test_dump_gpu import frames

pytestmark = pytest.mark.gpu

BIG = rm.BIG


def _free_flight(extra=()):
    """the eight grains of test_displace_gpu.test_free_flight_is_exact: box [0, 4)^3, dyadic numbers, dt = 2^-10"""
    lmp = Lammps()
    lmp.set_box([0.0, 0.0, 0.0], [4.0, 4.0, 4.0])
    lmp.create_atoms(np.array(FF_X), np.full(8, 0.125), np.full(8, 1.0), v=np.array(FF_V))
    for line in ["atom_style sphere", "boundary p p p", "newton off", "communicate single vel yes", "neighbor 0.25 bin",
                 "neigh_modify delay 0", "pair_style gran/hooke/history 1000.0 NULL 1.0 NULL 0.5 1", "pair_coeff * *",
                 "timestep %.17g" % 2.0 ** -10, "fix 1 all nve/sphere"] + list(extra):
        lmp.command(line)
    return lmp


def _define(lmp, rid, region):
    """the region, its sub-regions first (IDs rid_0, rid_1, ...)"""
    if region[0] in ("union", "intersect"):
        ids = []
        for k, sub in enumerate(region[1]):
            ids.append("%s_%d" % (rid, k))
            _define(lmp, ids[-1], sub)
        lmp.command("region %s %s %d %s side %s units box" % (rid, region[0], len(ids), " ".join(ids), region[-1]))
    else:
        lmp.command(rm.command(rid, region))


def _check_group(lmp, name, want, what=""):
    """group_mask and group_count against a bool per atom in the engine's order"""
    got = lmp.group_mask(name)
    assert got.dtype == bool and got.shape == want.shape
    assert (got == want).all(), (what, np.nonzero(got != want)[0])
    assert lmp.group_count(name) == int(want.sum()), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. points

BLOCK = ("block", 0.5, 2.0, 1.0, 3.0, 0.25, 3.5, "in")
R_S = 1.3125                                    # r / 3 = 7/16 and r / 7 = 3/16 are dyadic: the quadruples are exact
SPHERE = ("sphere", 2.0, 2.0, 2.0, R_S, "in")
R_C = 1.25                                      # r / 5 = 1/4
CYL_Z = ("cylinder", "z", 2.0, 2.0, R_C, 0.5, 3.0, "in")
CYL_X = ("cylinder", "x", 2.0, 1.5, R_C, -BIG, 4.0, "out")      # lo INF, hi EDGE of the box [0, 4]
CYL_Y = ("cylinder", "y", 1.0, 2.5, R_C, 0.0, BIG, "in")        # lo EDGE, hi INF
PLANE = ("plane", 1.0, 1.0, 1.0, 3.0, 4.0, 0.0, "in")
PLANE_Z = ("plane", 0.0, 0.0, 1.5, 0.0, 0.0, -2.0, "out")
BLOCK_INF = ("block", -BIG, BIG, 1.0, 4.0, 0.0, 3.5, "out")     # INF INF 1 EDGE EDGE 3.5
NESTED = ("union", [("intersect", [BLOCK, CYL_Z], "in"), ("sphere", 2.0, 2.0, 2.0, R_S, "out")], "in")
POINT_REGIONS = dict(block=BLOCK, sphere=SPHERE, cylz=CYL_Z, cylx=CYL_X, cyly=CYL_Y, plane=PLANE, planez=PLANE_Z,
                     blockinf=BLOCK_INF, nested=NESTED)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)


def _signed_perms(t):
    out = set()
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for s in range(8):
            out.add(tuple(t[p[k]] * (1.0 if (s >> k) & 1 else -1.0) for k in range(3)))
    return np.array(sorted(out))


def _pool():
    """every point set of the issue in one pool, shuffled by a fixed seed so that each prefix is a mixture"""
    g = np.array([0.4375, 0.5, 0.5625, 1.0, 1.25, 1.9375, 2.0, 2.0625, 3.0, 3.5])          # a 2^-4 grid through every face
    gy = np.array([0.9375, 1.0, 1.0625, 2.0, 2.9375, 3.0, 3.0625])
    gz = np.array([0.1875, 0.25, 0.3125, 1.5, 3.4375, 3.5, 3.5625])
    lattice = np.array([[a, b, c] for a in g for b in gy for c in gz])
    c = np.array([2.0, 2.0, 2.0])
    sph = np.concatenate([c + _signed_perms((1.0, 2.0, 2.0)) * (R_S / 3.0), c + _signed_perms((2.0, 3.0, 6.0)) * (R_S / 7.0)])
    ring = np.array([[sx * a, sy * b] for a, b in ((3.0, 4.0), (4.0, 3.0), (5.0, 0.0), (0.0, 5.0)) for sx in (-1.0, 1.0)
                     for sy in (-1.0, 1.0)]) * (R_C / 5.0)
    cyl = np.concatenate([np.column_stack([2.0 + ring[:, 0], 2.0 + ring[:, 1], np.full(len(ring), z)]) for z in (0.5, 1.0, 3.0, 3.25)] +
                         [np.column_stack([np.full(len(ring), x), 2.0 + ring[:, 0], 1.5 + ring[:, 1]]) for x in (-1.0, 4.0, 4.5)] +
                         [np.column_stack([1.0 + ring[:, 0], np.full(len(ring), y), 2.5 + ring[:, 1]]) for y in (0.0, -0.5, 7.0)])
    onplane = np.array([[1.0, 1.0, z] for z in (-3.0, 1.0, 9.0)] + [[x, y, 1.5] for x in (0.0, 2.5) for y in (-1.0, 3.0)] +
                       [[1.0 + 4.0 * t, 1.0 - 3.0 * t, 2.0] for t in (-2.0, -0.5, 0.25, 1.0, 3.0)])
    far = np.array([[1.0e25, 2.0, 1.0], [-1.0e25, 2.0, 1.0], [1.0, 1.0e19, 1.0], [1.0, -1.0e21, 1.0], [2.0, 2.0, 1.0e300],
                    [-7.0, 2.0, 1.5], [2.0, 1.5, -9.0e19], [1.0, 1.0e19, 2.5], [1.0e150, 1.0e150, 1.0e150]])
    rnd = np.random.default_rng(20261).uniform(-1.0, 5.0, size=(1025, 3))
    pool = np.concatenate([lattice, sph, cyl, onplane, far, rnd])
    return np.ascontiguousarray(pool[np.random.default_rng(7).permutation(len(pool))])


POOL = _pool()


@pytest.fixture(scope="module")
def points_engine():
    lmp = _free_flight()
    for rid, region in POINT_REGIONS.items():
        _define(lmp, rid, region)
    yield lmp
    lmp.close()


def _primitives(region):
    return [q for sub in region[1] for q in _primitives(sub)] if region[0] in ("union", "intersect") else [region]


def _classes(region, p):
    """(on a surface, matching and on none, not matching and on none) of the points p, from the model; for a union or
    intersect `on a surface` is: on the surface of one of its primitives"""
    on = np.any([rm.on_boundary(q, p) for q in _primitives(region)], axis=0)
    m = rm.match(region, p)
    return on, m & ~on, ~m & ~on


def _ordered(rid):
    """the pool in an order of its own for region `rid`: a point on a surface, a matching one, a non-matching one, and so on
    in turn while each class lasts, so that EVERY prefix of three points or more -- the arrays the count test passes to
    the GPU -- holds a point inside, one outside and one exactly on a surface"""
    on, yes, no = [list(np.nonzero(c)[0]) for c in _classes(POINT_REGIONS[rid], POOL)]
    order = []
    for k in range(len(POOL)):
        for c in (on, yes, no):
            if k < len(c):
                order.append(c[k])
    assert sorted(order) == list(range(len(POOL)))
    return np.ascontiguousarray(POOL[order])


def _assert_conditions(rid, p):
    """from the model alone, on exactly the array that goes to the GPU"""
    on, yes, no = _classes(POINT_REGIONS[rid], p)
    m = rm.match(POINT_REGIONS[rid], p)
    assert on.any() and m.any() and (~m).any() and (yes.any() or no.any()), rid
    assert (on & m).any() or (on & ~m).any()


def test_the_pool_holds_every_point_set_of_the_issue():
    """conditions on the pool, from the model alone; test_region_match_of_the_whole_pool_is_the_model passes ALL of it"""
    assert len(POOL) >= max(COUNTS)
    for rid in POINT_REGIONS:
        _assert_conditions(rid, POOL)
    # every face, edge and corner of the block
    b = BLOCK
    for cx in (b[1], b[2], 1.25):
        for cy in (b[3], b[4], 2.0):
            for cz in (b[5], b[6], 1.5):
                assert ((POOL[:, 0] == cx) & (POOL[:, 1] == cy) & (POOL[:, 2] == cz)).any(), (cx, cy, cz)
    assert rm.on_boundary(SPHERE, POOL).sum() >= 72 and rm.on_boundary(CYL_Z, POOL).sum() >= 48
    assert rm.on_boundary(CYL_X, POOL).sum() >= 32 and rm.on_boundary(CYL_Y, POOL).sum() >= 32
    assert rm.on_boundary(PLANE, POOL).sum() >= 3 and rm.on_boundary(PLANE_Z, POOL).sum() >= 4
    assert (np.abs(POOL) > 4.0).any(axis=1).sum() > 100          # points outside the box [0, 4]^3


@pytest.mark.parametrize("rid", sorted(POINT_REGIONS))
def test_region_match_of_the_whole_pool_is_the_model(points_engine, rid):
    """every point of every set: all faces, edges and corners, all quadruples, all rings, all points on the planes"""
    _assert_conditions(rid, POOL)
    got = points_engine.region_match(rid, POOL)
    want = rm.match(POINT_REGIONS[rid], POOL)
    assert got.shape == (len(POOL),) and got.dtype == bool
    assert (got == want).all(), (rid, POOL[got != want])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("rid", sorted(POINT_REGIONS))
def test_region_match_of_points_is_the_model(points_engine, rid, n):
    """the tail lane in the first wave, at a wave edge and at a block edge; the n points are the first n of the pool in the
    region's own order, and the conditions are asserted on those n"""
    p = _ordered(rid)[:n]
    if n >= 3:
        _assert_conditions(rid, p)
    else:
        assert np.any([rm.on_boundary(q, p) for q in _primitives(POINT_REGIONS[rid])])     # the one point is on a surface
    got = points_engine.region_match(rid, p)
    want = rm.match(POINT_REGIONS[rid], p)
    assert got.shape == (n,) and got.dtype == bool
    assert (got == want).all(), (rid, n, p[got != want])


def test_inf_and_edge_are_big_and_the_box_bound(points_engine):
    lmp = points_engine
    lmp.command("region e block EDGE EDGE INF INF 1 EDGE units box")
    want = rm.match(("block", 0.0, 4.0, -BIG, BIG, 1.0, 4.0, "in"), POOL)
    assert (lmp.region_match("e", POOL) == want).all() and want.any() and (~want).any()
    lmp.command("region e delete")
    with pytest.raises(SfError, match="Region ID does not exist"):
        lmp.region_match("e", POOL[:1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. static groups

def _engine_x(lmp):
    li = lmp.get_local_info()
    return li["x"], li["tag"]


def test_static_region_groups_on_the_small_bed():
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lo, hi = np.asarray(bed["boxlo"], float), np.asarray(bed["boxhi"], float)
    mid = 0.5 * (lo + hi)
    left = ("block", -BIG, mid[0], -BIG, BIG, -BIG, BIG, "in")
    ball = ("sphere", mid[0], 0.25 * (lo[1] + hi[1]), mid[2], 0.3 * (hi[0] - lo[0]), "in")
    _define(lmp, "left", left)
    _define(lmp, "ball", ball)
    x, tag = _engine_x(lmp)
    before = lmp.region_launches()
    lmp.command("group g region left")
    assert lmp.region_launches() == before + 1
    wl, wb = rm.match(left, x), rm.match(ball, x)
    assert 0 < wl.sum() < len(wl) and 0 < wb.sum() < len(wb) and (wb & ~wl).any() and (wb & wl).any()
    _check_group(lmp, "g", wl, "left")
    lmp.command("group g region ball")                      # adds to the group
    _check_group(lmp, "g", wl | wb, "left + ball")
    lmp.command("group b region ball")
    lmp.command("group only subtract g b")
    _check_group(lmp, "only", (wl | wb) & ~wb, "subtract")
    lmp.command("group l region left")
    lmp.command("group both intersect l b")
    _check_group(lmp, "both", wl & wb, "intersect")
    _check_group(lmp, "all", np.ones(len(tag), bool), "all")
    # by tag, and still so after a run that re-sorts nothing away
    by_tag = dict(zip(tag.tolist(), (wl | wb).tolist()))
    lmp.command("run 20")
    tag2 = lmp.get_local_info()["tag"]
    assert (lmp.group_mask("g") == np.array([by_tag[t] for t in tag2.tolist()])).all()
    lmp.close()


def test_static_region_group_with_atoms_exactly_on_the_faces():
    """70 atoms at (0.5 + 0.5 i, 0.5 + 0.5 j, 1 + k): the block [1, 2.5] x [1, 2] x [1, 1] has atoms on every face"""
    x = np.array([[0.5 + 0.5 * i, 0.5 + 0.5 * j, 1.0 + k] for i in range(7) for j in range(5) for k in range(2)])
    assert len(x) == 70
    lmp = Lammps()
    lmp.set_box([0.0, 0.0, 0.0], [4.0, 4.0, 4.0])
    lmp.create_atoms(x, np.full(70, 0.125), np.full(70, 1.0))
    for line in ["atom_style sphere", "boundary p p p", "newton off", "neighbor 0.25 bin", "neigh_modify delay 0",
                 "pair_style gran/hooke/history 1000.0 NULL 1.0 NULL 0.5 1", "pair_coeff * *", "timestep 1.0e-3"]:
        lmp.command(line)
    slab = ("block", 1.0, 2.5, 1.0, 2.0, 1.0, 1.0, "in")
    _define(lmp, "slab", slab)
    _define(lmp, "notslab", slab[:-1] + ("out",))
    xe, _ = _engine_x(lmp)
    want = rm.match(slab, xe)
    assert want.sum() == 4 * 3 and rm.on_boundary(slab, xe).sum() == 12      # i in 1..4, j in 1..3, k = 0: all on z = 1
    lmp.command("group in region slab")
    lmp.command("group out region notslab")
    _check_group(lmp, "in", want, "slab")
    _check_group(lmp, "out", ~want, "side out")
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the dynamic schedule, exact

# grain 4 enters through xhi at step 6, grain 1 through yhi at step 13, grain 3 leaves through zlo at step 19
SCHED_BLOCK = ("block", -BIG, 3.6875 - 6.0 / 256.0, 0.5, 3.3125 - 13.0 / 256.0, 1.375 - 18.0 / 256.0, BIG, "in")
SCHED_N = 4
SCHED_PIECES = [("run", 7), ("run", 7), ("run", 1), ("step", 3), ("step", 1), ("step", 0), ("run", 0), ("step", 2)]
SCHED_END = sum(n for _, n in SCHED_PIECES)


@pytest.fixture(scope="module")
def flight_positions():
    """engine A: no region; the positions at every step 0 .. SCHED_END, in tag order (tags 1 .. 8 are the rows of FF_X)"""
    A = _free_flight()
    xs = []
    for t in range(SCHED_END + 1):
        if t:
            A.command("run 1")
        li = A.get_local_info()
        xs.append(li["x"][np.argsort(li["tag"], kind="stable")])
    A.close()
    x0, v0 = np.array(FF_X), np.array(FF_V)
    for t, x in enumerate(xs):
        assert (x == x0 + (t * 2.0 ** -10) * v0).all(), t        # exact, and no wrap in these few steps
    return xs


def test_the_schedule_case_can_tell_the_rules_apart(flight_positions):
    """from the model alone: membership differs between consecutive deciding steps, between a deciding step and the end of
    its piece, between the start of a `step` piece and its deciding step, and at a run's setup that is no multiple of N"""
    M = [rm.match(SCHED_BLOCK, x) for x in flight_positions]
    assert 0 < M[0].sum() < 8
    deciding = rm.deciding_steps(0, SCHED_PIECES, SCHED_N)
    assert deciding == [4, 12, 14, 16, 16, 16, 19, 20]
    ends = np.cumsum([n for _, n in SCHED_PIECES]).tolist()
    starts = [0] + ends[:-1]
    assert sum((M[a] != M[b]).any() for a, b in zip(deciding[:-1], deciding[1:])) >= 3
    assert sum((M[d] != M[e]).any() for d, e in zip(deciding, ends)) >= 3
    # run 1 from step 14: only the setup can have given M[14], the last multiple of 4 gives another answer
    assert SCHED_PIECES[2] == ("run", 1) and (M[14] != M[12]).any()
    # step(1) to 19 and step(0) at 19: an evaluation at the end or at the start of the piece would have given M[19]
    assert (M[19] != M[16]).any() and starts[5] == 19 and SCHED_PIECES[5] == ("step", 0)
    assert SCHED_PIECES[6] == ("run", 0) and deciding[6] == 19


def test_dynamic_group_follows_the_schedule_exactly(flight_positions):
    M = [rm.match(SCHED_BLOCK, x) for x in flight_positions]
    B = _free_flight()
    _define(B, "r", SCHED_BLOCK)
    B.command("group g dynamic all region r every %d" % SCHED_N)
    assert not B.group_mask("g").any() and B.group_count("g") == 0 and B.region_launches() == 0    # the command assigns nothing
    deciding = rm.deciding_steps(0, SCHED_PIECES, SCHED_N)
    t = 0
    for (kind, n), d in zip(SCHED_PIECES, deciding):
        if kind == "run":
            B.command("run %d" % n)
        else:
            B.step(n)
        t += n
        li = B.get_local_info()
        assert B.info().nsteps == t
        assert (li["x"][np.argsort(li["tag"], kind="stable")] == flight_positions[t]).all()
        _check_group(B, "g", M[d][li["tag"] - 1], (kind, n, t, d))
    # a group defined between step() pieces is evaluated once at the next piece, whatever the step; a formerly static
    # group keeps its atoms until then
    r2 = ("block", -BIG, 2.2, -BIG, BIG, -BIG, BIG, "in")           # another region, so that the two counters differ
    _define(B, "r2", r2)
    M2 = rm.match(r2, flight_positions[t])
    assert M2.sum() == 3 and M[20].sum() == 5
    B.command("group h type 1")
    B.command("group h dynamic all region r2 every 100")
    assert B.group_mask("h").all() and B.group_count("h") == 8        # (no launch has counted it yet: counted as it stands)
    launches = B.region_launches()
    B.step(1)
    li = B.get_local_info()
    _check_group(B, "h", M2[li["tag"] - 1], "first piece after the definition")
    # g was not due in that launch (step 22, every 4), only counted in it: its counter is its population as it stood
    assert B.region_launches() == launches + 1
    _check_group(B, "g", M[20][li["tag"] - 1], "only counted")
    # ... and at step 24 it is h that is only counted, g that is evaluated (from positions the model extrapolates exactly)
    B.step(2)
    li = B.get_local_info()
    x24 = np.array(FF_X) + (24 * 2.0 ** -10) * np.array(FF_V)
    assert B.region_launches() == launches + 2 and (li["x"][np.argsort(li["tag"], kind="stable")] == x24).all()
    _check_group(B, "h", M2[li["tag"] - 1], "only counted, step 24")
    _check_group(B, "g", rm.match(SCHED_BLOCK, x24)[li["tag"] - 1], "evaluated, step 24")
    # a slot that is used again does not show its earlier owner's count
    B.command("group h static")
    B.command("group k dynamic all region r every 100")
    assert B.group_count("k") == 0 and not B.group_mask("k").any()
    B.command("group k static")
    B.command("group h dynamic all region r2 every 100")
    # group static freezes the membership: no further update, and the other styles work on it again
    B.command("group g static")
    keep = dict(zip(li["tag"].tolist(), B.group_mask("g").tolist()))
    launches = B.region_launches()
    B.command("group h static")
    B.command("run 8")
    assert B.region_launches() == launches
    li = B.get_local_info()
    assert B.group_mask("g").tolist() == [keep[q] for q in li["tag"].tolist()]
    B.close()


def test_a_cut_of_the_run_is_not_a_setup(flight_positions, tmp_path):
    """fix ave/time 1 1 1 cuts the run at every step; the sum of the tags of a dynamic group with every 4 changes at
    multiples of 4 only"""
    M = [rm.match(SCHED_BLOCK, x) for x in flight_positions]
    tags = np.arange(1, 9)
    want = {t: float(tags[M[SCHED_N * (t // SCHED_N)]].sum()) for t in range(SCHED_END + 1)}
    now = {t: float(tags[M[t]].sum()) for t in range(SCHED_END + 1)}
    assert len({want[t] for t in range(0, SCHED_END + 1, SCHED_N)}) >= 4 and sum(want[t] != now[t] for t in want) >= 3
    C = _free_flight()
    _define(C, "r", SCHED_BLOCK)
    path = str(tmp_path / "sum.txt")
    for line in ["group g dynamic all region r every %d" % SCHED_N, "compute p all property/atom id type",
                 "compute s g reduce sum c_p[1]", "fix f g ave/time 1 1 1 c_s file " + path]:
        C.command(line)
    C.command("run %d" % SCHED_END)
    got = C.ave_time("f")
    assert got["step"] == SCHED_END and got["values"][0] == want[SCHED_END]
    C.close()
    rows = [ln.split() for ln in open(path).read().splitlines() if not ln.startswith("#")]
    series = {int(r[0]): float(r[1]) for r in rows}
    assert sorted(series) == list(range(SCHED_END + 1))
    assert series == want


# ---------------------------------------------------------------------------------------------------------------------
# 4. readers, 5. passive, 6. reordering and atom changes: the sheared bed

H_FRAC = 0.55        # the dynamic group: above this fraction of the bed's height


def _above(bed):
    z = bed["x"][:, 2]
    h = float(z.min() + H_FRAC * (z.max() - z.min()))
    return ("block", -BIG, BIG, -BIG, BIG, h, BIG, "in")


def test_readers_of_a_dynamic_group(tmp_path):
    bed = _flow_bed()
    up = _above(bed)
    dump = str(tmp_path / "up.dump")
    delta = 1.0e-3
    chunk_args = "bin/1d z lower %r units box" % delta
    lmp = _flow_engine(bed, [rm.command("up", up), "group up dynamic all region up every 5",
                             "group up2 dynamic two region up every 5",
                             "dump d up custom 10 %s id x y z" % dump,
                             "compute cc up chunk/atom " + chunk_args,
                             "fix fc up ave/chunk 10 1 10 cc density/number",
                             "compute vxa up reduce ave vx"])
    before = lmp.region_launches()
    lmp.command("run 20")
    assert lmp.region_launches() - before == 1 + 4            # the setup and steps 5 10 15 20: two groups, one launch each
    lmp.sync()
    li = lmp.get_local_info()
    want = rm.match(up, li["x"])                              # step 20 is a multiple of 5: decided by the positions now
    assert 0.1 * N_FLOW < want.sum() < 0.9 * N_FLOW
    _check_group(lmp, "up", want, "up")
    _check_group(lmp, "up2", want & (np.asarray(bed["type"])[li["tag"] - 1] == 2), "up2: the parent is `two`")
    # dump custom: the frame of step 20 holds exactly the model's tags
    fr = frames(dump)
    assert [f[0] for f in fr] == [0, 10, 20]
    assert sorted(int(r.split()[0]) for r in fr[-1][3]) == sorted(li["tag"][want].tolist())
    # chunk/atom + ave/chunk density/number: the model fed the model's mask
    B = km.bins("compute cc up chunk/atom " + chunk_args, bed["boxlo"], bed["boxhi"], bed["periodic"])
    avg = km.Averager(B, ["density/number"], "all", False, 1)
    avg.add_sample(km.assign(B, li["x"], want), {})
    count, values = avg.output()
    got = lmp.ave_chunk("fc")
    assert got["step"] == 20 and (got["count"] == count).all() and (got["values"] == values).all() and count.sum() == want.sum()
    # compute reduce ave vx over the group, within the summation bound of tests/global_model.py
    vx = li["v"][:, 0]
    g = lmp.compute_global("vxa")[0]
    w, bound = gm.reduce("ave", vx, want), gm.gate("ave", vx, want)
    print("reduce ave vx over %d atoms: %.17g, model %.17g, |diff| %.2e, bound %.2e" % (want.sum(), g, w, abs(g - w), bound))
    assert abs(g - w) <= bound
    # contacts() takes the group as it stands
    rows = lmp.contacts("up")
    members = set(li["tag"][want].tolist())
    assert len(rows["tag1"]) > 0 and set(rows["tag1"].tolist()) <= members and set(rows["tag2"].tolist()) <= members
    lmp.close()


def _end_state(lmp):
    st = lmp.get_state()
    nb, fl = lmp.neighbors()
    o = np.lexsort((nb[:, 4], nb[:, 3], nb[:, 2], nb[:, 1], nb[:, 0]))
    return st, nb[o], fl[o]


def test_regions_and_dynamic_groups_are_passive(tmp_path):
    """the same bed with a region, a region group and two dynamic groups (every 1), and without any of them: the same bits
    of x, v, omega and of the neighbour list.  Both engines keep a dump of `id x y z` at every step, as the passivity tests
    of the other output sections do: a dynamic group with every 1 ends a piece of the run at every step, and a piece ends with
    the second half-kick of its last step and begins with the first of the next, each rounded on its own -- an engine that
    is never cut rounds them together, with or without this feature"""
    bed = _flow_bed()
    up = _above(bed)
    ends = []
    for k, extra in enumerate(([], [rm.command("up", up), "group up dynamic all region up every 1", "group s region up",
                                    "group up2 dynamic two region up"])):
        lmp = _flow_engine(bed, ["dump u all custom 1 %s id x y z" % (tmp_path / ("u%d.dump" % k))] + extra)
        lmp.command("run 150")
        lmp.step(150)
        ends.append(_end_state(lmp))
        if extra:
            assert lmp.region_launches() == 1 + 1 + 150 + 150      # group s; the setup of the run; every step
        else:
            assert lmp.region_launches() == 0
        assert lmp.info().nbuilds > 1
        lmp.sync()
        lmp.close()
    assert (tmp_path / "u0.dump").read_bytes() == (tmp_path / "u1.dump").read_bytes()
    (a, na, fa), (b, nb, fb) = ends
    for k in ("x", "v", "omega", "tag"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert na.tobytes() == nb.tobytes() and fa.tobytes() == fb.tobytes()


def test_masks_survive_reordering_deletion_and_creation():
    bed = _flow_bed()
    up = _above(bed)
    lmp = _flow_engine(bed, [rm.command("up", up), "group s region up", "group up dynamic all region up every 5"])
    li0 = lmp.get_local_info()
    static = dict(zip(li0["tag"].tolist(), rm.match(up, li0["x"]).tolist()))
    assert 0 < sum(static.values()) < N_FLOW
    builds = lmp.info().nbuilds
    lmp.command("run 400")
    li = lmp.get_local_info()
    assert lmp.info().nbuilds > builds + 1                                                    # the list was rebuilt
    _check_group(lmp, "s", np.array([static[t] for t in li["tag"].tolist()]), "the static group follows the tags")
    _check_group(lmp, "up", rm.match(up, li["x"]), "step 400")
    # a member goes, an atom comes inside the region: the next update has both
    member = int(li["tag"][rm.match(up, li["x"])][0])
    lmp.delete_particle([member])
    top = float(li["x"][:, 2].max())
    d = float(bed["diameter"][0])
    pos = [0.5 * float(bed["boxhi"][0]), 0.5 * float(bed["boxhi"][1]), top + 2.0 * d]
    assert pos[2] + d < float(bed["boxhi"][2])
    lmp.create_particle(pos, [N_FLOW + 1], d, 2650.0, 1, [0.0, 0.0, 0.0])
    lmp.command("run 5")
    li = lmp.get_local_info()
    want = rm.match(up, li["x"])
    assert len(li["tag"]) == N_FLOW and member not in li["tag"].tolist() and want[li["tag"] == N_FLOW + 1].all()
    _check_group(lmp, "up", want, "after delete and create")
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. restart

def test_restart_keeps_the_mask_and_a_dynamic_group_comes_back_static(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    lo, hi = np.asarray(bed["boxlo"], float), np.asarray(bed["boxhi"], float)
    left = ("block", -BIG, 0.5 * (lo[0] + hi[0]), -BIG, BIG, -BIG, BIG, "in")
    low = ("block", -BIG, BIG, -BIG, 0.5 * (lo[1] + 0.6 * hi[1]), -BIG, BIG, "in")
    _define(lmp, "left", left)
    _define(lmp, "low", low)
    lmp.command("group s region left")
    lmp.command("group d dynamic all region low every 3")
    lmp.command("run 10")
    F = str(tmp_path / "F.sfr")
    lmp.write_restart(F)
    li = lmp.get_local_info()
    ms, md = lmp.group_mask("s"), lmp.group_mask("d")
    assert 0 < ms.sum() < len(ms) and 0 < md.sum() < len(md)
    lmp.close()
    state = restart.read(F)                                   # the file format is unchanged: restart.py reads it as before
    assert restart.header(F)["step"] == 10 and len(state["tag"]) == len(li["tag"])
    names = [g[0] if isinstance(g, (tuple, list)) else g for g in restart.header(F)["groups"]]
    assert "s" in names and "d" in names
    R = Lammps()
    R.read_restart(F)
    lr = R.get_local_info()
    by_s, by_d = dict(zip(li["tag"].tolist(), ms.tolist())), dict(zip(li["tag"].tolist(), md.tolist()))
    assert R.group_mask("s").tolist() == [by_s[t] for t in lr["tag"].tolist()]
    assert R.group_mask("d").tolist() == [by_d[t] for t in lr["tag"].tolist()]
    assert R.group_count("d") == int(md.sum()) and R.region_launches() == 0
    with pytest.raises(SfError, match="is not a dynamic group"):
        R.region_cost("d")
    with pytest.raises(SfError, match="Group region ID does not exist"):      # regions are not stored
        R.command("group d region low")
    R.command("group d type 1")                                # a static group again: the other styles work on it
    assert R.group_mask("d").all()
    R.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals

BOX = "region b block 0 1 0 1 0 1 units box"


def _nine(lmp):
    for k in range(8):
        lmp.command("group d%d dynamic all region b" % k)


@pytest.mark.parametrize("before,line,msg", [
    ([], "region r block 0 1 0 1 0 1", "give units box"),
    ([], "region r block 0 1 0 1 0 1 units lattice", "units lattice is not supported"),
    ([], "region r prism 0 1 0 1 0 1 0 0 0 units box", "region style prism is not supported"),
    ([], "region r block 0 1 0 1 0 1 move v_x NULL NULL units box", "region keyword move is not supported"),
    ([], "region r block 0 1 0 1 0 1 open 1 units box", "region keyword open is not supported"),
    ([BOX], "region u union 2 b nosuch units box", "Region union region ID does not exist"),
    ([BOX], "region i intersect 2 nosuch b units box", "Region intersect region ID does not exist"),
    ([BOX], BOX, "Reuse of region ID"),
    ([BOX, "group g dynamic all region b"], "region b delete", "a dynamic group uses it"),
    ([BOX, "region s sphere 0 0 0 1 units box", "region u union 2 b s units box"], "region s delete",
     "is a union or intersect of it"),
    ([], "region nosuch delete", "Delete region ID does not exist"),
    ([], "region r block 1 0 0 1 0 1 units box", "Illegal region block command"),
    ([], "region r plane 0 0 0 0 0 0 units box", "Illegal region plane command"),
    ([], "group g region nosuch", "Group region ID does not exist"),
    ([], "group g dynamic all region nosuch", "Group region ID does not exist"),
    ([BOX, "group p dynamic all region b"], "group g dynamic p region b", "parent group cannot be dynamic"),
    ([BOX], "group g dynamic g region b", "Group dynamic cannot reference itself"),
    ([BOX, "group p type 1", "group g dynamic p region b"], "group p dynamic all region b", "a parent group cannot be dynamic"),
    ([BOX], "group g dynamic nosuch region b", "Group dynamic parent group does not exist"),
    ([BOX], "group g dynamic all region b every 0", "Illegal group command"),
    ([BOX], "group g dynamic all var v", "keyword var is not supported"),
    ([BOX], "group g dynamic all property p", "keyword property is not supported"),
    ([BOX, "group g dynamic all region b"], "fix 9 g gravity 9.81 vector 0 -1 0", "dynamic group"),
    ([BOX, "group g dynamic all region b"], "fix 9 g nve/sphere", "dynamic group"),
    ([BOX, "group g dynamic all region b"], "fix 9 g freeze", "dynamic group"),
    ([BOX, "group g dynamic all region b"], "fix 9 g rigid/nve single", "dynamic group"),
    ([BOX, "group g dynamic all region b"], "fix 9 all rigid/nve group 1 g", "dynamic group"),
    ([BOX, "group g type 1", "fix 9 g gravity 9.81 vector 0 -1 0"], "group g dynamic all region b", "its group bit is decided"),
    ([BOX, "group g dynamic all region b"], "group g type 1", "is a dynamic group"),
    ([BOX, "group g dynamic all region b"], "group g union all", "is a dynamic group"),
    ([BOX, "group g dynamic all region b"], "group g region b", "is a dynamic group"),
    ([BOX, _nine], "group d8 dynamic all region b", "Too many dynamic groups"),
    ([BOX, _decompose], "group g dynamic all region b", "group dynamic: one rank only"),
])
def test_refusals(before, line, msg):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    for b in before:
        if callable(b):
            b(lmp)
        else:
            lmp.command(b)
    with pytest.raises(SfError, match=msg):
        lmp.command(line)
    if _decompose not in before:
        lmp.command("run 0")   # the engine stays usable
    lmp.close()


def test_read_restart_is_refused_while_a_dynamic_group_exists(tmp_path):
    bed, cfg = _small()
    lmp = dc.make_hip(bed, cfg)
    F = str(tmp_path / "F.sfr")
    lmp.write_restart(F)
    lmp.close()
    R = Lammps()
    R.command("region b block 0 1 0 1 0 1 units box")            # (numbers only: no box is needed)
    R.command("group g dynamic all region b")
    with pytest.raises(SfError, match="Cannot read_restart while a dynamic group is defined"):
        R.read_restart(F)
    R.command("group g static")
    R.read_restart(F)
    assert R.get_local_n() == len(bed["x"])
    R.close()


def test_inf_needs_a_box():
    lmp = Lammps()
    with pytest.raises(SfError, match="Cannot use region INF or EDGE when box does not exist"):
        lmp.command("region r block INF 1 0 1 0 1 units box")
    lmp.command("region r block 0 1 0 1 0 1 units box")
    lmp.close()
