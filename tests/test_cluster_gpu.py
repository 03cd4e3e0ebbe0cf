"""`compute cluster/atom CUT [surface no|yes] [size no|yes]` and `compute cluster/stats CID` on the GPU
against the NumPy statement of the rules (tests/cluster_model.py, itself held to hand-computed answers by
tests/test_cluster_model.py).

The model is fed the engine's own bits -- get_state(), the tags, the radii, the group masks, the box -- and every value is an
integer, so every comparison is ==."""
import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError
from tests import cluster_model as cm
from tests import dem_cases as dc
from tests import nbr_model as nm
from tests.test_compute_atom_gpu import _decompose
from tests.test_dump_gpu import frames
from tests.test_global_gpu import GROUPS
from tests.test_nbr_gpu import D, _bed, _cutoffs, _engine, _ncells

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 64   # the cap of the host's verify loop


def _state(lmp, bed, groups=GROUPS):
    """what the model is fed, sorted by tag like compute_atom(): positions, tags, radii, the group masks, the box, rsq"""
    st = lmp.get_state()
    tags = np.asarray(lmp.get_local_info()["tag"])
    order = np.argsort(tags, kind="stable")
    lo, hi, per = np.asarray(bed["boxlo"], np.float64), np.asarray(bed["boxhi"], np.float64), tuple(bed["periodic"])
    rad = lmp.compute_atom("rad")
    return dict(x=st["x"], tag=tags[order], rad=rad, masks={g: np.asarray(lmp.group_mask(g))[order].astype(bool) for g in groups},
                lo=lo, hi=hi, per=per, rsq=nm.pair_rsq(st["x"], lo, hi, per), rmax=float(np.asarray(bed["diameter"]).max()) / 2)


def _model(s, group, cut, surface=False):
    return cm.cluster_atom(s["x"], s["rad"], s["tag"], s["masks"][group], s["lo"], s["hi"], s["per"], cut, surface,
                           rmax=s["rmax"], rsq=s["rsq"])


def _same(lmp, cid, want):
    got = lmp.compute_atom(cid)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (cid, int((got != want).sum()))
    assert 1 <= lmp.cluster_rounds(cid) < MAX_ROUNDS or len(want) == 0


def _with_radius(lmp):
    lmp.command("compute rad all property/atom radius")
    return lmp


# ---------------------------------------------------------------------------------------------------------------------
# a. the beds of section 20 at three moments, every cutoff of _cutoffs, three groups, both link rules, with and without size

@pytest.mark.parametrize("n", [108, 257, 864, 1])
def test_every_bed_at_three_moments_equals_the_model(n):
    lmp, bed = _engine(n)
    _with_radius(lmp)
    cuts, L = _cutoffs(bed)
    rmax = float(np.asarray(bed["diameter"]).max()) / 2
    specs = []
    for name, rc in cuts.items():
        # surface yes: the gap whose grid has the same cutoff (2 rmax + CUT), or 0.03 D where that cutoff is below a diameter
        # (the smallest bed is 4.16 D long: more than three cells still)
        gap = rc - 2.0 * rmax if rc - 2.0 * rmax > 0.0 else 0.03 * D
        for surface, cut in ((False, rc), (True, gap)):
            cells = _ncells(L, cm.grid_cutoff(cut, surface, rmax))
            assert cells == _ncells(L, rc) or (name == "short" and cells > 3)   # > 3, 1, 2 (864: three_d), 3, 2 cells
            for gname in GROUPS:
                for size in (False, True):
                    cid = "cl_%s_%s_%d%d" % (name, gname, surface, size)
                    lmp.command("compute %s %s cluster/atom %.17g surface %s%s" % (cid, gname, cut, "yes" if surface else "no",
                                                                                  " size yes" if size else ""))
                    specs.append((cid, gname, cut, surface, size))
    assert _ncells(L, cuts["short"]) > 3 and [_ncells(L, cuts[k]) for k in ("under_half", "two", "third")] == [1, 2, 3]
    lmp.command("run 0")
    seen_outside, joined = False, 0
    for moment, steps in (("step 0", 0), ("25 steps", 25), ("outside", 15)):
        if steps:
            lmp.command("run %d" % steps)
        s = _state(lmp, bed)
        outside = bool((s["x"][:, 0] < s["lo"][0]).any())
        assert outside or moment != "outside"
        seen_outside = seen_outside or outside
        models = {}
        for cid, gname, cut, surface, size in specs:
            key = (gname, cut, surface)
            if key not in models:
                models[key] = _model(s, gname, cut, surface)
            want = models[key]
            _same(lmp, cid, want if size else want[:, 0].copy())
            joined += int((want[:, 1] > 1).sum())
        assert not models[("none", cuts["short"], False)].any()
    assert seen_outside and (n == 1 or joined > 0)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# b. hand-placed atoms: a serpentine chain that needs a link through a periodic face, the smallest tag in its middle

A = 2.0 ** -8      # the cutoff of the chain tests: a power of two, so that a spacing of exactly the cutoff can be built
S = 0.99 * A       # the spacing of the chain
NCHAIN, NLINE = 600, 41
LO, HI, PER = np.zeros(3), np.array([64 * A, 64 * A, 4 * A]), (1, 0, 0)


def _chain(exact_gap_after=None):
    """(x, tags, types) of 600 atoms on a serpentine path of spacing S -- rows of 48 along x, three spacings apart in y, joined
    at alternating ends by two atoms -- that starts at x = 40 A and so crosses the periodic face at 64 A in every row; then a
    straight line of 41 atoms far from it whose middle atom has type 2.  exact_gap_after = k: the path is cut behind its atom
    k, whose x becomes a multiple of A / 1024, and everything after it is moved along x so that atom k + 1 lies exactly A
    further: dx = A, dy = dz = 0 and rsq = A A with no rounding anywhere"""
    path, c, r, step = [], 0, 0, 1
    while len(path) < NCHAIN:
        path.append((c, 3 * r))
        if (step > 0 and c == 47) or (step < 0 and c == 0):
            path += [(c, 3 * r + 1), (c, 3 * r + 2)]
            r, step = r + 1, -step
        else:
            c += step
    path = np.array(path[:NCHAIN], dtype=np.float64)
    x = np.zeros((NCHAIN + NLINE, 3))
    x[:NCHAIN, 0] = 40 * A + S * path[:, 0]
    x[:NCHAIN, 1] = 2 * A + S * path[:, 1]
    if exact_gap_after is not None:
        k = exact_gap_after
        assert path[k, 1] == path[k + 1, 1] and path[k + 1, 0] == path[k, 0] + 1    # inside a row, going up in x
        xk = np.round(x[k, 0] * 1024 / A) * A / 1024
        shift = (xk + A) - x[k + 1, 0]
        x[k, 0] = xk
        x[k + 1:NCHAIN, 0] += shift
        x[k + 1, 0] = xk + A
        assert x[k + 1, 0] - x[k, 0] == A and x[k + 1, 1] == x[k, 1] and xk + A < 64 * A
    x[:NCHAIN, 0] = np.where(x[:NCHAIN, 0] >= 64 * A, x[:NCHAIN, 0] - 64 * A, x[:NCHAIN, 0])
    x[NCHAIN:, 0] = 4 * A + S * np.arange(NLINE)
    x[NCHAIN:, 1] = 50 * A
    x[:, 2] = 2 * A
    n = len(x)
    tags = 5 + 3 * np.random.default_rng(3).permutation(n)        # with gaps, in no order
    lowest = int(np.argmin(tags))
    tags[[lowest, NCHAIN // 2]] = tags[[NCHAIN // 2, lowest]]     # the smallest tag sits in the middle of the chain
    types = np.ones(n, np.int32)
    types[NCHAIN + NLINE // 2] = 2
    return x, tags.astype(np.int32), types


def _placed(x, tags, types):
    n = len(x)
    lmp = Lammps()
    lmp.set_box(LO, HI)
    lmp.create_atoms(x, np.full(n, 0.25 * A), np.full(n, 2650.0), v=np.zeros((n, 3)), type_=types, tag=tags)
    bed = dict(x=x, v=np.zeros((n, 3)), diameter=np.full(n, 0.25 * A), density=np.full(n, 2650.0), boxlo=LO, boxhi=HI,
               periodic=PER, type=types)
    cfg = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=0.0, dt=1.0e-6, skin=0.1 * A, walls=[])
    for line in dc.script_lines(bed, cfg):   # (nothing touches: the forces of `run 0` are zero)
        lmp.command(line)
    lmp.command("group one type 1")
    _with_radius(lmp)
    return lmp, bed


def _placed_state(lmp, bed, x, tags):
    s = _state(lmp, bed, groups=("all", "one"))
    order = np.argsort(tags, kind="stable")
    assert s["x"].tobytes() == x[order].tobytes() and s["tag"].tolist() == tags[order].tolist()
    return s, order


def test_a_serpentine_chain_through_a_periodic_face_is_one_cluster():
    x, tags, types = _chain()
    lmp, bed = _placed(x, tags, types)
    lmp.command("compute cl all cluster/atom %.17g size yes" % A)
    lmp.command("compute c1 one cluster/atom %.17g size yes" % A)
    lmp.command("compute st all cluster/stats cl")
    lmp.command("compute s1 one cluster/stats c1")
    lmp.command("run 0")
    s, order = _placed_state(lmp, bed, x, tags)
    chain = np.isin(s["tag"], tags[:NCHAIN])
    assert tags[NCHAIN // 2] == tags.min() and (x[:NCHAIN, 0] < 8 * A).any() and (x[:NCHAIN, 0] > 60 * A).any()
    want = _model(s, "all", A)
    # by hand: the chain is one cluster under the smallest tag of all, the line another
    assert (want[chain] == [tags.min(), NCHAIN]).all() and (want[~chain] == [tags[NCHAIN:].min(), NLINE]).all()
    _same(lmp, "cl", want)
    assert lmp.compute_global("st").tolist() == [2.0, float(NCHAIN), float(NCHAIN + NLINE)]
    # the two halves of the line meet only through the atom of type 2, which is not in group `one`: three clusters
    w1 = _model(s, "one", A)
    line = s["tag"][~chain]
    mid = tags[NCHAIN + NLINE // 2]
    left, right = tags[NCHAIN:NCHAIN + NLINE // 2], tags[NCHAIN + NLINE // 2 + 1:]
    assert w1[s["tag"] == mid].tolist() == [[0.0, 0.0]]
    assert (w1[np.isin(s["tag"], left)] == [left.min(), NLINE // 2]).all()
    assert (w1[np.isin(s["tag"], right)] == [right.min(), NLINE // 2]).all() and len(line) == NLINE
    _same(lmp, "c1", w1)
    assert lmp.compute_global("s1").tolist() == [3.0, float(NCHAIN), float(NCHAIN + NLINE - 1)]
    assert lmp.compute_global("s1").tolist() == cm.cluster_stats(w1[:, 0], s["masks"]["one"]).tolist()
    lmp.close()


def test_one_spacing_of_exactly_the_cutoff_parts_the_chain():
    k = 2 * 50 + 20   # a row is 48 atoms and 2 joining ones; the third row runs up in x: its atom 20 and the next
    x, tags, types = _chain(exact_gap_after=k)
    lmp, bed = _placed(x, tags, types)
    lmp.command("compute cl all cluster/atom %.17g size yes" % A)
    lmp.command("compute st all cluster/stats cl")
    lmp.command("run 0")
    s, order = _placed_state(lmp, bed, x, tags)
    i, j = int(np.nonzero(s["tag"] == tags[k])[0][0]), int(np.nonzero(s["tag"] == tags[k + 1])[0][0])
    assert s["rsq"][i, j] == A * A and s["rsq"][j, i] == A * A
    want = _model(s, "all", A)
    head, tail = np.isin(s["tag"], tags[:k + 1]), np.isin(s["tag"], tags[k + 1:NCHAIN])
    assert (want[head] == [tags[:k + 1].min(), k + 1]).all() and (want[tail] == [tags[k + 1:NCHAIN].min(), NCHAIN - k - 1]).all()
    _same(lmp, "cl", want)
    assert lmp.compute_global("st").tolist() == [3.0, float(NCHAIN - k - 1), float(NCHAIN + NLINE)]
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# c. tags with gaps: atoms deleted and one created

def test_deleted_and_created_atoms_ids_are_tags_and_sizes_shrink():
    lmp, bed = _engine(108)
    _with_radius(lmp)
    cut = 1.05 * D
    lmp.command("compute cl all cluster/atom %.17g size yes" % cut)
    lmp.command("compute st all cluster/stats cl")
    lmp.command("run 0")
    s0 = _state(lmp, bed)
    w0 = _model(s0, "all", cut)
    _same(lmp, "cl", w0)
    assert w0[:, 1].max() > 50
    gone = [1, 5, 17, 60]    # (tag 1 among them: the smallest tag of its cluster goes)
    lmp.delete_particle(gone)
    top = float(np.asarray(bed["x"])[:, 1].max())
    new = 108 + 7
    lmp.create_particle(np.array([[1.0e-3, top + 3.0e-3, 1.0e-3]]), [new], 1.0e-3, 2650.0, 1, [0.0, 0.0, 0.0])
    s1 = _state(lmp, bed)
    assert s1["tag"].tolist() == sorted((set(range(1, 109)) - set(gone)) | {new})
    w1 = _model(s1, "all", cut)
    _same(lmp, "cl", w1)
    assert set(w1[:, 0].astype(int)) <= set(s1["tag"].tolist()) and 1 not in w1[:, 0]
    assert w1[s1["tag"] == new].tolist() == [[float(new), 1.0]]                   # alone, above the bed, under its own tag
    assert w1[:, 1].max() < w0[:, 1].max()
    st = lmp.compute_global("st")
    assert st.tolist() == cm.cluster_stats(w1[:, 0], s1["masks"]["all"]).tolist() and st[2] == 105.0
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. surface yes on a bed of two radii

def _two_radii():
    bed, cfg = _bed(108)
    d = np.array(bed["diameter"], dtype=np.float64)
    d[np.arange(len(d)) % 3 != 0] = 0.8 * D     # two grains of three are smaller: they touch nothing any more
    bed["diameter"] = d
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    lmp.command("group none type 3")
    return _with_radius(lmp), bed


def test_surface_yes_on_two_radii_differs_from_the_centre_rule_and_equals_the_model():
    lmp, bed = _two_radii()
    gap = 0.05 * D
    rmax = 0.5 * D
    centre = 2.0 * rmax + gap
    lmp.command("compute sf all cluster/atom %.17g surface yes size yes" % gap)
    lmp.command("compute ce all cluster/atom %.17g size yes" % centre)
    lmp.command("run 0")
    s = _state(lmp, bed)
    assert s["rmax"] == rmax and sorted(set(s["rad"].tolist())) == [0.4 * D, 0.5 * D]
    a_sf = cm.links(s["x"], s["rad"], s["masks"]["all"], s["lo"], s["hi"], s["per"], gap, True, s["rsq"])
    a_ce = cm.links(s["x"], s["rad"], s["masks"]["all"], s["lo"], s["hi"], s["per"], centre, False, s["rsq"])
    assert (a_ce & ~a_sf).any() and not (a_sf & ~a_ce).any()      # the model says so first: pairs the centre rule alone links
    w_sf, w_ce = _model(s, "all", gap, True), _model(s, "all", centre)
    assert (w_sf != w_ce).any() and w_sf[:, 1].max() < w_ce[:, 1].max()
    _same(lmp, "sf", w_sf)
    _same(lmp, "ce", w_ce)
    lmp.close()


def test_the_periodic_length_refusal_fires_at_two_rmax_plus_cut():
    lmp, bed = _two_radii()
    L = float(bed["boxhi"][0]) - float(bed["boxlo"][0])
    rmax = 0.5 * D
    under, over = 0.5 * L * (1.0 - 1.0e-9) - 2.0 * rmax, 0.5 * L * (1.0 + 1.0e-9) - 2.0 * rmax
    lmp.command("compute ok all cluster/atom %.17g surface yes" % under)
    lmp.command("compute no all cluster/atom %.17g surface yes" % over)
    lmp.command("compute centre all cluster/atom %.17g" % over)      # the same number as a centre cutoff is well inside
    lmp.command("run 0")
    s = _state(lmp, bed)
    _same(lmp, "ok", _model(s, "all", under, True)[:, 0].copy())
    _same(lmp, "centre", _model(s, "all", over)[:, 0].copy())
    with pytest.raises(SfError, match="compute cluster/atom: cutoff is longer than half a periodic box length"):
        lmp.compute_atom("no")
    with pytest.raises(ValueError):
        _model(s, "all", over, True)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. the consumers of a per-atom compute and of a global vector

def test_dump_reduce_ave_histo_ave_time_and_thermo_read_the_values(tmp_path):
    lmp, bed = _engine(108)
    _with_radius(lmp)
    cut = 1.05 * D
    path = tmp_path / "cl.dump"
    for line in ("log %s" % (tmp_path / "log.lammps"), "compute cl two cluster/atom %.17g" % cut, "compute cl2 two cluster/atom %.17g size yes" % cut,
                 "compute st all cluster/stats cl2", "compute mx all reduce max c_cl2[2]",
                 "fix hh all ave/histo 5 1 5 0.5 40.5 40 c_cl2[2] mode vector",
                 "fix t all ave/time 5 1 5 c_st[1] c_st[2] c_st[3]",
                 "thermo_style custom step c_st[1] c_st[3]", "thermo 5",
                 "dump d all custom 5 %s id c_cl c_cl2[2]" % path, "dump_modify d sort id"):
        lmp.command(line)
    lmp.command("run 0")
    for step in (5, 10, 15):
        lmp.command("run 5")
        s = _state(lmp, bed)
        want = _model(s, "two", cut)
        stats = cm.cluster_stats(want[:, 0], s["masks"]["all"])
        assert 1 < stats[0] < stats[2] and stats[1] > 1                         # several clusters, one of them of several grains
        out = lmp.ave_time("t")
        assert out["step"] == step and out["values"].tolist() == stats.tolist()   # fix ave/time, at each sample
        assert lmp.get_thermo("c_st[1]") == stats[0] and lmp.get_thermo("c_st[3]") == stats[2]   # thermo
    _same(lmp, "cl", want[:, 0].copy())
    _same(lmp, "cl2", want)
    assert lmp.compute_global("st").tolist() == stats.tolist()
    assert lmp.compute_global("mx").tolist() == [stats[1]] == [want[:, 1].max()]    # compute reduce max
    h = lmp.ave_histo("hh")                                                        # fix ave/histo
    assert h["step"] == 15 and np.asarray(h["count"]).tolist() == \
        np.histogram(want[:, 1], bins=40, range=(0.5, 40.5))[0].astype(float).tolist()
    lmp.sync()
    fr = frames(str(path))                                                         # dump custom
    assert [f[0] for f in fr] == [0, 5, 10, 15]
    rows = [r.split(b" ") for r in fr[-1][3]]
    assert [float(r[1]) for r in rows] == want[:, 0].tolist() and [float(r[2]) for r in rows] == want[:, 1].tolist()
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# f. passive, shared, and launched once per step

def _forty_steps(extras):
    bed, cfg = _bed(108)
    lmp = dc.make_hip(bed, cfg)
    if extras:
        lmp.command("group two type 2")
        lmp.command("compute cl all cluster/atom %.17g size yes" % (1.05 * D))
        lmp.command("compute sf two cluster/atom %.17g surface yes" % (0.05 * D))
        lmp.command("compute st all cluster/stats cl")
    for _ in range(4):
        lmp.command("run 10")
        if extras:
            lmp.compute_atom("cl"), lmp.compute_atom("sf"), lmp.compute_global("st")
    lmp.sync()
    st, hist = lmp.get_state(), lmp.history()
    lmp.close()
    return st, hist


def test_the_run_goes_on_with_the_same_bits():
    plain, watched = _forty_steps(False), _forty_steps(True)
    for k in ("x", "v", "omega", "f", "torque"):
        assert plain[0][k].tobytes() == watched[0][k].tobytes(), k
    assert sorted(plain[1]) == sorted(watched[1]) and all(plain[1][p].tobytes() == watched[1][p].tobytes() for p in plain[1])


def test_one_grid_with_coord_atom_and_nothing_launched_twice_at_one_step():
    lmp, bed = _engine(108)
    cut = 1.3 * D
    lmp.command("compute c all coord/atom cutoff %.17g" % cut)
    lmp.command("compute cl all cluster/atom %.17g size yes" % cut)
    lmp.command("compute st all cluster/stats cl")
    lmp.command("run 10")
    assert lmp.nbr_launches() == dict(grid_builds=0, launches=0, host_copies=0), "nothing is launched without a consumer"
    lmp.compute_atom("c")
    one = lmp.nbr_launches()
    first = lmp.compute_atom("cl")
    two = lmp.nbr_launches()
    rounds = lmp.cluster_rounds("cl")
    assert one["grid_builds"] == two["grid_builds"] == 1                       # the same cutoff at the same step: the same grid
    assert 1 <= rounds < MAX_ROUNDS
    assert two["launches"] - one["launches"] == 4 + 2 * rounds and two["host_copies"] - one["host_copies"] == rounds
    g0 = lmp.global_launches()["launches"]
    lmp.compute_global("st")
    g1 = lmp.global_launches()["launches"]
    assert g1 - g0 == 2
    again = lmp.compute_atom("cl")                                             # a second query at the same step
    lmp.compute_global("st")
    assert lmp.nbr_launches() == two and lmp.global_launches()["launches"] == g1 and again.tobytes() == first.tobytes()
    assert lmp.cluster_rounds("cl") == rounds
    g, w = lmp.nbr_cost("cl")
    assert g > 0.0 and w > 0.0
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# g. refusals

ILLEGAL = "Illegal compute cluster/atom command"
REFUSALS = [
    ("compute x all cluster/atom", ILLEGAL),
    ("compute x all cluster/atom cutoff 1e-3", ILLEGAL),
    ("compute x all cluster/atom 0", ILLEGAL),
    ("compute x all cluster/atom -1e-3", ILLEGAL),
    ("compute x all cluster/atom -1e-3 surface yes", ILLEGAL),
    ("compute x all cluster/atom nan", ILLEGAL),
    ("compute x all cluster/atom inf surface yes", ILLEGAL),
    ("compute x all cluster/atom 1e-3 surface", ILLEGAL),
    ("compute x all cluster/atom 1e-3 surface maybe", ILLEGAL),
    ("compute x all cluster/atom 1e-3 size 2", ILLEGAL),
    ("compute x all cluster/atom 1e-3 extra yes", ILLEGAL),
    ("compute x all cluster/atom 1e-3 1e-3", ILLEGAL),
    ("compute x nobody cluster/atom 1e-3", "nobody"),
    ("compute cl all cluster/atom 1e-3", "Reuse of compute ID"),
    ("compute x all fragment/atom", "compute fragment/atom is not supported (there are no bonds; cluster/atom is)"),
    ("compute x all aggregate/atom 1e-3", "compute aggregate/atom is not supported (there are no bonds; cluster/atom is)"),
    ("compute x all cluster/stats", "Illegal compute cluster/stats command"),
    ("compute x all cluster/stats cl extra", "Illegal compute cluster/stats command"),
    ("compute x all cluster/stats c_cl", "give the ID of the cluster/atom compute itself (cl, not c_cl)"),
    ("compute x all cluster/stats nope", "compute cluster/stats: Could not find compute ID nope"),
    ("compute x all cluster/stats c", "compute cluster/stats: compute c is not a compute cluster/atom"),
    ("compute x all cluster/stats r", "compute cluster/stats: compute r is not a compute cluster/atom"),
    ("compute x all cluster/stats st", "compute cluster/stats: compute st is not a compute cluster/atom"),
    ("compute x all reduce sum c_cl[1]", "Compute reduce compute does not calculate a per-atom array"),
    ("compute x all reduce sum c_cl2", "Compute reduce compute does not calculate a per-atom vector"),
    ("compute x all reduce sum c_cl2[3]", "Compute reduce compute array is accessed out-of-range"),
    ("compute x all reduce sum c_st[1]", "Compute reduce compute calculates global values"),
    ("thermo_style custom step c_st", "Thermo compute does not compute scalar"),
    ("thermo_style custom step c_st[4]", "Thermo compute vector is accessed out-of-range"),
    ("fix x all ave/time 2 3 10 c_st", "Fix ave/time compute does not calculate a scalar"),
    ("fix x all ave/time 2 3 10 c_cl", "Fix ave/time compute does not calculate a scalar"),
]


def test_every_refusal_by_message():
    lmp, bed = _engine(108)
    for line in ("compute cl all cluster/atom 1.05e-3", "compute cl2 all cluster/atom 1.05e-3 size yes",
                 "compute c all coord/atom cutoff 1.3e-3", "compute r all reduce sum vx", "compute st all cluster/stats cl"):
        lmp.command(line)
    for line, msg in REFUSALS:
        with pytest.raises(SfError) as err:
            lmp.command(line)
        assert msg in str(err.value), (line, str(err.value))
    for query, msg in ((lambda: lmp.cluster_rounds("c"), "Could not find compute cluster/atom ID c"),
                       (lambda: lmp.cluster_rounds("nope"), "Could not find compute cluster/atom ID nope"),
                       (lambda: lmp.compute_global("cl"), "does not calculate a global scalar or vector"),
                       (lambda: lmp.compute_atom("st"), "does not calculate per-atom values")):
        with pytest.raises(SfError) as err:
            query()
        assert msg in str(err.value), str(err.value)
    # what was refused left nothing behind
    lmp.command("run 0")
    assert lmp.cluster_rounds("cl") == 0
    ids = lmp.compute_atom("cl")
    assert lmp.compute_global("st")[2] == 108.0 and lmp.cluster_rounds("cl") >= 1
    # a cluster compute that a stats compute still names goes; the stats compute refuses at its next evaluation, and works
    # again once the ID names a cluster/atom compute again
    lmp.command("uncompute cl")
    with pytest.raises(SfError, match="compute cluster/stats: Could not find compute ID cl"):
        lmp.compute_global("st")
    lmp.command("compute cl all ke/atom")
    with pytest.raises(SfError, match="compute cluster/stats: compute cl is not a compute cluster/atom"):
        lmp.compute_global("st")
    lmp.command("uncompute cl")
    lmp.command("compute cl two cluster/atom 1.05e-3")
    assert lmp.compute_global("st")[2] == float((np.asarray(bed["type"]) == 2).sum()) and len(ids) == 108
    lmp.close()


@pytest.mark.parametrize("line,msg", [
    ("compute x all cluster/atom 1.05e-3", "compute cluster/atom: one rank only"),
    ("compute x all cluster/stats cl", "compute cluster/stats: one rank only"),
])
def test_a_decomposed_handle_is_refused_at_each_command_and_at_evaluation(line, msg):
    lmp, bed = _engine(108)
    lmp.command("compute cl all cluster/atom 1.05e-3")
    lmp.command("compute st all cluster/stats cl")
    _decompose(lmp)
    with pytest.raises(SfError, match=msg):
        lmp.command(line)
    with pytest.raises(SfError, match="compute cluster/atom: one rank only"):
        lmp.compute_atom("cl")
    with pytest.raises(SfError, match="compute cluster/stats: one rank only"):
        lmp.compute_global("st")
    with pytest.raises(SfError, match="compute cluster/atom: one rank only"):
        lmp.nbr_cost("cl")
    lmp.close()
