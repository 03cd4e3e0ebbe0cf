"""`compute rdf ... cutoff Rc`, `compute coord/atom cutoff Rc` and `fix ave/time ... mode vector` on the
GPU against the NumPy statement of the rules (tests/nbr_model.py, itself held to hand-computed answers by
tests/test_nbr_model.py).

The model is fed the engine's own bits -- get_state(), the box, the periodic flags, the group masks -- and every quantity is an
integer count or a fixed sequence of IEEE operations on integer counts, so every comparison is ==."""
import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError
from tests import dem_cases as dc
from tests import global_model as gm
from tests import nbr_model as nm
from tests.test_compute_atom_gpu import _decompose
from tests.test_contacts_gpu import _small
from tests.test_dump_gpu import frames
from tests.test_global_gpu import GROUPS, _groups, _masks, _sized, _third

pytestmark = pytest.mark.gpu

D = 1.0e-3   # the grain diameter of the beds


# ---------------------------------------------------------------------------------------------------------------------
# the beds: the lattice is moved along x (a periodic dimension) so that its first plane lies 5 um inside the face, and the
# lowest-x atom flies outwards: it is outside the box within a few steps, long before half a skin makes a rebuild wrap it

def _shifted(bed):
    x = np.array(bed["x"], dtype=np.float64)
    x[:, 0] -= x[:, 0].min() - 5.0e-6
    assert x[:, 0].max() < float(bed["boxhi"][0])
    v = np.array(bed["v"], dtype=np.float64)
    v[np.argmin(x[:, 0])] = (-1.0, 0.0, 0.0)
    bed["x"], bed["v"] = x, v
    return bed


def _bed(n):
    if n == 108:
        bed, cfg = _small("hertz", types=_third)
    else:
        bed, cfg = _sized(n)
    return _shifted(bed), cfg


def _engine(n):
    bed, cfg = _bed(n)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    lmp.command("compute ty all property/atom type")
    return lmp, bed


def _inputs(lmp, bed):
    """what the model is fed: positions and types sorted by tag, the group masks, the box"""
    st = lmp.get_state()
    order = np.argsort(lmp.get_local_info()["tag"], kind="stable")
    types = lmp.compute_atom("ty").astype(np.int64)
    assert types.tolist() == np.asarray(bed["type"]).tolist()
    masks = {g: lmp.group_mask(g)[order] for g in GROUPS}
    want = _masks(bed)
    assert all(masks[g].tolist() == want[g].tolist() for g in GROUPS)
    lo, hi, per = np.asarray(bed["boxlo"], np.float64), np.asarray(bed["boxhi"], np.float64), tuple(bed["periodic"])
    return dict(x=st["x"], t=types, masks=masks, lo=lo, hi=hi, per=per, rsq=nm.pair_rsq(st["x"], lo, hi, per))


def _rdf_model(inp, group, nbin, rc, pairs):
    c = nm.rdf_counts(inp["x"], inp["t"], inp["masks"][group], inp["lo"], inp["hi"], inp["per"], nbin, rc, pairs, rsq=inp["rsq"])
    return c, nm.rdf_array(c, inp["lo"], inp["hi"], nbin, rc)


def _check_rdf(lmp, inp, cid, group, nbin, rc, pairs):
    c, arr = _rdf_model(inp, group, nbin, rc, pairs)
    got = lmp.rdf_counts(cid)
    for k in ("counts", "icount", "jcount", "duplicates"):
        assert got[k].tolist() == c[k].tolist(), (cid, k)
    a = lmp.compute_array(cid)
    assert a.shape == arr.shape and a.tobytes() == arr.tobytes(), (cid, np.abs(a - arr).max())
    return c


def _check_coord(lmp, inp, cid, group, rc, ranges):
    want = nm.coord_atom(inp["x"], inp["t"], inp["masks"][group], inp["lo"], inp["hi"], inp["per"], rc, ranges, rsq=inp["rsq"])
    got = lmp.compute_atom(cid)
    want = want if len(ranges) > 1 else want[:, 0]
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), cid
    return want


PAIR_SETS = {"none": (), "three": (("1", "1"), ("1", "2"), ("2", "2")), "star": (("*", "*"),), "range": (("1*2", "2"),)}


def _pair_words(pairs):
    return " ".join("%s %s" % p for p in pairs)


def _cutoffs(bed):
    """({name: Rc}, L): cutoffs that give more than three, one, two and three cells in x, a periodic dimension of length L"""
    L = float(bed["boxhi"][0]) - float(bed["boxlo"][0])
    out = {"short": 0.9 * D, "under_half": 0.5 * L * (1.0 - 1.0e-9)}
    if 3.0 * D <= 0.5 * L:
        out["three_d"] = 3.0 * D
    out["third"] = L / 3.2      # three cells
    out["two"] = L / 2.4        # two cells
    return out, L


def _ncells(L, rc):
    return max(1, int(np.floor(L / (rc * (1.0 + 2.0 ** -20)))))


@pytest.mark.parametrize("n", [108, 257, 864, 1])
def test_every_bed_at_three_moments_equals_the_model(n):
    lmp, bed = _engine(n)
    cuts, L = _cutoffs(bed)
    cells = {name: _ncells(L, rc) for name, rc in cuts.items()}
    assert cells["short"] > 3 and cells["under_half"] == 1 and cells["third"] == 3 and cells["two"] == 2
    if n == 864:
        assert cells["three_d"] == 2   # three diameters on the 864-grain bed: two cells, each of more atoms than a block has lanes
    specs = []
    for name, rc in cuts.items():
        for gname, nbin, pkey in (("all", 100, "none"), ("two", 7, "three"), ("all", 1, "star"), ("none", 7, "range"),
                                  ("all", 7, "range")):
            cid = "g_%s_%s_%d_%s" % (name, gname, nbin, pkey)
            lmp.command("compute %s %s rdf %d %s cutoff %.17g" % (cid, gname, nbin, _pair_words(PAIR_SETS[pkey]), rc))
            specs.append((cid, gname, nbin, rc, PAIR_SETS[pkey] or (("*", "*"),)))
        for gname, ranges in (("all", ()), ("two", ("1",)), ("all", ("1", "2", "1*2")), ("none", ("*",))):
            cid = "c_%s_%s_%d" % (name, gname, len(ranges))
            lmp.command("compute %s %s coord/atom cutoff %.17g %s" % (cid, gname, rc, " ".join(ranges)))
            specs.append((cid, gname, None, rc, ranges or ("*",)))
    lmp.command("run 0")
    seen_outside = False
    for moment, steps in (("step 0", 0), ("25 steps", 25), ("outside", 15)):
        if steps:
            lmp.command("run %d" % steps)
        inp = _inputs(lmp, bed)
        outside = bool((inp["x"][:, 0] < inp["lo"][0]).any())
        if moment == "outside":
            assert outside, "no atom lies outside the box: x min %.6g" % inp["x"][:, 0].min()
        seen_outside = seen_outside or outside
        total = 0
        for cid, gname, nbin, rc, what in specs:
            if nbin is None:
                _check_coord(lmp, inp, cid, gname, rc, what)
            else:
                c = _check_rdf(lmp, inp, cid, gname, nbin, rc, what)
                total += int(c["counts"].sum())
                if "short" in cid and gname == "all" and nbin == 100 and n > 1:
                    # a cutoff shorter than the diameter: the leading bins are empty (the grains overlap by 2 % at most)
                    assert c["counts"][0, :80].sum() == 0
        assert n == 1 or total > 0
    assert seen_outside
    lmp.close()


def test_a_cutoff_over_half_a_periodic_length_is_refused_at_evaluation():
    lmp, bed = _engine(108)
    L = float(bed["boxhi"][0]) - float(bed["boxlo"][0])
    over = 0.5 * L * (1.0 + 1.0e-9)
    lmp.command("compute g all rdf 10 cutoff %.17g" % over)
    lmp.command("compute c all coord/atom cutoff %.17g" % over)
    lmp.command("run 0")
    for query in (lambda: lmp.compute_array("g"), lambda: lmp.rdf_counts("g"), lambda: lmp.compute_atom("c")):
        with pytest.raises(SfError, match="cutoff is longer than half a periodic box length"):
            query()
    lmp.close()


def test_a_lattice_with_pairs_at_exactly_the_cutoff_and_at_bin_edges():
    """a simple cubic lattice of spacing 2^-8 filled through create_atoms, radii small enough that nothing touches; Rc = two
    spacings, Nbin = 8: the distances 1 and 2 spacings fall exactly on bin edges (bins 4 and 8), and the pairs at exactly Rc
    are in neither style"""
    a = 2.0 ** -8
    k = np.arange(6, dtype=np.float64)
    x = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * a + 0.5 * a
    n = len(x)
    lo, hi, per = np.zeros(3), np.full(3, 6 * a), (1, 0, 1)
    types = (1 + (np.arange(n) % 2)).astype(np.int32)
    lmp = Lammps()
    lmp.set_box(lo, hi)
    lmp.create_atoms(x, np.full(n, 0.25 * a), np.full(n, 2650.0), v=np.zeros((n, 3)), type_=types)
    bed = dict(x=x, v=np.zeros((n, 3)), diameter=np.full(n, 0.25 * a), density=np.full(n, 2650.0), boxlo=lo, boxhi=hi,
               periodic=per, type=types)
    cfg = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=0.0, dt=1.0e-6, skin=0.1 * a, walls=[])
    for line in dc.script_lines(bed, cfg):
        lmp.command(line)
    rc = 2.0 * a
    lmp.command("compute g all rdf 8 1 1 1 2 * * cutoff %.17g" % rc)
    lmp.command("compute c all coord/atom cutoff %.17g * 2" % rc)
    lmp.command("run 0")
    st = lmp.get_state()
    assert st["x"].tobytes() == x.tobytes()
    every = np.ones(n, bool)
    pairs = (("1", "1"), ("1", "2"), ("*", "*"))
    want = nm.rdf_counts(st["x"], types, every, lo, hi, per, 8, rc, pairs)
    got = lmp.rdf_counts("g")
    assert got["counts"].tolist() == want["counts"].tolist()
    # by hand, for the inner atoms of the periodic dimensions: bin 4 holds the distance a, bins 5 and 6 a sqrt 2 and a sqrt 3;
    # the distance 2 a is the cutoff itself and is skipped
    assert want["counts"][2, :4].sum() == 0 and want["counts"][2, 4] > 0 and want["counts"][2, 7] == 0
    assert lmp.compute_array("g").tobytes() == nm.rdf_array(want, lo, hi, 8, rc).tobytes()
    coord = nm.coord_atom(st["x"], types, every, lo, hi, per, rc, ("*", "2"))
    assert lmp.compute_atom("c").tobytes() == coord.tobytes()
    inner = (x[:, 1] > 2 * a) & (x[:, 1] < 4 * a)
    assert set(coord[inner, 0].tolist()) == {26.0}   # 6 + 12 + 8 within sqrt 3 spacings; the 6 at exactly 2 a are not counted
    assert int(coord[:, 0].sum()) == int(want["counts"][2].sum())
    lmp.close()


def test_nbin_times_npairs_of_8192_is_taken_and_8193_is_not():
    lmp, bed = _engine(108)
    lmp.command("compute big all rdf 8192 cutoff 1.3e-3")
    lmp.command("compute two all rdf 4096 1 1 2 2 cutoff 1.3e-3")
    for line in ("compute x all rdf 8193 cutoff 1.3e-3", "compute x all rdf 4097 1 1 2 2 cutoff 1.3e-3"):
        with pytest.raises(SfError, match="above 8192"):
            lmp.command(line)
    lmp.command("run 0")
    inp = _inputs(lmp, bed)
    _check_rdf(lmp, inp, "big", "all", 8192, 1.3e-3, (("*", "*"),))
    _check_rdf(lmp, inp, "two", "all", 4096, 1.3e-3, (("1", "1"), ("2", "2")))
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# coord/atom behind the consumers of a per-atom compute

def test_coord_atom_reaches_dump_custom_reduce_ave_histo_and_ave_chunk(tmp_path):
    lmp, bed = _engine(108)
    rc = 1.3e-3
    lmp.command("compute c3 all coord/atom cutoff %.17g 1 2 *" % rc)
    lmp.command("compute c1 two coord/atom cutoff %.17g 2" % rc)
    lmp.command("compute sums all reduce sum c_c3[1] c_c3[3] c_c1")
    lmp.command("compute ch all chunk/atom bin/1d y lower 0.61e-3 units box")
    lmp.command("fix pc all ave/chunk 1 1 1 ch c_c3[3] c_c1")
    lmp.command("fix hh all ave/histo 1 1 1 -0.5 19.5 20 c_c3[3] mode vector")
    path = tmp_path / "c.dump"
    lmp.command("dump d all custom 25 %s id c_c3[2] c_c1" % path)
    lmp.command("dump_modify d sort id")
    lmp.command("run 25")
    inp = _inputs(lmp, bed)
    c3 = _check_coord(lmp, inp, "c3", "all", rc, ("1", "2", "*"))
    c1 = _check_coord(lmp, inp, "c1", "two", rc, ("2",))
    assert (c3[:, 0] + c3[:, 1]).tolist() == c3[:, 2].tolist() and c3[:, 2].max() >= 12 and not c1[~inp["masks"]["two"]].any()
    fr = frames(str(path))
    assert [f[0] for f in fr] == [0, 25]
    rows = [r.split(b" ") for r in fr[-1][3]]
    assert [float(r[1]) for r in rows] == c3[:, 1].tolist() and [float(r[2]) for r in rows] == c1.tolist()
    assert all(r[1] == b"%g" % v for r, v in zip(rows, c3[:, 1]))
    # integers below 2^53 add exactly in any order
    assert lmp.compute_global("sums").tolist() == [c3[:, 0].sum(), c3[:, 2].sum(), c1.sum()]
    h = lmp.ave_histo("hh")
    assert np.asarray(h["count"]).tolist() == np.bincount(c3[:, 2].astype(int), minlength=20)[:20].astype(float).tolist()
    ch = lmp.compute_atom("ch").astype(int)
    out = lmp.ave_chunk("pc")
    nchunk = len(out["count"])
    for k in range(nchunk):
        sel = ch == k + 1
        if sel.any():
            assert out["values"][k][0] == c3[sel, 2].sum() / sel.sum()
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# determinism, sharing and launch accounting

def _bits(lmp, ids):
    return b"".join(lmp.compute_array(i).tobytes() + lmp.rdf_counts(i)["counts"].tobytes() for i in ids)


def test_two_fresh_engines_and_an_rdf_next_to_others_give_the_same_bits():
    out = []
    for extra in (False, False, True):
        lmp, bed = _engine(257)
        if extra:
            lmp.command("compute o1 two rdf 7 1 2 cutoff 1.3e-3")
            lmp.command("compute o2 all coord/atom cutoff 2.0e-3 1 2")
        lmp.command("compute g all rdf 100 1 1 1 2 cutoff 2.0e-3")
        lmp.command("run 25")
        if extra:
            lmp.compute_array("o1"), lmp.compute_atom("o2")
        out.append(_bits(lmp, ["g"]) + (lmp.compute_atom("o2").tobytes() if extra else b""))
        lmp.close()
    assert out[0] == out[1] and out[2].startswith(out[0])


def test_one_grid_per_cutoff_and_step_and_nothing_without_a_consumer():
    lmp, bed = _engine(108)
    lmp.command("compute g all rdf 10 cutoff 1.3e-3")
    lmp.command("compute c all coord/atom cutoff 1.3e-3")
    lmp.command("compute far all rdf 10 cutoff 2.0e-3")
    lmp.command("run 30")
    zero = dict(grid_builds=0, launches=0, host_copies=0)
    assert lmp.nbr_launches() == zero, "nothing is launched without a consumer"
    lmp.compute_array("g")
    one = lmp.nbr_launches()
    assert one["grid_builds"] == 1 and one["host_copies"] == 1
    lmp.compute_atom("c")            # the same cutoff at the same step: the same grid
    lmp.compute_array("g")           # ... and the same array
    two = lmp.nbr_launches()
    assert two["grid_builds"] == 1 and two["launches"] == one["launches"] + 1
    lmp.compute_array("far")         # another cutoff: another grid
    assert lmp.nbr_launches()["grid_builds"] == 2
    lmp.command("run 5")
    assert lmp.nbr_launches()["grid_builds"] == 2
    lmp.compute_array("g")
    assert lmp.nbr_launches()["grid_builds"] == 3
    g, w = lmp.nbr_cost("g")
    gc, wc = lmp.nbr_cost("c")
    assert g > 0.0 and w > 0.0 and gc > 0.0 and wc > 0.0
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# fix ave/time mode vector

VWORDS = ["c_g[2]", "c_g[3]", "c_h[1]", "c_h[4]"]


def _vector_engine():
    lmp, bed = _engine(108)
    lmp.command("compute g all rdf 7 cutoff 1.3e-3")
    lmp.command("compute h two rdf 7 1 2 2 2 cutoff 2.0e-3")
    return lmp


def _columns(lmp):
    g, h = lmp.compute_array("g"), lmp.compute_array("h")
    return np.stack([g[:, 1], g[:, 2], h[:, 0], h[:, 3]], axis=1)


@pytest.mark.parametrize("ave", ["one", "running", "window 2"])
@pytest.mark.parametrize("sched", [(2, 3, 10, 0), (10, 1, 10, 0), (5, 2, 10, 25)])
def test_time_averages_of_columns_are_the_models(sched, ave):
    nevery, nrepeat, nfreq, start = sched
    lmp = _vector_engine()
    lmp.command("fix t all ave/time %d %d %d %s mode vector ave %s" % (nevery, nrepeat, nfreq, " ".join(VWORDS), ave)
                + (" start %d" % start if start else ""))
    with pytest.raises(SfError, match="has made no output yet"):
        lmp.ave_time("t")
    end, piece = 60, (2 if nevery % 2 == 0 else 1)
    plan = gm.schedule(0, nevery, nrepeat, nfreq, end, start)
    assert len(plan) >= 4
    samples = {s for _, ss in plan for s in ss}
    outputs = {o for o, _ in plan}
    w = ave.split()
    model = nm.VectorAverager(7, 4, nrepeat, w[0], int(w[1]) if len(w) > 1 else 0)
    lmp.command("run 0")
    step, nout = 0, 0
    while True:
        if step in samples:
            model.add_sample(_columns(lmp))
        if step in outputs:
            want = model.output()
            got = lmp.ave_time("t")
            assert got["step"] == step and got["names"] == VWORDS and got["values"].shape == (7, 4)
            assert got["values"].tobytes() == want.tobytes(), (step, np.abs(got["values"] - want).max())
            nout += 1
        if step >= end:
            break
        lmp.command("run %d" % piece)
        step += piece
    assert nout == len(plan)
    lmp.close()


@pytest.mark.parametrize("sched", [(2, 3, 10, 0), (10, 1, 10, 0), (5, 2, 10, 25)])
def test_output_steps_of_one_uncut_run(tmp_path, sched):
    nevery, nrepeat, nfreq, start = sched
    lmp = _vector_engine()
    path = tmp_path / "t.txt"
    lmp.command("fix t all ave/time %d %d %d c_g[2] mode vector file %s" % (nevery, nrepeat, nfreq, path)
                + (" start %d" % start if start else ""))
    lmp.command("run 60")
    body = open(path).read().splitlines()[3:]
    heads = [ln.split() for ln in body[::8]]
    assert [int(h[0]) for h in heads] == [o for o, _ in gm.schedule(0, nevery, nrepeat, nfreq, 60, start)]
    assert all(h[1] == "7" for h in heads) and len(body) == 8 * len(heads)
    assert lmp.ave_time("t")["step"] == 60
    lmp.close()


def test_files_are_the_models_text(tmp_path):
    lmp = _vector_engine()
    vals = "c_g[2] c_h[4]"
    p = {k: tmp_path / (k + ".txt") for k in ("plain", "over", "titles", "fmt")}
    lmp.command("fix plain all ave/time 2 3 10 %s mode vector file %s" % (vals, p["plain"]))
    lmp.command("fix over all ave/time 2 3 10 %s mode vector file %s overwrite" % (vals, p["over"]))
    lmp.command("fix titles all ave/time 2 3 10 %s file %s title1 \"# one two\" title2 '# three  four' title3 \"# Row g  n\" "
                "mode vector" % (vals, p["titles"]))
    lmp.command("fix fmt all ave/time 2 3 10 %s mode vector file %s format \" %%.10g\"" % (vals, p["fmt"]))
    words = vals.split()
    want = {"plain": nm.vector_header("plain", words), "over": nm.vector_header("over", words),
            "titles": nm.vector_header("titles", words, "# one two", "# three  four", "# Row g  n"),
            "fmt": nm.vector_header("fmt", words)}
    over_head = want["over"]
    for k in range(3):
        lmp.command("run 10")
        step = 10 * (k + 1)
        for name in want:
            out = lmp.ave_time(name)
            assert out["step"] == step and out["values"].shape == (7, 2)
            text = nm.vector_block(step, out["values"], " %.10g" if name == "fmt" else " %g")
            want[name] = over_head + text if name == "over" else want[name] + text
        for name in want:
            assert open(p[name], "rb").read() == want[name].encode(), name
    assert want["plain"].count("\n") == 3 + 3 * 8 and want["over"].count("\n") == 3 + 8
    lmp.close()


def test_a_sample_that_is_not_an_output_makes_no_host_copy():
    lmp = _vector_engine()
    lmp.command("fix t all ave/time 5 2 10 c_g[2] c_h[2] mode vector")
    lmp.command("run 0")
    b_n, b_g = lmp.nbr_launches(), lmp.global_launches()
    lmp.command("run 5")   # step 5: a sample, not an output
    a_n, a_g = lmp.nbr_launches(), lmp.global_launches()
    assert a_n["grid_builds"] - b_n["grid_builds"] == 2 and a_n["launches"] > b_n["launches"]
    assert a_n["host_copies"] == b_n["host_copies"] and a_g["host_copies"] == b_g["host_copies"]
    assert a_g["launches"] - b_g["launches"] == 2   # one addition launch per column
    lmp.command("run 5")   # step 10: the output
    o_n, o_g = lmp.nbr_launches(), lmp.global_launches()
    assert o_n["host_copies"] == a_n["host_copies"] and o_g["host_copies"] - a_g["host_copies"] == 1
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# passivity

def _passive_run(tmp_path, name, extras):
    bed, cfg = _bed(108)
    lmp = dc.make_hip(bed, cfg)
    dump = tmp_path / (name + ".dump")
    lmp.command("dump d all custom 5 %s id x y z vx vy vz fx fy fz" % dump)
    lmp.command("dump_modify d sort id")
    if extras:
        lmp.command("group two type 2")
        lmp.command("compute g all rdf 20 1 1 1 2 cutoff 2.0e-3")
        lmp.command("compute c two coord/atom cutoff 1.3e-3 1 2")
        lmp.command("fix t all ave/time 5 2 10 c_g[2] c_g[5] mode vector file %s" % (tmp_path / (name + ".txt")))
    for piece in (55, 30, 45):
        lmp.command("run %d" % piece)
        if extras:
            lmp.compute_array("g"), lmp.rdf_counts("g"), lmp.compute_atom("c")
    lmp.sync()
    st, hist, nb = lmp.get_state(), lmp.history(), lmp.info().nbuilds
    if extras:
        assert lmp.nbr_launches()["launches"] > 0 and lmp.ave_time("t")["step"] == 130
    lmp.close()
    text = open(tmp_path / (name + ".txt"), "rb").read() if extras else b""
    return st, hist, nb, open(dump, "rb").read(), text


def test_the_run_goes_on_with_the_same_bits(tmp_path):
    plain = _passive_run(tmp_path, "plain", False)
    one = _passive_run(tmp_path, "one", True)
    two = _passive_run(tmp_path, "two", True)
    for other in (one, two):
        for k in ("x", "v", "omega", "f", "torque"):
            assert plain[0][k].tobytes() == other[0][k].tobytes(), k
        assert sorted(plain[1]) == sorted(other[1])
        assert all(plain[1][p].tobytes() == other[1][p].tobytes() for p in plain[1])
        assert plain[2] == other[2] and plain[3] == other[3]
    assert one[4].replace(b"fix one", b"fix two") == two[4] and one[4].count(b"\n") == 3 + 13 * 21


# ---------------------------------------------------------------------------------------------------------------------
# refusals

REFUSALS = [
    ("compute x all rdf", "Illegal compute rdf command"),
    ("compute x all rdf 0 cutoff 1e-3", "Illegal compute rdf command"),
    ("compute x all rdf 10 1 cutoff 1e-3", "Illegal compute rdf command"),
    ("compute x all rdf 10 2*1 1 cutoff 1e-3", "Illegal compute rdf command"),
    ("compute x all rdf 10 cutoff 0", "Illegal compute rdf command"),
    ("compute x all rdf 10 cutoff 1e-3 extra", "Illegal compute rdf command"),
    ("compute x all rdf 10", "compute rdf: the cutoff keyword is required (this engine's pair list ends at the contact distance "
                             "plus the skin)"),
    ("compute x all rdf 10 1 1", "the cutoff keyword is required"),
    ("compute x all rdf 8193 cutoff 1e-3", "above 8192"),
    ("compute g all rdf 10 cutoff 1e-3", "Reuse of compute ID"),
    ("compute g all ke", "Reuse of compute ID"),
    ("compute c all coord/atom cutoff 1e-3", "Reuse of compute ID"),
    ("compute x all coord/atom", "Illegal compute coord/atom command"),
    ("compute x all coord/atom cutoff", "Illegal compute coord/atom command"),
    ("compute x all coord/atom cutoff -1", "Illegal compute coord/atom command"),
    ("compute x all coord/atom cutoff 1e-3 x", "Illegal compute coord/atom command"),
    ("compute x all coord/atom orientorder o 0.5", "compute coord/atom: only cstyle cutoff is supported"),
    ("compute x all coord/atom 2.0e-3", "compute coord/atom: only cstyle cutoff is supported"),
    ("compute x all coord/atom cutoff 1e-3 1 2 3 4 5 6 7 8 9", "more than 8 type ranges"),
    ("compute x all msd", "reduce, ke and erotate/sphere"),
    ("compute x all msd", "rdf"),
    ("compute x all temp", "Invalid compute style temp"),
    ("compute x all pressure NULL", "Invalid compute style pressure"),
    ("compute x all reduce sum c_g", "Compute reduce compute calculates global values"),
    ("compute x all reduce sum c_g[2]", "Compute reduce compute calculates global values"),
    ("thermo_style custom step c_g", "Thermo compute does not compute scalar"),
    ("thermo_style custom step c_g[2]", "Thermo compute does not compute vector"),
    ("fix x all ave/histo 1 1 1 0 1 10 c_g[2]", "Fix ave/histo compute does not calculate a global scalar or vector"),
    ("dump x all custom 10 {p} id c_g", "Dump custom compute does not compute per-atom info"),
    ("dump x all local 10 {p} index c_g", "Dump local compute does not compute local info"),
    ("fix x all ave/chunk 2 3 10 ch c_g", "Fix ave/chunk compute does not calculate per-atom values"),
    ("fix x all ave/chunk 2 3 10 g vx", "Fix ave/chunk does not use chunk/atom compute"),
    ("fix x all ave/time 2 3 10 c_g", "Fix ave/time compute does not calculate a scalar"),
    ("fix x all ave/time 2 3 10 c_g[2]", "Fix ave/time compute does not calculate a vector"),
    ("fix x all ave/time 2 3 10 c_g[2] mode scalar", "Fix ave/time compute does not calculate a vector"),
    ("fix x all ave/time 2 3 10 c_r mode vector", "mode vector is not supported"),
    ("fix x all ave/time 2 3 10 c_g mode vector", "mode vector is not supported"),
    ("fix x all ave/time 2 3 10 c_rv[1] mode vector", "Fix ave/time compute does not calculate an array"),
    ("fix x all ave/time 2 3 10 c_c[1] mode vector", "Fix ave/time compute does not calculate an array"),
    ("fix x all ave/time 2 3 10 c_nope[1] mode vector", "Compute ID for fix ave/time does not exist"),
    ("fix x all ave/time 2 3 10 c_g[4] mode vector", "Fix ave/time compute array is accessed out-of-range"),
    ("fix x all ave/time 2 3 10 c_g[2] c_g7[2] mode vector", "Fix ave/time columns must all be the same length"),
    ("fix x all ave/time 2 3 10 c_g[2] mode vector off 1", "off is not supported"),
    ("fix x all ave/time 2 3 10 c_g[2] mode", "Illegal fix ave/time command"),
    ("fix tv all ave/time 2 3 10 c_g[2] mode vector", "this fix ID is in use"),
    ("uncompute g", "a fix ave/time still uses this compute"),
]


def _refusal_engine():
    lmp, bed = _engine(108)
    for line in ("compute g all rdf 10 cutoff 1.3e-3", "compute g7 all rdf 7 cutoff 1.3e-3", "compute c all coord/atom cutoff 1.3e-3 1 2",
                 "compute r all reduce sum vx", "compute rv all reduce sum vx vy",
                 "compute ch all chunk/atom bin/1d y lower 0.61e-3 units box", "fix tv all ave/time 2 3 10 c_g[2] c_g[3] mode vector"):
        lmp.command(line)
    return lmp


def test_every_refusal_by_message(tmp_path):
    lmp = _refusal_engine()
    for line, msg in REFUSALS:
        with pytest.raises(SfError) as err:
            lmp.command(line.replace("{p}", str(tmp_path / "x.dump")))
        assert msg in str(err.value), (line, str(err.value))
    for query, msg in ((lambda: lmp.compute_global("g"), "does not calculate a global scalar or vector"),
                       (lambda: lmp.compute_atom("g"), "does not calculate per-atom values"),
                       (lambda: lmp.compute_array("c"), "does not calculate a global array"),
                       (lambda: lmp.compute_array("r"), "does not calculate a global array"),
                       (lambda: lmp.compute_array("nope"), "Could not find compute ID nope"),
                       (lambda: lmp.rdf_counts("c"), "Could not find compute rdf ID c"),
                       (lambda: lmp.nbr_cost("r"), "Could not find compute rdf or coord/atom ID r")):
        with pytest.raises(SfError) as err:
            query()
        assert msg in str(err.value), str(err.value)
    # what was refused left nothing behind: the engine still runs, and an array no fix names can go
    lmp.command("run 10")
    assert lmp.ave_time("tv")["values"].shape == (10, 2)
    lmp.command("uncompute g7")
    lmp.command("unfix tv")
    lmp.command("uncompute g")
    with pytest.raises(SfError, match="Could not find compute ID g"):
        lmp.compute_array("g")
    lmp.close()


@pytest.mark.parametrize("line,msg", [
    ("compute x all rdf 10 cutoff 1.3e-3", "compute rdf: one rank only"),
    ("compute x all coord/atom cutoff 1.3e-3", "compute coord/atom: one rank only"),
    ("fix x all ave/time 2 3 10 c_g[2] mode vector", "fix ave/time: one rank only"),
])
def test_a_decomposed_handle_is_refused_at_each_command_and_at_evaluation(line, msg):
    lmp, bed = _engine(108)
    lmp.command("compute g all rdf 10 cutoff 1.3e-3")
    lmp.command("compute c all coord/atom cutoff 1.3e-3")
    _decompose(lmp)
    with pytest.raises(SfError, match=msg):
        lmp.command(line)
    with pytest.raises(SfError, match="compute rdf: one rank only"):
        lmp.compute_array("g")
    with pytest.raises(SfError, match="compute coord/atom: one rank only"):
        lmp.compute_atom("c")
    lmp.close()
