"""`fix ID group ave/histo ...`, Lammps.ave_histo(), ave_histo_launches() (csrc/sf_histo.hip): histograms counted on the GPU
against the NumPy statement of the rules (tests/histo_model.py, itself held to hand-computed answers by
tests/test_histo_model.py).

The model is fed the engine's own bits (get_state(), compute_atom(), contacts(), compute_global()).  The binning expression is
IEEE float64 without contraction and the counters are integers, so every count, total, missing, min, max, coordinate and
fraction is compared with ==: no tolerance applies anywhere in this file.

The beds are those of tests/test_global_gpu.py: the 108-grain bed; 864 grains (three full blocks of 256 and a partial one); 257
grains (one block and one element); one atom."""
import numpy as np
import pytest

from sedifoam_amd import SfError, synthetic
from tests import dem_cases as dc
from tests import global_model as gm
from tests import histo_model as hm
from tests.test_compute_atom_gpu import _decompose
from tests.test_contacts_gpu import STYLES, _small
from tests.test_global_gpu import GROUPS, _groups, _masks, _sized, _third

pytestmark = pytest.mark.gpu

NBIN = 7


def _range(values):
    """lo < hi from the data, so that some values fall below lo and some above hi (where the data has three distinct values)"""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    lo, hi = float(v[len(v) // 5]), float(v[(4 * len(v)) // 5])
    if not lo < hi:
        hi = lo + 1.0
    return lo, hi


def _same(got, want, bins, step=None):
    assert got["nbins"] == bins.nbins and got["count"].dtype == np.float64
    assert got["count"].tolist() == want.count.tolist(), (got["count"], want.count)
    assert (got["total"], got["missing"], got["min"], got["max"]) == (want.total, want.missing, want.min, want.max)
    assert got["coord"].tolist() == bins.coord.tolist()
    assert got["frac"].tolist() == want.frac.tolist()
    assert got["count"].sum() == got["total"]
    if step is not None:
        assert got["step"] == step


def _fix(lmp, fid, group, sched, lo, hi, nbin, values, rest=""):
    lmp.command("fix %s %s ave/histo %s %r %r %d %s %s" % (fid, group, sched, float(lo), float(hi), nbin, values, rest))


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-atom values over three groups and the three `beyond` modes

ATOM_VALUES = {"v": "vx vy vz", "y": "y", "fz": "fz", "k": "c_k", "s4": "c_s[4]", "c": "c_c", "prop": "c_prop[16]", "k2": "c_k2"}


def _atom_columns(st, lmp):
    prop = lmp.compute_atom("prop")
    return {"v": [st["v"][:, 0], st["v"][:, 1], st["v"][:, 2]], "y": [st["x"][:, 1]], "fz": [st["f"][:, 2]],
            "k": [lmp.compute_atom("k")], "s4": [lmp.compute_atom("s")[:, 3]], "c": [lmp.compute_atom("c")], "prop": [prop[:, 15]],
            "k2": [lmp.compute_atom("k2")]}


@pytest.fixture(scope="module")
def moved():
    """the 108-grain bed after 25 steps; ranges from the data; every fix samples the state of step 25 at the setup of `run 0`"""
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    for line in ("compute k all ke/atom", "compute k2 two ke/atom", "compute s all stress/atom", "compute c all contact/atom",
                 "compute prop all property/atom id type mass radius diameter x y z vx vy vz fx fy fz omegax omegay omegaz"):
        lmp.command(line)
    lmp.command("run 25")
    cols = _atom_columns(lmp.get_state(), lmp)
    ranges = {name: _range(np.concatenate(c)) for name, c in cols.items()}
    for name, words in ATOM_VALUES.items():
        for g in GROUPS:
            for beyond in hm.BEYOND:
                _fix(lmp, "h_%s_%s_%s" % (name, g, beyond), g, "1 1 1", ranges[name][0], ranges[name][1], NBIN, words,
                     "mode vector beyond " + beyond)
    before = lmp.ave_histo_launches()
    lmp.command("run 0")
    after = lmp.ave_histo_launches()
    st = lmp.get_state()
    assert (st["tag"] == np.arange(1, len(bed["x"]) + 1)).all() and lmp.info().nsteps == 25
    out = dict(bed=bed, ranges=ranges, cols=_atom_columns(st, lmp), nfix=len(ATOM_VALUES) * 9,
               launches=after["launches"] - before["launches"], copies=after["host_copies"] - before["host_copies"])
    out["got"] = {(n, g, b): lmp.ave_histo("h_%s_%s_%s" % (n, g, b)) for n in ATOM_VALUES for g in GROUPS for b in hm.BEYOND}
    lmp.close()
    return out


@pytest.mark.parametrize("beyond", hm.BEYOND)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", list(ATOM_VALUES))
def test_per_atom_values(moved, name, group, beyond):
    mask = _masks(moved["bed"])[group]
    assert mask.sum() == {"all": 108, "two": 36, "none": 0}[group]
    lo, hi = moved["ranges"][name]
    bins = hm.Bins(lo, hi, NBIN, beyond)
    values = np.concatenate([c[mask] for c in moved["cols"][name]])
    want = hm.bin_values(bins, values)
    _same(moved["got"][(name, group, beyond)], want, bins, 25)
    if group == "all" and name in ("v", "y", "k", "prop"):
        assert (values < lo).any() and (values > hi).any()
    assert want.missing == (((values < lo) | (values > hi)).sum() if beyond == "ignore" else 0)
    if group == "none":
        assert want.total == 0 and want.min == 1.0e20 and want.max == -1.0e20
    if name == "k2" and group == "all":   # atoms outside the named compute's own group read 0, and are binned
        assert (values == 0.0).sum() == 72 and want.min == 0.0


def test_one_launch_per_fix_and_sample(moved):
    # (the fixes over the empty group launch too: the grid depends on the element count alone, not on the group)
    assert moved["launches"] == moved["nfix"] and moved["copies"] == moved["nfix"]


@pytest.mark.parametrize("n", [1, 257, 864])
def test_sizes_around_the_block(n):
    bed, cfg = _sized(n)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    lmp.command("compute k all ke/atom")
    lmp.command("run 5")
    st = lmp.get_state()
    rv, rk = _range(st["v"]) if n > 1 else (-0.05, 0.05), _range(lmp.compute_atom("k")) if n > 1 else (0.0, 1.0e-9)
    for g in ("all", "two"):
        for beyond in hm.BEYOND:
            _fix(lmp, "v_%s_%s" % (g, beyond), g, "1 1 1", rv[0], rv[1], 100, "vx vy vz", "mode vector kind peratom beyond " + beyond)
            _fix(lmp, "k_%s_%s" % (g, beyond), g, "1 1 1", rk[0], rk[1], 3, "c_k", "mode vector beyond " + beyond)
    lmp.command("run 0")
    st, k = lmp.get_state(), lmp.compute_atom("k")
    for g in ("all", "two"):
        mask = _masks(bed)[g]
        for beyond in hm.BEYOND:
            bins = hm.Bins(rv[0], rv[1], 100, beyond)
            _same(lmp.ave_histo("v_%s_%s" % (g, beyond)), hm.bin_values(bins, st["v"][mask].T), bins, 5)
            bins = hm.Bins(rk[0], rk[1], 3, beyond)
            _same(lmp.ave_histo("k_%s_%s" % (g, beyond)), hm.bin_values(bins, k[mask]), bins, 5)
    assert lmp.ave_histo("v_all_end")["total"] == 3 * n
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact edges

def test_values_on_the_edges():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute p all property/atom type")
    lmp.command("compute pid all property/atom id")
    for beyond in hm.BEYOND:
        lmp.command("fix t_%s all ave/histo 1 1 1 1 2 4 c_p mode vector beyond %s" % (beyond, beyond))
    lmp.command("fix ids all ave/histo 1 1 1 1 108 107 c_pid mode vector")
    lmp.command("run 0")
    t = np.asarray(bed["type"], np.float64)
    assert (t == 1).sum() == 72 and (t == 2).sum() == 36
    for beyond, count in (("ignore", [72, 0, 0, 36]), ("end", [72, 0, 0, 36]), ("extra", [0, 72, 0, 0, 0, 36])):
        bins = hm.Bins(1, 2, 4, beyond)
        want = hm.bin_values(bins, t)
        assert want.count.tolist() == count and want.missing == 0
        _same(lmp.ave_histo("t_" + beyond), want, bins, 0)
    bins = hm.Bins(1, 108, 107)
    want = hm.bin_values(bins, np.arange(1, 109))
    assert want.count.tolist() == [1] * 106 + [2]   # every value on an edge; the last bin holds two
    _same(lmp.ave_histo("ids"), want, bins, 0)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. local values

def test_the_columns_of_a_compute_pair_local():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    lmp.command("compute pl all pair/local dist force tag1 eng")
    lmp.command("compute pl1 two pair/local force")
    lmp.command("run 25")
    rows = lmp.contacts()
    rf, rd = _range(rows["force"]), _range(rows["dist"])
    for beyond in hm.BEYOND:
        # (the group of the fix does not matter for rows: `none` is empty)
        _fix(lmp, "f_" + beyond, "none", "1 1 1", rf[0], rf[1], NBIN, "c_pl[2]", "mode vector kind local beyond " + beyond)
        _fix(lmp, "d_" + beyond, "all", "1 1 1", rd[0], rd[1], 100, "c_pl[1]", "mode vector beyond " + beyond)
        _fix(lmp, "two_" + beyond, "all", "1 1 1", rf[0], rf[1], NBIN, "c_pl[2] c_pl1 c_pl[4]", "mode vector beyond " + beyond)
    _fix(lmp, "tag", "all", "1 1 1", 1.0, 109.0, 108, "c_pl[3]", "mode vector")
    before = lmp.ave_histo_launches()["launches"]
    lmp.command("run 0")
    assert lmp.ave_histo_launches()["launches"] - before == 3 * (1 + 1 + 2) + 1   # (two computes named: two launches)
    rows, rows2 = lmp.contacts(), lmp.contacts("two")
    n = len(rows["tag1"])
    assert n > 4 * 108 and 0 < len(rows2["tag1"]) < n
    for beyond in hm.BEYOND:
        bins = hm.Bins(rf[0], rf[1], NBIN, beyond)
        want = hm.bin_values(bins, rows["force"])
        assert want.total + want.missing == n
        _same(lmp.ave_histo("f_" + beyond), want, bins, 25)
        _same(lmp.ave_histo("two_" + beyond), hm.bin_values(bins, np.concatenate([rows["force"], rows2["force"], np.zeros(n)])),
              bins, 25)
        bins = hm.Bins(rd[0], rd[1], 100, beyond)
        _same(lmp.ave_histo("d_" + beyond), hm.bin_values(bins, rows["dist"]), bins, 25)
    bins = hm.Bins(1.0, 109.0, 108)
    _same(lmp.ave_histo("tag"), hm.bin_values(bins, rows["tag1"]), bins, 25)
    lmp.close()


def test_a_bed_with_no_touching_pair_has_zero_rows():
    bed = synthetic.fcc_bed((2, 2, 2), spacing=1.6, seed=3, vmax=0.2)
    cfg = dict(STYLES["hertz"], g=0.0, dt=1.0e-6, skin=0.25e-3, walls=[])
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute pl all pair/local dist force")
    lmp.command("fix h all ave/histo 1 1 1 0 1 5 c_pl[1] c_pl[2] mode vector beyond extra")
    lmp.command("run 0")
    assert len(lmp.contacts()["tag1"]) == 0
    bins = hm.Bins(0, 1, 5, "extra")
    _same(lmp.ave_histo("h"), hm.bin_values(bins, []), bins, 0)
    assert lmp.ave_histo("h")["frac"].tolist() == [0.0] * 7
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. global values

def test_global_scalars_and_vectors_over_a_schedule():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute r all reduce max y")
    lmp.command("compute r3 all reduce sum vx vy vz")
    lmp.command("run 0")
    y0, s0 = lmp.compute_global("r")[0], lmp.compute_global("r3")
    ry = (y0 - 1.0e-6, y0 + 1.0e-6)
    rs = (float(s0.min()), float(s0.max()))
    _fix(lmp, "sc", "all", "2 3 10", ry[0], ry[1], 8, "c_r", "beyond end")
    _fix(lmp, "vec", "all", "2 3 10", rs[0], rs[1], 5, "c_r3", "mode vector kind global beyond extra")
    _fix(lmp, "mix", "all", "2 3 10", rs[0], rs[1], 5, "c_r3[2] c_r c_r3[3]", "mode scalar")
    bins = {"sc": hm.Bins(ry[0], ry[1], 8, "end"), "vec": hm.Bins(rs[0], rs[1], 5, "extra"), "mix": hm.Bins(rs[0], rs[1], 5)}
    plan = gm.schedule(0, 2, 3, 10, 30)
    assert [o for o, _ in plan] == [10, 20, 30] and plan[0][1] == [6, 8, 10]
    samples, outputs = {s for _, ss in plan for s in ss}, {o for o, _ in plan}
    blocks = {k: hm.Block(b.nbins) for k, b in bins.items()}
    for step in range(2, 31, 2):
        lmp.command("run 2")
        if step in samples:
            r, r3 = lmp.compute_global("r"), lmp.compute_global("r3")
            hm.bin_values(bins["sc"], r, blocks["sc"])
            hm.bin_values(bins["vec"], r3, blocks["vec"])
            hm.bin_values(bins["mix"], [r3[1], r[0], r3[2]], blocks["mix"])
        if step in outputs:
            for k in bins:
                _same(lmp.ave_histo(k), blocks[k], bins[k], step)
            assert blocks["sc"].total == 3 and blocks["vec"].total == 9 and blocks["mix"].total + blocks["mix"].missing == 9
            blocks = {k: hm.Block(b.nbins) for k, b in bins.items()}
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. averaging

@pytest.mark.parametrize("ave", ["one", "running", "window 2"])
@pytest.mark.parametrize("sched", [(2, 3, 10, 0), (10, 1, 10, 0), (5, 2, 10, 25)])
def test_averages_over_four_outputs(sched, ave):
    """a piecewise run; the model is fed get_state() after each piece that ends on a sample step"""
    nevery, nrepeat, nfreq, start = sched
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    lo, hi = -0.1, 0.12
    _fix(lmp, "h", "two", "%d %d %d" % (nevery, nrepeat, nfreq), lo, hi, 11, "vx vy vz",
         "mode vector beyond end ave %s" % ave + (" start %d" % start if start else ""))
    with pytest.raises(SfError, match="has made no output yet"):
        lmp.ave_histo("h")
    bins = hm.Bins(lo, hi, 11, "end")
    mask = _masks(bed)["two"]
    plan = gm.schedule(0, nevery, nrepeat, nfreq, 60, start)
    assert len(plan) >= 4
    samples, outputs = {s for _, ss in plan for s in ss}, {o for o, _ in plan}
    w = ave.split()
    model = hm.Averager(bins.nbins, w[0], int(w[1]) if len(w) > 1 else 0)
    piece = 2 if nevery % 2 == 0 else 1
    lmp.command("run 0")
    step, nout, block = 0, 0, hm.Block(bins.nbins)
    while True:
        if step in samples:
            hm.bin_values(bins, lmp.get_state()["v"][mask], block)
        if step in outputs:
            assert block.total == 3 * 36 * nrepeat
            _same(lmp.ave_histo("h"), model.output(block), bins, step)
            block = hm.Block(bins.nbins)
            nout += 1
        elif nout:
            assert lmp.ave_histo("h")["step"] == max(o for o in outputs if o < step)
        if step >= 60:
            break
        lmp.command("run %d" % piece)
        step += piece
    assert nout == len(plan)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the one-bin case

@pytest.mark.parametrize("n", [108, 864])
def test_a_bed_at_rest_puts_everything_into_one_bin(n):
    bed, cfg = _small("hertz", types=_third) if n == 108 else _sized(n)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("velocity all set 0 0 0")
    lmp.command("fix h all ave/histo 1 1 1 -1 1 3 vx vy vz mode vector")
    lmp.command("run 0")
    got = lmp.ave_histo("h")
    assert got["count"].tolist() == [0, 3 * n, 0] and got["total"] == 3 * n and got["missing"] == 0
    assert got["min"] == 0.0 and got["max"] == 0.0 and got["frac"].tolist() == [0.0, 1.0, 0.0]
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. files, 8. the query

def _last_block(path, nbins):
    lines = open(path).read().splitlines()
    return lines[-(nbins + 1):]


def test_files_are_the_models_text_and_unfix_stops_one(tmp_path):
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    p = {k: tmp_path / (k + ".txt") for k in ("plain", "over", "titles", "gone")}
    lo, hi = -0.1, 0.12
    rest = {"plain": "", "over": " overwrite", "gone": "",
            "titles": " title1 \"# one two\" title2 '# three  four' title3 \"# five\""}
    for name in p:
        _fix(lmp, name, "all", "10 1 10", lo, hi, 6, "vx vz", "mode vector beyond extra ave running file %s%s" % (p[name], rest[name]))
    bins = hm.Bins(lo, hi, 6, "extra")
    want = {name: hm.header(name) for name in p}
    want["titles"] = hm.header("titles", "# one two", "# three  four", "# five")
    head = want["over"]
    model = hm.Averager(bins.nbins, "running")
    for k in range(4):   # (Nrepeat 1: the first sample is that of step 0, at the setup of the first run)
        lmp.command("run %d" % (10 if k else 0))
        step = 10 * k
        v = lmp.get_state()["v"]
        out = model.output(hm.bin_values(bins, v[:, [0, 2]]))
        text = hm.text(step, bins, out)
        for name in want:
            if name == "gone" and k > 1:
                continue
            want[name] = head + text if name == "over" else want[name] + text
            # the query is the file's last block
            got = lmp.ave_histo(name)
            _same(got, out, bins, step)
            block = _last_block(p[name], bins.nbins)
            assert block[0] == "%d %d %g %g %g %g" % (got["step"], got["nbins"], got["total"], got["missing"], got["min"], got["max"])
            assert block[1:] == ["%d %g %g %g" % (i + 1, got["coord"][i], got["count"][i], got["frac"][i]) for i in range(bins.nbins)]
        if k == 1:
            lmp.command("unfix gone")
            with pytest.raises(SfError, match="Could not find fix ave/histo ID gone"):
                lmp.ave_histo("gone")
        for name in want:
            assert open(p[name], "rb").read() == want[name].encode(), name
    assert want["gone"].count("\n") == 3 + 2 * 9 and want["plain"].count("\n") == 3 + 4 * 9 and want["over"].count("\n") == 3 + 9
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. passivity and determinism

def _passive_run(tmp_path, name, extras):
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    dump = tmp_path / (name + ".dump")
    lmp.command("dump d all custom 5 %s id x y z vx vy vz fx fy fz" % dump)
    lmp.command("dump_modify d sort id")
    files = [tmp_path / ("%s_%s.txt" % (name, k)) for k in ("atom", "local", "global")]
    if extras:
        lmp.command("group two type 2")
        lmp.command("compute k all ke/atom")
        lmp.command("compute pl all pair/local force dist")
        lmp.command("compute r all reduce max y c_k")
        lmp.command("fix ha two ave/histo 5 2 10 -0.1 0.1 20 vx vy vz c_k mode vector beyond end file %s" % files[0])
        lmp.command("fix hl all ave/histo 5 2 10 0 0.05 25 c_pl[1] mode vector beyond extra ave running file %s" % files[1])
        lmp.command("fix hg all ave/histo 5 2 10 0 0.01 10 c_r[1] c_r[2] ave window 3 file %s" % files[2])
        lmp.command("fix t all ave/time 5 2 10 c_r[1] c_r[2]")
    for piece in (55, 30, 45):
        lmp.command("run %d" % piece)
        if extras:
            for fid in ("ha", "hl", "hg"):
                lmp.ave_histo(fid)
            lmp.ave_time("t")
            lmp.compute_global("r")
    lmp.sync()
    st, hist, nb = lmp.get_state(), lmp.history(), lmp.info().nbuilds
    if extras:
        assert lmp.ave_histo_launches()["launches"] == 3 * 26 and all(lmp.ave_histo(f)["step"] == 130 for f in ("ha", "hl", "hg"))
        assert lmp.ave_histo("ha")["total"] == 2 * 4 * 36 and lmp.ave_histo("hl")["total"] > 13 * 2 * 4 * 108
    lmp.close()
    text = [open(f, "rb").read() for f in files] if extras else []
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
    assert one[4] == two[4]
    assert [t.count(b"\n") for t in one[4]] == [3 + 13 * 21, 3 + 13 * 28, 3 + 13 * 11]


# ---------------------------------------------------------------------------------------------------------------------
# 10. accounting

def test_a_sample_that_is_not_an_output_makes_no_host_copy():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute k all ke/atom")
    lmp.command("fix h all ave/histo 5 2 10 -1 1 10 vx c_k mode vector")
    lmp.command("fix g all ave/histo 5 2 10 -1 1 10 fx mode vector")
    lmp.command("run 4")
    assert lmp.ave_histo_launches() == dict(launches=0, host_copies=0)   # (no sample yet: nothing ran)
    lmp.command("run 1")   # step 5: a sample of both fixes
    assert lmp.ave_histo_launches() == dict(launches=2, host_copies=0)
    lmp.command("run 3")   # steps 6 to 8: no fix is due
    assert lmp.ave_histo_launches() == dict(launches=2, host_copies=0)
    lmp.command("run 2")   # step 10: the second sample and the output
    assert lmp.ave_histo_launches() == dict(launches=4, host_copies=2)
    assert lmp.ave_histo("h")["total"] == 2 * 2 * 108
    assert lmp.ave_histo_launches() == dict(launches=4, host_copies=2)   # (a query copies nothing)
    assert lmp.ave_histo_cost("h") > 0.0 and lmp.ave_histo_cost("g") > 0.0
    lmp.command("run 10")
    assert lmp.ave_histo("h")["total"] == 2 * 2 * 108   # (the cost query left the counters alone)
    lmp.close()


@pytest.mark.parametrize("with_histo", [False, True])
def test_a_reduce_that_two_fixes_name_is_evaluated_once(with_histo):
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute r all reduce max y")
    lmp.command("compute q all reduce sum vx vy")
    lmp.command("fix t all ave/time 5 2 10 c_r")
    if with_histo:
        lmp.command("fix h all ave/histo 5 2 10 0 1 10 c_r")
    lmp.command("run 4")
    assert lmp.global_launches()["launches"] == 0
    lmp.command("run 1")
    assert lmp.global_launches() == dict(launches=2, host_copies=0)   # one gather and one fold, histogram or not
    assert lmp.ave_histo_launches()["launches"] == (1 if with_histo else 0)
    if with_histo:
        # a fix ave/histo alone brings its reduce into the plan: h2 samples q at the setup of the run (step 5, one gather and
        # one fold); at step 10 r and q go in one gather and one fold, for the three fixes
        lmp.command("fix h2 all ave/histo 5 2 10 -1 1 10 c_q mode vector")
        lmp.command("run 5")
        assert lmp.global_launches() == dict(launches=6, host_copies=1)
        assert lmp.ave_histo_launches() == dict(launches=4, host_copies=2)
        assert lmp.ave_histo("h2")["total"] + lmp.ave_histo("h2")["missing"] == 4 and lmp.ave_histo("h")["total"] == 2
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals

H = "fix x all ave/histo 2 3 10 0 1 10 "
REFUSALS = [
    ("fix x all ave/histo 2 3 10 0 1 10", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 3 3 10 0 1 10 vx mode vector", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 2 6 10 0 1 10 vx mode vector", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 0 3 10 0 1 10 vx mode vector", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 2 3 10 1 1 10 vx mode vector", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 2 3 10 2 1 10 vx mode vector", "Illegal fix ave/histo command"),
    ("fix x all ave/histo 2 3 10 0 1 0 vx mode vector", "Illegal fix ave/histo command"),
    (H + "vx mode vector bogus 1", "Illegal fix ave/histo command"),
    (H + "vx mode", "Illegal fix ave/histo command"),
    (H + "c_nope", "Compute ID for fix ave/histo does not exist"),
    (H + "vx c_pl[1] mode vector", "Fix ave/histo inputs are not all global, peratom, or local"),
    (H + "c_r1 c_k", "Fix ave/histo inputs are not all global, peratom, or local"),
    (H + "vx", "Fix ave/histo cannot input per-atom values in scalar mode"),
    (H + "c_k", "Fix ave/histo cannot input per-atom values in scalar mode"),
    (H + "c_pl[1]", "Fix ave/histo cannot input local values in scalar mode"),
    (H + "c_rv", "Fix ave/histo compute does not calculate a global scalar"),
    (H + "c_r1[1]", "Fix ave/histo compute does not calculate a global vector"),
    (H + "c_r1 mode vector", "Fix ave/histo compute does not calculate a global vector"),
    (H + "c_rv[3]", "Fix ave/histo compute vector is accessed out-of-range"),
    (H + "c_s mode vector", "Fix ave/histo compute does not calculate a per-atom vector"),
    (H + "c_k[1] mode vector", "Fix ave/histo compute does not calculate a per-atom array"),
    (H + "c_s[7] mode vector", "Fix ave/histo compute array is accessed out-of-range"),
    (H + "c_pl mode vector", "Fix ave/histo compute does not calculate a local vector"),
    (H + "c_pl1[1] mode vector", "Fix ave/histo compute does not calculate a local array"),
    (H + "c_pl[3] mode vector", "Fix ave/histo compute array is accessed out-of-range"),
    (H + "vx mode vector kind local", "kind local does not agree with the values, which are peratom"),
    (H + "c_r1 kind peratom", "kind peratom does not agree with the values, which are global"),
    (H + "f_t mode vector", "f_t is not supported"),
    (H + "v_t mode vector", "v_t is not supported"),
    (H + "c_s[*] mode vector", "c_s[*] is not supported"),
    (H + "vx mode vector file {p} append", "append is not supported"),
    ("fix x all ave/histo/weight 2 3 10 0 1 10 vx c_k mode vector", "fix ave/histo/weight is not supported"),
    ("fix x all ave/histo 2 3 10 0 1 8193 vx mode vector", "more than 8192 bins"),
    (H + "vx mode vector title1 \"# open", "Unbalanced quotes"),
    ("fix x nogroup ave/histo 2 3 10 0 1 10 vx mode vector", "nogroup"),
    ("fix h all ave/histo 2 3 10 0 1 10 vx mode vector", "this fix ID is in use"),
    ("fix t all ave/histo 2 3 10 0 1 10 vx mode vector", "this fix ID is in use"),
    ("fix p all ave/histo 2 3 10 0 1 10 vx mode vector", "this fix ID is in use"),
    ("fix h all ave/time 2 3 10 c_r1", "this fix ID is in use"),
    ("fix h all ave/chunk 2 3 10 ch vx", "this fix ID is in use"),
    ("uncompute k", "a fix ave/histo still uses this compute"),
    ("uncompute pl", "a fix ave/histo still uses this compute"),
    ("uncompute r1", "a fix ave/histo still uses this compute"),
    ("unfix nope", "only a fix ave/chunk can be removed"),
]


def _refusal_engine():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    for line in ("compute k all ke/atom", "compute s all stress/atom", "compute pl all pair/local dist force",
                 "compute pl1 all pair/local force", "compute ch all chunk/atom bin/1d y lower 0.61e-3 units box",
                 "compute rv all reduce sum vx vy", "compute r1 all reduce max y", "compute r2 all reduce min y",
                 "fix t all ave/time 2 3 10 c_r2", "fix p all ave/chunk 2 3 10 ch vx",
                 "fix h all ave/histo 2 3 10 0 1 10 c_k mode vector", "fix hl all ave/histo 2 3 10 0 1 10 c_pl[1] mode vector",
                 "fix hg all ave/histo 2 3 10 0 1 10 c_r1"):
        lmp.command(line)
    return lmp


def test_refusals_by_message(tmp_path):
    lmp = _refusal_engine()
    for line, msg in REFUSALS:
        line = line.replace("{p}", str(tmp_path / "x.txt"))
        with pytest.raises(SfError) as e:
            lmp.command(line)
        assert msg in str(e.value), (line, str(e.value))
    with pytest.raises(SfError, match="Could not find fix ave/histo ID nope"):
        lmp.ave_histo("nope")
    with pytest.raises(SfError, match="Could not find fix ave/histo ID t"):
        lmp.ave_histo("t")
    with pytest.raises(SfError, match="Could not find fix ave/time ID h"):
        lmp.ave_time("h")
    with pytest.raises(SfError, match="has made no output yet"):
        lmp.ave_histo("h")
    # nothing above changed anything: the commands go on working, and unfix frees the computes
    lmp.command("run 10")
    assert lmp.ave_histo("h")["step"] == 10 and lmp.ave_histo("hg")["total"] + lmp.ave_histo("hg")["missing"] == 3
    for fid in ("h", "hl", "hg"):
        lmp.command("unfix " + fid)
    for cid in ("k", "pl", "r1"):
        lmp.command("uncompute " + cid)
    lmp.command("fix h all ave/histo 2 3 10 0 1 10 vx mode vector")
    lmp.close()


def test_a_decomposed_handle_is_refused(tmp_path):
    lmp = _refusal_engine()
    lmp.command("run 0")
    _decompose(lmp)
    with pytest.raises(SfError, match="fix ave/histo: one rank only"):
        lmp.command("fix x all ave/histo 2 3 10 0 1 10 vx mode vector")
    with pytest.raises(SfError, match="fix ave/histo: one rank only"):
        lmp.ave_histo_cost("h")
    lmp.close()
