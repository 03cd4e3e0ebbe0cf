"""`compute ID group reduce ...`, `compute ke`, `compute erotate/sphere`, `compute property/atom`, `fix ID group ave/time ...`,
the c_ columns of thermo_style custom, Lammps.compute_global(), ave_time() and global_launches() (csrc/sf_global.hip): whole-bed
reductions on the GPU against the NumPy statement of the rules (tests/global_model.py, itself held to hand-computed answers by
tests/test_global_model.py).

The model is fed the engine's own bits (get_state(), compute_atom(), contacts()), so only the order of the summation is under
test.  sum and sumsq are held to 2 n 2^-53 sum |term| (n elements: each of the two summations is within n 2^-53 sum |term| of
the exact sum); ave and avesq to that over the count plus one rounding of each of the two divisions (global_model.gate); min,
max and counts compare with ==.  A time average is held to Nrepeat 2^-53 sum |sample| of its block (the accumulator adds the
samples in order, as the model does: the expected error is 0).  Measured on an MI355X: see DESIGN.md section 15.

The beds: the 108-grain bed of tests/test_contacts_gpu.py; a 6 x 6 x 6 fcc bed of 864 grains (three full blocks of 256 and a
partial one); a bed of one atom; a bed of 257 atoms (one block and one element)."""
import numpy as np
import pytest

from sedifoam_amd import SfError, synthetic
from tests import dem_cases as dc
from tests import global_model as gm
from tests.test_compute_atom_gpu import _decompose
from tests.test_contacts_gpu import STYLES, _small
from tests.test_dump_gpu import frames

pytestmark = pytest.mark.gpu

ATTRS = "id type mass radius diameter x y z vx vy vz fx fy fz omegax omegay omegaz tqx tqy tqz".split()
GROUPS = ("all", "two", "none")
ATOM_INPUTS = "vx y fz c_k c_s[4] c_prop[16] c_p1"
ROW_VALUES = "dist force fx p1 tag1 eng"
WORST = {}


def _third(bed):
    return (1 + (np.arange(len(bed["x"])) % 3 == 0)).astype(np.int32)


def _cut(bed, n):
    for k in ("x", "v", "diameter", "density", "omega", "type"):
        if k in bed:
            bed[k] = np.asarray(bed[k])[:n].copy()
    bed["n"] = n
    return bed


def _sized(n):
    """a bed of n grains resting on the wall: 864 = 6 x 6 x 6 cells, otherwise the first n grains of a larger lattice"""
    cells = {864: (6, 6, 6), 257: (4, 4, 5), 1: (3, 3, 3)}[n]
    bed = synthetic.fcc_bed(cells, seed=5, vmax=0.2)
    bed["omega"] = np.random.default_rng(11).uniform(-50.0, 50.0, size=(len(bed["x"]), 3))
    bed = _cut(bed, n)
    bed["type"] = _third(bed)
    cfg = dict(STYLES["hertz"], g=9.81, dt=1.0e-6, skin=0.25e-3, walls=[(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))])
    assert len(bed["x"]) == n
    return bed, cfg


def _masks(bed):
    t = np.asarray(bed["type"])
    return {"all": np.ones(len(t), bool), "two": t == 2, "none": np.zeros(len(t), bool)}


def _groups(lmp):
    lmp.command("group two type 2")
    lmp.command("group none type 3")


def _check(what, mode, got, values, mask=None):
    want, g = gm.reduce(mode, values, mask), gm.gate(mode, values, mask)
    err = abs(got - want)
    rel = err / g if g > 0 else (0.0 if err == 0 else float("inf"))
    WORST[mode] = max(WORST.get(mode, 0.0), rel)
    print("%s %s: got %.17g want %.17g |err| %.3e gate %.3e" % (what, mode, got, want, err, g))
    if mode in ("min", "max"):
        assert got == want, (what, mode, got, want)
    else:
        assert err <= g, (what, mode, got, want, err, g)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every mode on an atom attribute, on c_k, c_s[k] and c_prop[k], and on the columns of a compute pair/local

@pytest.fixture(scope="module")
def moved():
    """the 108-grain bed after 25 steps with every reduce defined; the state, the per-atom columns, the rows, the values"""
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    lmp.command("compute k all ke/atom")
    lmp.command("compute k2 two ke/atom")
    lmp.command("compute s all stress/atom")
    lmp.command("compute prop all property/atom " + " ".join(ATTRS))
    lmp.command("compute p1 all property/atom radius")
    lmp.command("compute pl all pair/local " + ROW_VALUES)
    lmp.command("compute pl1 two pair/local force")
    for mode in gm.MODES:
        for g in GROUPS:
            lmp.command("compute r_%s_%s %s reduce %s %s" % (mode, g, g, mode, ATOM_INPUTS))
        lmp.command("compute q_%s none reduce %s c_pl[1] c_pl[2] c_pl[3] c_pl[4] c_pl[5] c_pl[6] c_pl1" % (mode, mode))
    lmp.command("compute rk2 all reduce sum c_k2")
    lmp.command("compute mk2 all reduce min c_k2")
    lmp.command("run 25")
    st = lmp.get_state()
    assert (st["tag"] == np.arange(1, len(bed["x"]) + 1)).all()
    out = dict(bed=bed, st=st, k=lmp.compute_atom("k"), k2=lmp.compute_atom("k2"), s=lmp.compute_atom("s"),
               prop=lmp.compute_atom("prop"), p1=lmp.compute_atom("p1"), rows=lmp.contacts(), rows2=lmp.contacts("two"))
    names = ["r_%s_%s" % (m, g) for m in gm.MODES for g in GROUPS] + ["q_%s" % m for m in gm.MODES] + ["rk2", "mk2"]
    out["val"] = {name: lmp.compute_global(name) for name in names}
    lmp.close()
    return out


def _atom_columns(m):
    st = m["st"]
    return [st["v"][:, 0], st["x"][:, 1], st["f"][:, 2], m["k"], m["s"][:, 3], m["prop"][:, 15], m["p1"]]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", gm.MODES)
def test_every_mode_on_atom_inputs(moved, mode, group):
    mask = _masks(moved["bed"])[group]
    assert mask.sum() == {"all": 108, "two": 36, "none": 0}[group]
    got = moved["val"]["r_%s_%s" % (mode, group)]
    cols = _atom_columns(moved)
    assert got.shape == (len(cols),) and got.dtype == np.float64
    for name, g, col in zip(ATOM_INPUTS.split(), got, cols):
        _check("%s over %s" % (name, group), mode, g, col, mask)
    if group == "none":
        assert got.tolist() == [{"min": 1.0e20, "max": -1.0e20}.get(mode, 0.0)] * len(cols)


@pytest.mark.parametrize("mode", gm.MODES)
def test_every_mode_on_pair_local_columns(moved, mode):
    """over all rows of the compute, whatever the group of the reduce (here: an empty one)"""
    rows, got = moved["rows"], moved["val"]["q_%s" % mode]
    n = len(rows["tag1"])
    assert n > 4 * 108 and len(moved["rows2"]["tag1"]) < n
    cols = [rows["dist"], rows["force"], rows["f"][:, 0], rows["fs"][:, 0], rows["tag1"].astype(np.float64), np.zeros(n),
            moved["rows2"]["force"]]
    assert got.shape == (7,)
    for name, g, col in zip("dist force fx p1 tag1 eng force(two)".split(), got, cols):
        _check("rows " + name, mode, g, col)


def test_the_named_computes_group_decides_its_values(moved):
    k2, mask = moved["k2"], _masks(moved["bed"])["two"]
    assert not k2[~mask].any() and k2[mask].all()
    _check("c_k2 over all", "sum", moved["val"]["rk2"][0], k2)
    assert moved["val"]["mk2"][0] == 0.0


@pytest.mark.parametrize("mode", gm.MODES)
def test_a_bed_with_no_touching_pair_has_zero_rows(mode):
    bed = synthetic.fcc_bed((2, 2, 2), spacing=1.6, seed=3, vmax=0.2)
    cfg = dict(STYLES["hertz"], g=0.0, dt=1.0e-6, skin=0.25e-3, walls=[])
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute pl all pair/local dist force tag2")
    lmp.command("compute q all reduce %s c_pl[1] c_pl[2] c_pl[3]" % mode)
    lmp.command("run 0")
    assert len(lmp.contacts()["tag1"]) == 0
    got = lmp.compute_global("q")
    assert got.tolist() == [gm.reduce(mode, [])] * 3
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. block boundaries: 1, 257 and 864 atoms; compute ke and compute erotate/sphere

@pytest.mark.parametrize("n", [1, 257, 864])
def test_sizes_around_the_block_and_the_energy_computes(n):
    bed, cfg = _sized(n)
    lmp = dc.make_hip(bed, cfg)
    _groups(lmp)
    lmp.command("compute k all ke/atom")
    lmp.command("compute e all erotate/sphere/atom")
    for g in GROUPS:
        lmp.command("compute K_%s %s ke" % (g, g))
        lmp.command("compute E_%s %s erotate/sphere" % (g, g))
        for mode in gm.MODES:
            lmp.command("compute r_%s_%s %s reduce %s vx fy" % (mode, g, g, mode))
    lmp.command("run 5")
    st, k, e = lmp.get_state(), lmp.compute_atom("k"), lmp.compute_atom("e")
    assert k.shape == (n,) and k.all() and e.all()
    for g, mask in _masks(bed).items():
        K, E = lmp.compute_global("K_" + g), lmp.compute_global("E_" + g)
        assert K.shape == (1,) and E.shape == (1,)
        _check("ke over %s (n = %d)" % (g, n), "sum", K[0], k, mask)
        _check("erotate/sphere over %s (n = %d)" % (g, n), "sum", E[0], e, mask)
        for mode in gm.MODES:
            got = lmp.compute_global("r_%s_%s" % (mode, g))
            _check("vx over %s (n = %d)" % (g, n), mode, got[0], st["v"][:, 0], mask)
            _check("fy over %s (n = %d)" % (g, n), mode, got[1], st["f"][:, 1], mask)
    if n == 1:   # one term: the sum is the term, whatever the order
        assert lmp.compute_global("K_all")[0] == k[0] and lmp.compute_global("E_all")[0] == e[0]
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism and column independence

SEVENTEEN = "x y z vy vz fx fy fz c_k x y z vy vz fx fy vx"


def _independence_engine():
    bed, cfg = _sized(864)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute k all ke/atom")
    for mode in ("sum", "ave", "sumsq", "max"):
        lmp.command("compute a_%s all reduce %s vx" % (mode, mode))
        lmp.command("compute b_%s all reduce %s x y vx fz c_k" % (mode, mode))
        lmp.command("compute c_%s all reduce %s %s" % (mode, mode, SEVENTEEN))
    lmp.command("compute K all ke")
    lmp.command("run 10")
    return lmp


def test_two_fresh_engines_give_the_same_bits():
    out = []
    for _ in range(2):
        lmp = _independence_engine()
        out.append(b"".join(lmp.compute_global(name).tobytes() for name in ("a_sum", "b_ave", "c_sumsq", "c_sum", "K")))
        lmp.close()
    assert out[0] == out[1]


def test_a_columns_bits_do_not_depend_on_its_neighbours():
    lmp = _independence_engine()
    for mode in ("sum", "ave", "sumsq", "max"):
        alone = lmp.compute_global("a_" + mode)
        five = lmp.compute_global("b_" + mode)
        before = lmp.global_launches()["launches"]
        many = lmp.compute_global("c_" + mode)
        assert lmp.global_launches()["launches"] - before == 4, "17 columns: two gathers and two folds"
        assert alone.shape == (1,) and five.shape == (5,) and many.shape == (17,)
        assert alone.tobytes() == five[2:3].tobytes() == many[16:17].tobytes(), (mode, alone, five[2], many[16])
        # and the columns that appear twice in the set, in the first launch and across the two
        assert many[0:7].tobytes() == many[9:16].tobytes()
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. compute property/atom

def test_property_atom_is_the_state_and_reaches_dump_custom_and_ave_chunk(tmp_path):
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group two type 2")
    lmp.command("compute prop all property/atom " + " ".join(ATTRS))
    lmp.command("compute p1 two property/atom omegay")
    lmp.command("compute ch all chunk/atom bin/1d y lower 0.61e-3 units box")
    lmp.command("fix p all ave/chunk 1 1 1 ch c_prop[16] c_p1")
    path = tmp_path / "prop.dump"
    lmp.command("dump d all custom 25 %s id c_prop[4] c_prop[16] c_p1" % path)
    lmp.command("dump_modify d sort id")
    lmp.command("run 25")
    st, prop, p1 = lmp.get_state(), lmp.compute_atom("prop"), lmp.compute_atom("p1")
    n = len(bed["x"])
    r = 0.5 * np.asarray(bed["diameter"])
    mass = 4.0 * np.pi / 3.0 * r ** 3 * np.asarray(bed["density"])
    assert prop.shape == (n, 20) and p1.shape == (n,)
    want = dict(id=st["tag"].astype(np.float64), type=np.asarray(bed["type"], np.float64), radius=r, diameter=2.0 * r,
                x=st["x"][:, 0], y=st["x"][:, 1], z=st["x"][:, 2], vx=st["v"][:, 0], vy=st["v"][:, 1], vz=st["v"][:, 2],
                fx=st["f"][:, 0], fy=st["f"][:, 1], fz=st["f"][:, 2], omegax=st["omega"][:, 0], omegay=st["omega"][:, 1],
                omegaz=st["omega"][:, 2], tqx=st["torque"][:, 0], tqy=st["torque"][:, 1], tqz=st["torque"][:, 2])
    for k, a in enumerate(ATTRS):
        if a == "mass":   # (not in the state: the formula; at most eight roundings in each of the two evaluations)
            assert np.max(np.abs(prop[:, k] - mass) / mass) <= 8 * 2.0 ** -52
        else:
            assert (prop[:, k] == want[a]).all(), a
    mask = np.asarray(bed["type"]) == 2
    assert not p1[~mask].any() and (p1[mask] == st["omega"][mask, 1]).all()
    lmp.sync()
    fr = frames(str(path))
    assert [f[0] for f in fr] == [0, 25]
    assert fr[1][3] == [("%d %g %g %g \n" % (i + 1, prop[i, 3], prop[i, 15], p1[i])).encode() for i in range(n)]
    # as a value of fix ave/chunk: the chunk means of the column (norm all)
    out, ids = lmp.ave_chunk("p"), lmp.compute_atom("ch")
    assert out["step"] == 25 and out["names"] == ["c_prop[16]", "c_p1"]
    for j, col in enumerate((prop[:, 15], p1)):
        for c in range(len(out["count"])):
            sel = ids == c + 1
            assert out["count"][c] == sel.sum()
            if sel.any():
                scale = np.mean(np.abs(col[sel]))
                assert abs(out["values"][c, j] - np.mean(col[sel])) <= 1e-13 * (scale if scale > 0 else 1.0)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. fix ave/time

FIX_VALUES = ["c_r", "c_v[2]", "c_K"]


def _fix_engine():
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute r all reduce sum vx")
    lmp.command("compute v all reduce ave x y")
    lmp.command("compute K all ke")
    return lmp


def _now(lmp):
    return [lmp.compute_global("r")[0], lmp.compute_global("v")[1], lmp.compute_global("K")[0]]


@pytest.mark.parametrize("ave", ["one", "running", "window 2"])
@pytest.mark.parametrize("sched", [(2, 3, 10, 0), (10, 1, 10, 0), (5, 2, 10, 25)])
def test_time_averages_are_the_models(sched, ave):
    """a piecewise run; the model is fed compute_global() after each piece that ends on a sample step.  The pieces are `run 2`,
    and `run 1` for the schedule whose sample steps are odd (5 2 10 start 25: 25, 30, 35 ...)"""
    nevery, nrepeat, nfreq, start = sched
    lmp = _fix_engine()
    lmp.command("fix t all ave/time %d %d %d %s ave %s" % (nevery, nrepeat, nfreq, " ".join(FIX_VALUES), ave)
                + (" start %d" % start if start else ""))
    with pytest.raises(SfError, match="has made no output yet"):
        lmp.ave_time("t")
    end, piece = 60, (2 if nevery % 2 == 0 else 1)
    plan = gm.schedule(0, nevery, nrepeat, nfreq, end, start)
    assert len(plan) >= 4
    samples = {s for _, ss in plan for s in ss}
    outputs = {o for o, _ in plan}
    w = ave.split()
    model = gm.TimeAverager(3, nrepeat, w[0], int(w[1]) if len(w) > 1 else 0)
    lmp.command("run 0")
    step, gate, nout, worst = 0, [0.0] * 3, 0, 0.0
    mags = [0.0] * 3
    while True:
        if step in samples:
            vals = _now(lmp)
            model.add_sample(vals)
            mags = [m + abs(v) for m, v in zip(mags, vals)]
        if step in outputs:
            want = model.output()
            got = lmp.ave_time("t")
            assert got["step"] == step and got["names"] == FIX_VALUES
            gate = [max(g, nrepeat * gm.EPS * m) for g, m in zip(gate, mags)]   # (the largest block gate so far)
            mags = [0.0] * 3
            for j in range(3):
                err = abs(got["values"][j] - want[j])
                worst = max(worst, err)
                assert err <= gate[j], (step, j, got["values"][j], want[j], err, gate[j])
            nout += 1
        elif nout:
            assert lmp.ave_time("t")["step"] == max(o for o in outputs if o < step)
        if step >= end:
            break
        lmp.command("run %d" % piece)
        step += piece
    print("fix ave/time %s ave %s: %d outputs, worst |err| %.3e" % (sched, ave, nout, worst))
    assert nout == len(plan)
    lmp.close()


@pytest.mark.parametrize("sched", [(2, 3, 10, 0), (10, 1, 10, 0), (5, 2, 10, 25)])
def test_output_steps_of_one_uncut_run(tmp_path, sched):
    nevery, nrepeat, nfreq, start = sched
    lmp = _fix_engine()
    path = tmp_path / "t.txt"
    lmp.command("fix t all ave/time %d %d %d c_r file %s" % (nevery, nrepeat, nfreq, path) + (" start %d" % start if start else ""))
    lmp.command("run 60")
    body = open(path).read().splitlines()[2:]
    assert [int(ln.split()[0]) for ln in body] == [o for o, _ in gm.schedule(0, nevery, nrepeat, nfreq, 60, start)]
    assert lmp.ave_time("t")["step"] == 60
    lmp.close()


def test_files_are_the_models_text_and_unfix_stops_one(tmp_path):
    lmp = _fix_engine()
    vals = "c_r c_v[2]"
    p = {k: tmp_path / (k + ".txt") for k in ("plain", "over", "titles", "fmt", "gone")}
    lmp.command("fix plain all ave/time 2 3 10 %s file %s" % (vals, p["plain"]))
    lmp.command("fix over all ave/time 2 3 10 %s file %s overwrite" % (vals, p["over"]))
    lmp.command("fix titles all ave/time 2 3 10 %s file %s title1 \"# one two\" title2 '# three  four' title3 unused"
                % (vals, p["titles"]))
    lmp.command("fix fmt all ave/time 2 3 10 %s file %s format \" %%.10g\"" % (vals, p["fmt"]))
    lmp.command("fix gone all ave/time 2 3 10 %s file %s" % (vals, p["gone"]))
    words = vals.split()
    want = {"plain": gm.header("plain", words), "over": gm.header("over", words),
            "titles": gm.header("titles", words, "# one two", "# three  four"), "fmt": gm.header("fmt", words),
            "gone": gm.header("gone", words)}
    over_head = want["over"]
    for k in range(3):
        lmp.command("run 10")
        step = 10 * (k + 1)
        for name in want:
            if name == "gone" and k > 0:
                continue
            out = lmp.ave_time(name)
            assert out["step"] == step
            text = gm.line(step, out["values"], " %.10g" if name == "fmt" else " %g")
            want[name] = over_head + text if name == "over" else want[name] + text
        if k == 0:
            lmp.command("unfix gone")
            with pytest.raises(SfError, match="Could not find fix ave/time ID gone"):
                lmp.ave_time("gone")
        for name in want:
            assert open(p[name], "rb").read() == want[name].encode(), name
    assert want["gone"].count("\n") == 3 and want["plain"].count("\n") == 5 and want["over"].count("\n") == 3
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. thermo columns

def _thermo_rows(path):
    """[(header words, [row words])] of the thermo tables of a log"""
    tables, cur = [], None
    for ln in open(path).read().splitlines():
        if ln.startswith("Step "):
            cur = (ln.split(), [])
            tables.append(cur)
        elif ln.startswith("Loop time"):
            cur = None
        elif cur is not None and ln.strip():
            cur[1].append(ln)
    return tables


def test_thermo_columns_are_the_values_as_printed(tmp_path):
    bed, cfg = _small("hertz")
    n = len(bed["x"])
    lmp = dc.make_hip(bed, cfg)
    log = tmp_path / "log.lammps"
    lmp.command("log %s" % log)
    lmp.command("compute r all reduce sum vx")
    lmp.command("compute r2 all reduce max x y")
    lmp.command("compute ke all ke")
    lmp.command("thermo_style custom step c_r c_r2[2] c_ke")
    lmp.command("thermo 5")

    def last_row_is(norm, step):
        lmp.sync()
        head, rows = _thermo_rows(log)[-1]
        assert head == ["Step", "c_r", "c_r2[2]", "c_ke"]
        r, r2, ke = lmp.compute_global("r")[0], lmp.compute_global("r2")[1], lmp.compute_global("ke")[0]
        vals = [gm.thermo_value(r, True, norm, n), gm.thermo_value(r2, False, norm, n), gm.thermo_value(ke, True, norm, n)]
        assert rows[-1] == "%8d " % step + "".join(gm.thermo_cell(v) for v in vals), (rows[-1], vals)
        assert lmp.get_thermo("c_ke") == vals[2] and lmp.get_thermo("c_r") == vals[0] and lmp.get_thermo("c_r2[2]") == vals[1]
        return rows

    lmp.command("run 10")
    rows = last_row_is(True, 10)   # units lj: norm yes by default
    assert [int(r.split()[0]) for r in rows] == [0, 5, 10]
    lmp.command("thermo_modify norm no")
    lmp.command("run 0")
    last_row_is(False, 10)
    lmp.command("thermo_style custom step c_r c_r2[2] c_ke")   # (a new style: norm back to the default of the units)
    lmp.command("units si")
    lmp.command("run 5")
    last_row_is(False, 15)
    lmp.command("thermo_modify norm yes")
    lmp.command("run 0")
    last_row_is(True, 15)
    with pytest.raises(SfError, match="unknown thermo keyword"):
        lmp.get_thermo("c_none")
    lmp.close()


def test_no_kernel_of_the_global_computes_runs_for_a_style_without_c_columns(tmp_path):
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("log %s" % (tmp_path / "log.lammps"))
    lmp.command("compute r all reduce sum vx")
    lmp.command("compute K all ke")
    lmp.command("thermo_style custom step ke fmax")
    lmp.command("thermo 5")
    lmp.command("run 20")
    assert lmp.global_launches() == dict(launches=0, host_copies=0)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. passivity

def _passive_run(tmp_path, name, extras):
    bed, cfg = _small("hertz", types=_third)
    lmp = dc.make_hip(bed, cfg)
    dump = tmp_path / (name + ".dump")
    lmp.command("dump d all custom 5 %s id x y z vx vy vz fx fy fz" % dump)
    lmp.command("dump_modify d sort id")
    if extras:
        lmp.command("log %s" % (tmp_path / (name + ".log")))
        lmp.command("group two type 2")
        lmp.command("compute k all ke/atom")
        lmp.command("compute s all stress/atom")
        lmp.command("compute pl all pair/local force p4")
        lmp.command("compute r1 all reduce sum vx vy vz")
        lmp.command("compute r2 two reduce max y c_k")
        lmp.command("compute r3 all reduce ave c_s[1] c_s[2] c_s[3]")
        lmp.command("compute r4 all reduce max c_pl[1] c_pl[2]")
        lmp.command("compute K all ke")
        lmp.command("compute E two erotate/sphere")
        lmp.command("fix t all ave/time 5 2 10 c_r1[1] c_r2[2] c_r3[1] c_r4[1] c_K c_E file %s" % (tmp_path / (name + ".txt")))
        lmp.command("thermo_style custom step c_r1[2] c_r4[2] c_K")
        lmp.command("thermo 5")
    for piece in (55, 30, 45):
        lmp.command("run %d" % piece)
        if extras:
            for cid in ("r1", "r2", "r3", "r4", "K", "E"):
                lmp.compute_global(cid)
    lmp.sync()
    st, hist, nb = lmp.get_state(), lmp.history(), lmp.info().nbuilds
    if extras:
        assert lmp.global_launches()["launches"] > 0 and lmp.ave_time("t")["step"] == 130
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
    assert one[4] == two[4] and one[4].count(b"\n") == 2 + 13


# ---------------------------------------------------------------------------------------------------------------------
# 8. launch accounting

def _twelve(lmp):
    lmp.command("compute a all reduce sum x y z vx")
    lmp.command("compute b all reduce max vx vy vz fx")
    lmp.command("compute c all reduce sumsq fx fy fz")
    lmp.command("compute K all ke")
    lmp.command("fix f1 all ave/time 5 2 10 c_a[1] c_a[2] c_b[1] c_K")
    lmp.command("fix f2 all ave/time 5 2 10 c_b[4] c_c[1] c_c[3]")


def test_two_fixes_and_a_thermo_line_cost_two_launches_per_sample_step(tmp_path):
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("log %s" % (tmp_path / "log.lammps"))
    _twelve(lmp)
    lmp.command("thermo_style custom step c_a[3] c_a[4] c_b[2] c_b[3] c_c[2]")
    lmp.command("thermo 5")
    lmp.command("run 0")
    before = lmp.global_launches()
    lmp.command("run 20")
    after = lmp.global_launches()
    # the setup line (a, b, c: 11 columns), then the steps 5, 10, 15, 20 (12 columns): one gather and one fold each
    assert after["launches"] - before["launches"] == 2 + 4 * 2
    # copies: three computes per thermo line (five lines), two fixes at each of the outputs 10 and 20
    assert after["host_copies"] - before["host_copies"] == 3 * 5 + 2 * 2
    lmp.close()


def test_a_sample_that_is_not_an_output_makes_no_host_copy():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    _twelve(lmp)
    lmp.command("run 4")
    assert lmp.global_launches() == dict(launches=0, host_copies=0)   # (no sample yet: nothing ran)
    lmp.command("run 1")   # step 5: a sample of both fixes
    assert lmp.global_launches() == dict(launches=2, host_copies=0)
    lmp.command("run 5")   # step 10: the second sample and the output
    assert lmp.global_launches() == dict(launches=4, host_copies=2)
    want = [lmp.compute_global("a")[0], lmp.compute_global("a")[1], lmp.compute_global("b")[0], lmp.compute_global("K")[0]]
    assert lmp.global_launches() == dict(launches=4, host_copies=6)   # (fresh values: copies only)
    assert lmp.ave_time("f1")["step"] == 10 and len(want) == len(lmp.ave_time("f1")["values"])
    lmp.close()


def test_no_consumer_means_no_launch():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("compute a all reduce sum x y z vx")
    lmp.command("compute K all ke")
    lmp.command("compute p all property/atom radius")
    lmp.command("run 20")
    assert lmp.global_launches() == dict(launches=0, host_copies=0)
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals

REFUSALS = [
    ("compute x all reduce sum", "Illegal compute reduce command"),
    ("compute x all reduce total vx", "Illegal compute reduce command"),
    ("compute x all reduce sum c_k[", "Illegal compute reduce command"),
    ("compute x all reduce sum vx replace 1 2", "replace is not supported"),
    ("compute x all reduce sum vx inputs local", "inputs is not supported"),
    ("compute x all reduce sum f_1", "f_1 is not supported"),
    ("compute x all reduce sum v_a", "v_a is not supported"),
    ("compute x all reduce sumabs vx", "sumabs is not supported"),
    ("compute x all reduce/region box sum vx", "compute reduce/region is not supported"),
    ("compute x all reduce sum c_nope", "Compute ID for compute reduce does not exist"),
    ("compute x all reduce sum c_s", "Compute reduce compute does not calculate a per-atom vector"),
    ("compute x all reduce sum c_k[1]", "Compute reduce compute does not calculate a per-atom array"),
    ("compute x all reduce sum c_s[7]", "Compute reduce compute array is accessed out-of-range"),
    ("compute x all reduce sum c_pl", "Compute reduce compute does not calculate a local vector"),
    ("compute x all reduce sum c_pl[3]", "Compute reduce compute array is accessed out-of-range"),
    ("compute x all reduce sum c_r", "Compute reduce compute calculates global values"),
    ("compute x nogroup reduce sum vx", "nogroup"),
    ("compute r all reduce sum vx", "Reuse of compute ID"),
    ("compute k all ke", "Reuse of compute ID"),
    ("compute x all ke extra", "Illegal compute ke command"),
    ("compute x all erotate/sphere extra", "Illegal compute erotate/sphere command"),
    ("compute x all temp", "Invalid compute style temp"),
    ("compute x all pressure NULL", "Invalid compute style pressure"),
    ("compute x all msd", "reduce, ke and erotate/sphere"),
    ("compute x all property/atom", "Illegal compute property/atom command"),
    ("compute x all property/atom mol", "Invalid keyword in compute property/atom command: mol"),
    ("uncompute nope", "Could not find compute ID to delete"),
    ("uncompute k", "a compute reduce still uses this compute"),
    ("uncompute pl", "a compute reduce still uses this compute"),
    ("uncompute r", "a fix ave/time still uses this compute"),
    ("uncompute K", "thermo_style custom still names this compute"),
    ("fix x all ave/time 2 3 10", "Illegal fix ave/time command"),
    ("fix x all ave/time 3 3 10 c_r", "Illegal fix ave/time command"),
    ("fix x all ave/time 2 6 10 c_r", "Illegal fix ave/time command"),
    ("fix x all ave/time 2 3 10 c_nope", "Compute ID for fix ave/time does not exist"),
    ("fix x all ave/time 2 3 10 c_rv", "Fix ave/time compute does not calculate a scalar"),
    ("fix x all ave/time 2 3 10 c_k", "Fix ave/time compute does not calculate a scalar"),
    ("fix x all ave/time 2 3 10 c_r1[1]", "Fix ave/time compute does not calculate a vector"),
    ("fix x all ave/time 2 3 10 c_rv[3]", "Fix ave/time compute vector is accessed out-of-range"),
    ("fix x all ave/time 2 3 10 f_t", "f_t is not supported"),
    ("fix x all ave/time 2 3 10 v_t", "v_t is not supported"),
    ("fix x all ave/time 2 3 10 c_r mode vector", "mode vector is not supported"),
    ("fix x all ave/time 2 3 10 c_r off 1", "off is not supported"),
    ("fix x all ave/time 2 3 10 c_r format %s", "is not one %g-class conversion"),
    ("fix x all ave/time 2 3 10 c_r title1 \"# open", "Unbalanced quotes"),
    ("fix t all ave/time 2 3 10 c_r", "this fix ID is in use"),
    ("fix p all ave/time 2 3 10 c_r", "this fix ID is in use"),
    ("fix t all ave/chunk 2 3 10 ch vx", "this fix ID is in use"),
    ("fix x all ave/chunk 2 3 10 ch c_r", "Fix ave/chunk compute does not calculate per-atom values"),
    ("fix x all ave/chunk 2 3 10 r vx", "Fix ave/chunk does not use chunk/atom compute"),
    ("unfix nope", "only a fix ave/chunk can be removed"),
    ("thermo_style custom step c_nope", "Could not find thermo custom compute ID"),
    ("thermo_style custom step c_rv", "Thermo compute does not compute scalar"),
    ("thermo_style custom step c_k", "Thermo compute does not compute scalar"),
    ("thermo_style custom step c_r1[1]", "Thermo compute does not compute vector"),
    ("thermo_style custom step c_rv[3]", "Thermo compute vector is accessed out-of-range"),
    ("thermo_style custom step c_r[0]", "Invalid keyword in thermo_style custom command"),
    ("thermo_style custom step f_t", "Invalid keyword in thermo_style custom command"),
    ("thermo_style custom step v_t", "Invalid keyword in thermo_style custom command"),
    ("dump x all custom 10 {p} id c_r", "Dump custom compute does not compute per-atom info"),
    ("dump x all local 10 {p} index c_r", "Dump local compute does not compute local info"),
]


def _refusal_engine():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    for line in ("compute k all ke/atom", "compute s all stress/atom", "compute pl all pair/local dist force",
                 "compute ch all chunk/atom bin/1d y lower 0.61e-3 units box", "compute r all reduce sum vx c_k c_pl[1]",
                 "compute rv all reduce sum vx vy", "compute r1 all reduce max y", "compute K all ke",
                 "fix t all ave/time 2 3 10 c_r[1] c_r1", "fix p all ave/chunk 2 3 10 ch vx", "thermo_style custom step c_K"):
        lmp.command(line)
    return lmp


def test_refusals_by_message(tmp_path):
    lmp = _refusal_engine()
    for line, msg in REFUSALS:
        line = line.replace("{p}", str(tmp_path / "x.dump"))
        with pytest.raises(SfError) as e:
            lmp.command(line)
        assert msg in str(e.value), (line, str(e.value))
    with pytest.raises(SfError, match="does not calculate per-atom values"):
        lmp.compute_atom("r")
    with pytest.raises(SfError, match="does not calculate a global scalar or vector"):
        lmp.compute_global("k")
    with pytest.raises(SfError, match="Could not find compute ID nope"):
        lmp.compute_global("nope")
    with pytest.raises(SfError, match="Could not find fix ave/time ID nope"):
        lmp.ave_time("nope")
    with pytest.raises(SfError, match="Could not find fix ave/time ID p"):
        lmp.ave_time("p")
    # nothing above changed anything: the commands go on working
    lmp.command("run 0")
    assert lmp.compute_global("r").shape == (3,) and lmp.compute_global("K").shape == (1,)
    lmp.command("unfix t")
    lmp.command("uncompute r1")
    lmp.command("thermo_style one")
    lmp.command("uncompute K")
    lmp.command("uncompute r")
    lmp.command("uncompute k")
    lmp.close()


def test_a_decomposed_handle_is_refused_at_every_command(tmp_path):
    lmp = _refusal_engine()
    lmp.command("run 0")
    _decompose(lmp)
    for line, msg in [("compute x all reduce sum vx", "compute reduce: one rank only"),
                      ("compute x all ke", "compute ke: one rank only"),
                      ("compute x all erotate/sphere", "compute erotate/sphere: one rank only"),
                      ("compute x all property/atom radius", "compute property/atom: one rank only"),
                      ("fix x all ave/time 2 3 10 c_r1", "fix ave/time: one rank only"),
                      ("thermo_style custom step c_K", "c_ columns on one rank only")]:
        with pytest.raises(SfError) as e:
            lmp.command(line)
        assert msg in str(e.value), (line, str(e.value))
    with pytest.raises(SfError, match="compute reduce: one rank only"):
        lmp.compute_global("r1")
    with pytest.raises(SfError, match="compute ke: one rank only"):
        lmp.compute_global("K")
    lmp.close()


def test_print_the_worst_measured_errors():
    """(runs last in this file: the worst |error| / gate seen by the cases above, per mode)"""
    print("worst error over gate: " + ", ".join("%s %.3f" % (m, WORST.get(m, 0.0)) for m in gm.MODES))
    assert all(v <= 1.0 for v in WORST.values())
