"""Periodic image counts and what rests on them (csrc/sf_unmap.h, sf_displace.hip, the styles in
sf_compute_atom.hip and sf_global.hip): xu yu zu ix iy iz of `compute
property/atom`, `compute displace/atom`, `compute com`, Lammps.images() -- against the NumPy
statement tests/displace_model.py (held to hand-computed answers by tests/test_displace_model.py).

The model is fed the engine's own bits (get_local_info(), images()), so what is under test is the bookkeeping of the wraps,
the references and, for com, the order of the summation: per-atom values compare with ==; a sum of N terms is held
to 2 N 2^-53 sum |term| (each of the two summations is within N 2^-53 sum |term| of the exact sum), stated from N below.

The beds: eight grains in free flight in a box of side 4 (every number dyadic: every operation exact); a sheared bed of
400 grains on a floor at z = 0, periodic in x and y, under tilted gravity, streaming through the x face; the 108-grain bed of
tests/test_contacts_gpu.py."""
import re

import numpy as np
import pytest

from sedifoam_amd import Lammps, SfError, synthetic
from tests import dem_cases as dc
from tests import displace_model as dm
from tests import global_model as gm
from tests import histo_model as hm
from tests.test_compute_atom_gpu import _decompose
from tests.test_contacts_gpu import _small
from tests.test_dump_gpu import frames

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _snap(lmp):
    """the owned atoms by tag: x, the image counts, the model's unwrapped position; `order`: the tags in the engine's order"""
    li, im = lmp.get_local_info(), lmp.images()
    assert im.shape == (len(li["tag"]), 3) and im.dtype == np.int32
    o = np.argsort(li["tag"], kind="stable")
    lo, hi = lmp.get_local_domain()[0::2], lmp.get_local_domain()[1::2]
    return dict(tag=li["tag"][o], x=li["x"][o], v=li["v"][o], image=im[o], xu=dm.unmap(li["x"][o], im[o], hi - lo),
                order=li["tag"].copy(), prd=hi - lo)


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. free flight, exact

FF_X = [[3.5, 1.75, 1.5], [2.25, 3.3125, 3.625], [1.1875, 1.0, 2.0625], [2.3125, 1.0, 1.375], [3.6875, 3.0, 3.375],
        [2.125, 1.5, 0.75], [2.6875, 2.0625, 1.625], [0.9375, 2.0, 0.1875]]
FF_V = [[0.0, 0.0, 0.0], [-1.0, -4.0, -4.0], [2.0, 1.0, -4.0], [2.0, 0.0, -4.0], [-4.0, 0.0, 1.0], [0.0, -4.0, 0.0],
        [2.0, -4.0, 1.0], [2.0, 1.0, -1.0]]


def test_free_flight_is_exact():
    """8 grains that never come within three diameters of each other (checked when the numbers were chosen, and below by
    their unchanged velocities), box [0, 4)^3 periodic in x y z, positions on a 2^-4 grid, velocities from {-4, -1, 0, 1, 2},
    dt = 2^-10, no force: x + dt v, x -+ L, x + ix L and xu - x0 are all exact, so every comparison is of bits"""
    x0, v0 = np.array(FF_X), np.array(FF_V)
    L, dt = 4.0, 2.0 ** -10
    assert (x0 * 16 == np.round(x0 * 16)).all() and set(v0.ravel()) == {-4.0, -1.0, 0.0, 1.0, 2.0} and not v0[0].any()
    lmp = Lammps()
    lmp.set_box([0.0, 0.0, 0.0], [L, L, L])
    lmp.create_atoms(x0, np.full(8, 0.125), np.full(8, 1.0), v=v0)
    for line in ["atom_style sphere", "boundary p p p", "newton off", "communicate single vel yes", "neighbor 0.25 bin",
                 "neigh_modify delay 0", "pair_style gran/hooke/history 1000.0 NULL 1.0 NULL 0.5 1", "pair_coeff * *",
                 "timestep %.17g" % dt, "fix 1 all nve/sphere",
                 "compute d all displace/atom", "compute p all property/atom xu yu zu ix iy iz x y z"]:
        lmp.command(line)
    before = _snap(lmp)
    assert _same(before["x"], x0) and not before["image"].any()
    jumped = False
    for q in range(1, 9):
        lmp.command("run 1024")
        s = _snap(lmp)
        want = x0 + (q * 1024 * dt) * v0
        assert _same(s["v"], v0), q                                     # (no contact ever happened)
        assert ((s["x"] >= -0.25) & (s["x"] < L + 0.25)).all()          # (wrapped at a rebuild: out by less than the skin)
        assert _same(s["xu"], want), (q, s["xu"] - want)                # xu == x + ix L == x0 + n dt v
        p = lmp.compute_atom("p")
        assert _same(p[:, 0:3], want) and (p[:, 3:6] == s["image"]).all() and _same(p[:, 6:9], s["x"])
        d = lmp.compute_atom("d")
        assert _same(d[:, 0:3], want - x0)
        assert _same(d[:, 3], dm.displace(want, x0)[:, 3])
        jumped = jumped or bool((np.abs(s["x"] - before["x"]) > 0.5 * L).any())
        before = s
    # conditions, not measurements
    assert np.abs(s["image"]).max() >= 3 and s["image"].max() > 0 and s["image"].min() < 0
    assert jumped
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. a flowing bed

N_FLOW = 400


def _flow_bed():
    """400 grains (5 x 4 x 5 fcc cells) on a floor at z = 0, periodic in x and y; a sheared stream along +x, 0.5 m/s at the
    floor to 2 m/s at the top (one box length is 6.9 mm: in 4 ms most grains leave through the x face), every third grain of
    type 2"""
    bed = synthetic.fcc_bed((5, 4, 5), seed=21, vmax=0.05)
    swap = [0, 2, 1]                                   # (the generator's floor is y = 0)
    for k in ("x", "v"):
        bed[k] = np.ascontiguousarray(bed[k][:, swap])
    bed["boxlo"], bed["boxhi"] = bed["boxlo"][swap], bed["boxhi"][swap]
    bed["periodic"] = (1, 1, 0)
    z = bed["x"][:, 2]
    bed["v"][:, 0] += 0.5 + 1.5 * z / z.max()
    bed["type"] = (1 + (np.arange(len(z)) % 3 == 0)).astype(np.int32)
    assert len(z) == N_FLOW
    return bed


def _flow_engine(bed, outputs=()):
    lmp = Lammps()
    lmp.set_box(bed["boxlo"], bed["boxhi"])
    lmp.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"], type_=bed["type"])
    kn, gam, xmu = 1.0e7, 0.5, 0.1
    for line in ["atom_style sphere", "boundary p p f", "newton off", "communicate single vel yes", "neighbor 0.25e-3 bin",
                 "neigh_modify delay 0", "pair_style gran/hertzFix/history %.17g NULL %.17g NULL %.17g 1" % (kn, gam, xmu),
                 "pair_coeff * *", "timestep 1.0e-6", "group two type 2", "group none type 3", "fix 1 all nve/sphere",
                 "fix 2 all gravity 9.81 vector 0.5 0 -0.8660254037844386",
                 "fix floor all wall/granFix %.17g NULL %.17g NULL %.17g 1 zplane 0.0 NULL" % (kn, gam, xmu)]:
        lmp.command(line)
    for line in outputs:
        lmp.command(line)
    return lmp


# (m, m2: the mean squared displacement, as a compute reduce over the columns of displace/atom)
FLOW_COMPUTES = ["compute d all displace/atom", "compute d2 two displace/atom", "compute m all reduce avesq c_d[1] c_d[2] c_d[3] c_d[4]",
                 "compute m2 two reduce avesq c_d2[1] c_d2[2] c_d2[3] c_d2[4]", "compute c all com", "compute c2 two com"]


def _flow_run():
    """4000 steps, a query every 200: the snapshots and every compute's values at each"""
    bed = _flow_bed()
    lmp = _flow_engine(bed, FLOW_COMPUTES)
    r = 0.5 * bed["diameter"]
    out = dict(bed=bed, mass=4.0 * np.pi / 3.0 * r ** 3 * bed["density"], snaps=[], vals=[])
    for q in range(21):
        if q:
            lmp.command("run 200")
        out["snaps"].append(_snap(lmp))
        vals = {c: lmp.compute_atom(c) for c in ("d", "d2")}
        vals.update({c: lmp.compute_global(c) for c in ("m", "m2", "c", "c2")})
        out["vals"].append(vals)
    lmp.close()
    return out


@pytest.fixture(scope="module")
def flow():
    return _flow_run()


def test_flowing_bed_really_flows_and_resorts(flow):
    first, last = flow["snaps"][0], flow["snaps"][-1]
    assert (first["tag"] == np.arange(1, N_FLOW + 1)).all() and (last["tag"] == first["tag"]).all()
    wrapped = np.abs(last["image"][:, 0]) >= 1
    print("atoms with |ix| >= 1 at the end: %d of %d; ix from %d to %d" % (wrapped.sum(), N_FLOW, last["image"][:, 0].min(),
                                                                            last["image"][:, 0].max()))
    assert wrapped.sum() >= 0.05 * N_FLOW
    assert first["order"].tolist() != last["order"].tolist()            # a re-sort really happened
    assert not last["image"][:, 2].any()                                # z is not periodic
    Lx = first["prd"][0]
    for a, b in zip(flow["snaps"][:-1], flow["snaps"][1:]):             # continuity: no unwrapped jump
        assert np.abs(b["xu"] - a["xu"]).max() < 0.25 * Lx
    assert max(np.abs(b["x"][:, 0] - a["x"][:, 0]).max() for a, b in zip(flow["snaps"][:-1], flow["snaps"][1:])) > 0.5 * Lx


def test_flowing_bed_displace_atom_is_the_model_to_the_bit(flow):
    x0 = flow["snaps"][0]["xu"]
    two = np.asarray(flow["bed"]["type"]) == 2
    assert _same(x0, flow["bed"]["x"])
    for q, (s, v) in enumerate(zip(flow["snaps"], flow["vals"])):
        assert v["d"].shape == (N_FLOW, 4)
        assert _same(v["d"], dm.displace(s["xu"], x0)), q
        assert _same(v["d2"], dm.displace(s["xu"], x0, in_group=two)), q
    # further than any difference of two wrapped coordinates could show
    assert np.abs(flow["vals"][-1]["d"][:, 0]).max() > 0.5 * flow["snaps"][0]["prd"][0]


def test_flowing_bed_com_and_msd_are_the_model_within_the_bound_of_reordering(flow):
    """com: |got - want| <= 2 N 2^-53 sum |m xu| / sum m, a quotient of sums of N terms whose additions come in another
    order.  The mean squared displacement is `compute reduce avesq` over the columns of displace/atom, held to that
    compute's own gate (tests/global_model.py: the same 2 n 2^-53 sum |term| over the count, and the divisions)"""
    mass = flow["mass"]
    two = np.asarray(flow["bed"]["type"]) == 2
    worst = 0.0
    for q, (s, v) in enumerate(zip(flow["snaps"], flow["vals"])):
        xu = s["xu"]
        for name, mask in (("c", None), ("c2", two)):
            n = N_FLOW if mask is None else int(mask.sum())
            sel = slice(None) if mask is None else mask
            want = dm.com(xu, mass, in_group=mask)
            bound = 2 * n * EPS * np.abs(xu[sel] * mass[sel, None]).sum(axis=0) / mass[sel].sum()
            err = np.abs(v[name] - want)
            worst = max(worst, float(np.max(err / bound)))
            assert v[name].shape == (3,) and (err <= bound).all(), (q, name, v[name], want, err, bound)
        for name, col, mask in (("m", "d", None), ("m2", "d2", two)):
            assert v[name].shape == (4,)
            for k in range(4):
                want, gate = gm.reduce("avesq", v[col][:, k], mask), gm.gate("avesq", v[col][:, k], mask)
                assert abs(v[name][k] - want) <= gate, (q, name, k, v[name][k], want, gate)
    print("com over 21 queries: worst |err| / bound %.3e" % worst)
    assert flow["vals"][0]["m"].tolist() == [0.0] * 4 and flow["vals"][-1]["m"][3] > flow["vals"][-1]["m"][0] > 0.0
    # the centre of mass follows the stream through the periodic face: further than the box is long would be a jump back
    cx = np.array([v["c"][0] for v in flow["vals"]])
    assert (np.diff(cx) > 0.0).all() and cx[-1] - cx[0] > 0.5 * flow["snaps"][0]["prd"][0]


def test_two_runs_give_the_same_bits(flow):
    again = _flow_run()
    for a, b in zip(flow["vals"], again["vals"]):
        for k in a:
            assert _same(a[k], b[k]), k
    assert (flow["snaps"][-1]["image"] == again["snaps"][-1]["image"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. passive

def _state_bits(lmp):
    st, h = lmp.get_state(), lmp.history()
    return ([st[k].tobytes() for k in ("x", "v", "omega", "f", "torque", "tag")], sorted((k, v.tobytes()) for k, v in h.items()),
            lmp.wall_shear(0).tobytes())


def test_the_outputs_are_passive(tmp_path):
    """the same bed with the computes, the queries and a dump of their columns every 100 steps, and without any of them:
    the same bits of the state, the history and the wall's history.  The bare run keeps a dump of `id x y z` on the same
    schedule, as the passivity tests of sections 13 to 16 do: an output step ends a piece of the run, and a piece ends with
    the second half-kick of its last step and begins with the first of the next, each rounded on its own.  The bare engine
    never makes an image table, so the wrap kernel runs there with its null pointer"""
    bed = _flow_bed()
    path = tmp_path / "u.dump"
    watched = _flow_engine(bed, ["compute d all displace/atom", "compute c all com", "compute p all property/atom xu yu zu ix iy iz",
                                 "compute m all reduce avesq c_d[4]",
                                 "dump u all custom 100 %s id c_p[1] c_p[2] c_p[3] c_p[4] c_p[5] c_p[6] c_d[4]" % path])
    plain = _flow_engine(bed, ["dump u all custom 100 %s id x y z" % (tmp_path / "bare.dump")])
    for _ in range(5):
        watched.command("run 200")
        plain.command("run 200")
        watched.compute_global("m"), watched.compute_global("c"), watched.compute_atom("d"), watched.images()
    a, b = _state_bits(watched), _state_bits(plain)
    assert len(a[1]) > N_FLOW and a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    # the frames hold what the queries return
    s, d = _snap(watched), watched.compute_atom("d")
    watched.sync()
    fr = frames(str(path))
    assert [f[0] for f in fr] == list(range(0, 1001, 100))
    rows = {int(r.split(b" ")[0]): r for r in fr[-1][3]}
    assert len(rows) == N_FLOW
    for t in range(1, N_FLOW + 1):
        k = t - 1
        want = "%d %g %g %g %g %g %g %g \n" % (t, s["xu"][k, 0], s["xu"][k, 1], s["xu"][k, 2], s["image"][k, 0], s["image"][k, 1],
                                              s["image"][k, 2], d[k, 3])
        assert rows[t] == want.encode(), t
    assert (s["image"][:, 0] == 1).any()                                       # (some grain has gone round)
    watched.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the consumers take the new values like any other

def test_every_consumer_gives_the_numbers_of_the_queries(tmp_path):
    bed = _flow_bed()
    path, log = tmp_path / "p.dump", tmp_path / "log.lammps"
    dz = 0.7e-3
    lmp = _flow_engine(bed, ["log %s" % log, "compute d all displace/atom", "compute c all com", "compute pu all property/atom xu ix",
                             "compute r all reduce max c_d[4]", "fix t all ave/time 300 1 300 c_c[1]",
                             "thermo_style custom step c_c[1] c_r", "thermo 300",
                             "fix h all ave/histo 300 1 300 0 4e-4 8 c_d[1] mode vector",
                             "compute ch all chunk/atom bin/1d z lower %r units box" % dz,
                             "fix p all ave/chunk 300 1 300 ch c_d[1]",
                             "dump u all custom 300 %s id c_pu[1] c_pu[2]" % path, "dump_modify u sort id"])
    lmp.command("run 300")
    s, d, c = _snap(lmp), lmp.compute_atom("d"), lmp.compute_global("c")
    assert d[:, 3].max() > 0.0 and c[0] > 0.0
    assert lmp.compute_global("r")[0] == d[:, 3].max()                                   # compute reduce
    out = lmp.ave_time("t")
    assert out["step"] == 300 and out["names"] == ["c_c[1]"] and out["values"][0] == c[0]   # fix ave/time
    assert lmp.get_thermo("c_c[1]") == c[0] and lmp.get_thermo("c_r") == d[:, 3].max()       # thermo (com is intensive)
    h = lmp.ave_histo("h")                                                                # fix ave/histo
    want = hm.bin_values(hm.Bins(0.0, 4e-4, 8), d[:, 0])
    assert h["step"] == 300 and h["count"].tolist() == want.count.tolist() and h["total"] == want.total > 0
    assert h["missing"] == want.missing and h["min"] == want.min and h["max"] == want.max
    ch, ids = lmp.ave_chunk("p"), lmp.compute_atom("ch")                                  # fix ave/chunk
    assert ch["step"] == 300 and ch["names"] == ["c_d[1]"] and len(ch["count"]) >= 4
    for c in range(len(ch["count"])):
        sel = ids == c + 1
        assert ch["count"][c] == sel.sum()
        if sel.any():   # a mean of n terms, added in another order
            assert abs(ch["values"][c, 0] - np.mean(d[sel, 0])) <= 2 * sel.sum() * EPS * np.abs(d[sel, 0]).sum() / sel.sum()
    pu = lmp.compute_atom("pu")                                                           # property/atom through dump custom
    assert _same(pu[:, 0], s["xu"][:, 0]) and (pu[:, 1] == s["image"][:, 0]).all() and s["image"][:, 0].any()
    lmp.sync()
    fr = frames(str(path))
    assert [f[0] for f in fr] == [0, 300]
    assert fr[1][3] == [("%d %g %g \n" % (i + 1, pu[i, 0], pu[i, 1])).encode() for i in range(N_FLOW)]
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. atoms created and deleted; computes defined late and again

def test_created_atoms_start_at_zero_and_the_others_keep_their_reference():
    bed, cfg = _small("hertz")
    bed["v"][:, 0] += 1.0
    n = len(bed["x"])
    lmp = dc.make_hip(bed, cfg)
    for line in ("compute d all displace/atom", "compute m all reduce avesq c_d[1] c_d[2] c_d[3]", "compute c all com",
                 "compute pm all property/atom mass"):
        lmp.command(line)
    s0 = _snap(lmp)
    ref = {int(t): s0["xu"][k] for k, t in enumerate(s0["tag"])}
    lmp.command("run 60")
    gone = [5, 17, 60]
    lmp.delete_particle(gone)
    top = float(bed["x"][:, 1].max())
    pos = np.array([[1.0e-3, top + 2.0e-3, 1.0e-3], [2.5e-3, top + 2.0e-3, 2.0e-3]])
    new = [17, n + 7]                                       # a reused tag and a tag beyond every earlier one
    lmp.create_particle(pos, new, 1.0e-3, 2650.0, 1, [0.3, 0.0, 0.1])
    s1 = _snap(lmp)
    assert s1["tag"].tolist() == sorted((set(range(1, n + 1)) - set(gone)) | set(new))
    is_new = np.isin(s1["tag"], new)
    assert not s1["image"][is_new].any() and _same(s1["x"][is_new], pos)
    for t, x in zip(s1["tag"][is_new], s1["xu"][is_new]):
        ref[int(t)] = x
    x0 = np.array([ref[int(t)] for t in s1["tag"]])
    d = lmp.compute_atom("d")
    assert d[is_new].tolist() == [[0.0] * 4] * 2            # exactly zero at creation
    assert _same(d, dm.displace(s1["xu"], x0)) and np.abs(d[~is_new, 0]).min() > 0.0
    lmp.command("run 60")
    s2 = _snap(lmp)
    d = lmp.compute_atom("d")
    assert _same(d, dm.displace(s2["xu"], x0))              # the new atoms from where they were made, the others as before
    assert (d[is_new, 0] > 0.0).all()
    nn = len(s2["tag"])
    m = lmp.compute_global("m")                             # the mean squared displacement, through compute reduce
    for k in range(3):
        assert abs(m[k] - gm.reduce("avesq", d[:, k])) <= gm.gate("avesq", d[:, k])
    # the centre of mass counts the atoms that are there now, the new ones with their own mass
    mass, c = lmp.compute_atom("pm"), lmp.compute_global("c")
    want = dm.com(s2["xu"], mass)
    assert (np.abs(c - want) <= 2 * nn * EPS * np.abs(s2["xu"] * mass[:, None]).sum(axis=0) / mass.sum()).all(), (c, want)
    # a compute defined after a run: its reference is the position at its definition
    lmp.command("compute late all displace/atom")
    assert not lmp.compute_atom("late").any()
    lmp.command("run 20")
    s3 = _snap(lmp)
    assert _same(lmp.compute_atom("late"), dm.displace(s3["xu"], s2["xu"]))
    assert _same(lmp.compute_atom("d"), dm.displace(s3["xu"], x0))
    # uncompute, then the same ID again: a fresh reference
    lmp.command("uncompute late")
    with pytest.raises(SfError, match="Could not find compute ID late"):
        lmp.compute_atom("late")
    lmp.command("compute late all displace/atom")
    assert not lmp.compute_atom("late").any()
    lmp.command("run 10")
    s4 = _snap(lmp)
    assert _same(lmp.compute_atom("late"), dm.displace(s4["xu"], s3["xu"])) and lmp.compute_atom("late")[:, 3].min() > 0.0
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. what is refused

NEEDS_IMAGES = ["compute x all displace/atom", "compute x all com", "compute x all property/atom x ix",
                "compute x all property/atom zu"]


@pytest.mark.parametrize("line", NEEDS_IMAGES)
def test_refused_with_rigid_bodies_and_on_more_than_one_rank(line, tmp_path):
    bed, cfg = _small("hertz")
    line = line.format(p=tmp_path / "r.dump")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("fix r all rigid/nve single")
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.command(line)
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.images()
    lmp.close()
    lmp = dc.make_hip(bed, cfg)
    _decompose(lmp)
    with pytest.raises(SfError, match="one rank"):
        lmp.command(line)
    with pytest.raises(SfError, match="one rank"):
        lmp.images()
    lmp.close()


@pytest.mark.parametrize("line,msg", [
    ("compute x all displace/atom extra", "Illegal compute displace/atom command"),
    ("compute x all com extra", "Illegal compute com command"),
    ("compute x all property/atom xs", "Invalid keyword in compute property/atom command: xs"),
    ("compute x nogroup com", "Could not find group ID"),
    ("dump x all custom 10 {p} id xs", "Invalid attribute xs in dump custom command"),
    ("dump x all custom 10 {p} id xsu", "Invalid attribute xsu in dump custom command"),
    ("compute r all reduce sum c_c", "Compute reduce compute calculates global values"),
    ("fix t all ave/time 2 3 10 c_c", "Fix ave/time compute does not calculate a scalar"),
    ("fix t all ave/time 2 3 10 c_c[4]", "Fix ave/time compute vector is accessed out-of-range"),
    ("dump x all custom 10 {p} id c_d[5]", "Dump custom compute vector is accessed out-of-range"),
    ("compute d all com", "Reuse of compute ID"),
])
def test_ill_formed_lines(line, msg, tmp_path):
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    for known in ("compute c all com", "compute d all displace/atom"):
        lmp.command(known)
    with pytest.raises(SfError, match=re.escape(msg)):
        lmp.command(line.format(p=tmp_path / "r.dump"))
    lmp.close()


def test_image_counts_must_be_asked_for_before_the_first_wrap_can_go_uncounted():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("run 1")   # (a rebuild has wrapped the periodic dimensions without a table)
    for line in ("compute x all com", "compute x all displace/atom", "compute x all property/atom ix"):
        with pytest.raises(SfError, match="before the first run"):
            lmp.command(line)
    with pytest.raises(SfError, match="before the first run"):
        lmp.images()
    lmp.close()


def test_an_empty_group_gives_zeros():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    lmp.command("group none type 3")
    for line in ("compute c none com", "compute d none displace/atom"):
        lmp.command(line)
    lmp.command("run 10")
    assert lmp.compute_global("c").tolist() == [0.0] * 3 and not lmp.compute_atom("d").any()
    lmp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. launches

def test_one_launch_for_com():
    bed, cfg = _small("hertz")
    lmp = dc.make_hip(bed, cfg)
    for line in ("compute c all com", "compute c2 all com", "fix t all ave/time 5 2 10 c_c[1]"):
        lmp.command(line)
    g0 = lmp.global_launches()
    assert g0["launches"] == 0
    lmp.command("run 5")   # a sample of the fix, no output: com is evaluated and added on the device
    g1 = lmp.global_launches()
    assert g1["launches"] - g0["launches"] == 2 and g1["host_copies"] == g0["host_copies"]   # com, the fix's addition
    lmp.command("run 2")
    g1 = lmp.global_launches()
    c = lmp.compute_global("c")
    g2 = lmp.global_launches()
    assert g2["launches"] - g1["launches"] == 1 and g2["host_copies"] - g1["host_copies"] == 1
    assert _same(lmp.compute_global("c"), c)
    g3 = lmp.global_launches()
    assert g3["launches"] == g2["launches"]                  # a second query at the same step: no launch
    assert _same(lmp.compute_global("c2"), c)                # another compute: one launch of its own, the same bits
    assert lmp.global_launches()["launches"] - g3["launches"] == 1
    lmp.close()
