"""tests/atom_compute_model.py -- the NumPy statement of the per-atom computes that tests/test_compute_atom_gpu.py holds the
GPU values to -- checked itself against the CPU oracle on a bed that has moved: the per-atom virial summed over the bed
is sum_i x_i (x) f_i of the oracle's pair forces, and the contact counts are the rows of tests/contact_model.py per atom."""
import numpy as np
import pytest

from sedifoam_amd import synthetic
from tests import atom_compute_model as am
from tests import contact_model as cm
from tests import dem_cases as dc

# The free bed flies apart (its initial overlaps are no longer balanced across the faces), so it is observed early, while
# every grain still has partners.
STEPS = 4
# Friction: the Hookean laws store a capped history that gives the capped force again, so they are run with a share of the
# contacts at the Coulomb cap.  The reference's hertzFix law rescales a capped history with a term that lacks its
# polyhertz factor (pair_gran_hertzFix_history.cpp, restated in oracle/orc_contact.c hertz_history_law), so the history it
# RETURNS after a capped evaluation does not give that evaluation's force again: hertz runs with a friction under which
# nothing caps, and the capped branch of that law is held to the engine's own state by the GPU test.
XMU = {"hooke": 0.1, "hooke_plain": 0.1, "hertz": 50.0}


def _bed():
    bed = synthetic.fcc_bed((3, 3, 3), seed=3, vmax=0.2)
    bed["omega"] = np.random.default_rng(7).uniform(-50.0, 50.0, size=(len(bed["x"]), 3))
    bed["periodic"] = (0, 0, 0)
    return bed


@pytest.mark.parametrize("pair", ["hooke", "hertz", "hooke_plain"])
def test_virial_summed_over_the_bed_is_the_oracles_and_counts_are_the_rows(pair):
    """Non-periodic, pair forces only (no wall, g = 0), STEPS steps of the oracle.  Its f after a run is the force
    evaluation of the last step: positions x(n), the HALF-step velocities v(n) - dt/2 f/m and omega(n) - dt/2 tq/(0.4 m r^2)
    (the final integrate undone), and the history it returns, which that evaluation has already updated -- so the model's law
    with shearupdate = false on exactly these inputs gives the oracle's pair forces.  Without periodic images
    sum_i x_i (x) f_i = sum over pairs of del (x) F = sum_i W(i); x is taken about its mean (sum f = 0 to rounding)."""
    bed = _bed()
    cfg = dict(pair=pair, kn=1.0e7 if pair == "hertz" else 5.0e4, gamman=0.5 if pair == "hertz" else 2.0e5,
               xmu=XMU[pair], g=0.0, dt=1.0e-6, skin=0.25e-3, walls=[])
    dem = dc.make_oracle(bed, cfg)
    dem.setup()
    dem.run(STEPS)
    st = dem.get()
    r = 0.5 * np.asarray(bed["diameter"])
    m = 4.0 * np.pi / 3.0 * r ** 3 * np.asarray(bed["density"])
    tag = np.arange(1, len(r) + 1, dtype=np.int32)
    assert (st["tag"] == tag).all()
    dtf = 0.5 * cfg["dt"]
    vh = st["v"] - dtf * st["f"] / m[:, None]
    wh = st["omega"] - dtf * st["torque"] / (0.4 * m * r * r)[:, None]
    hist = dem.history()
    pp = cm.pair_params(pair, cfg["kn"], None, cfg["gamman"], None, cfg["xmu"])
    mod = am.per_atom(bed["boxlo"], bed["boxhi"], bed["periodic"], tag, st["x"], r, m, vh, wh, hist, pp)
    got = mod["virial"].sum(axis=0)
    xc = st["x"] - st["x"].mean(axis=0)
    want = np.array([np.sum(xc[:, a] * st["f"][:, b]) for a, b in am.PAIRS6])
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("model vs oracle (%s): %d ordered pairs, sum rule rel %.3e" % (pair, len(mod["I"]), err))
    assert err <= am.SUM_GATE
    # the bed has moved and the inputs exercise the law: history where the style has one, contacts at the Coulomb cap and below
    assert float(np.max(np.abs(st["x"] - bed["x"]))) > 0.0
    if pair != "hooke_plain":
        assert max(float(np.max(np.abs(s))) for s in hist.values()) > 0.0
    print("capped share %.3f" % mod["capped"].mean())
    if pair == "hertz":
        assert not mod["capped"].any()
    else:
        assert 0.05 <= mod["capped"].mean() <= 0.95, mod["capped"].mean()
    # the per-atom forces as well (the half shares doubled are the pair forces on the atom)
    f = np.zeros_like(st["f"])
    np.add.at(f, mod["I"], mod["F"])
    assert dc.rel_err(f, st["f"]) <= am.SUM_GATE
    # counts: the rows of contact_model.contact_rows that name the atom
    rows = cm.contact_rows(bed["boxlo"], bed["boxhi"], bed["periodic"], tag, st["x"], r, m, st["v"], st["omega"], hist, pp)
    want_n = np.bincount(np.concatenate([rows["tag1"], rows["tag2"]]) - 1, minlength=len(tag))
    assert (mod["contacts"] == want_n).all() and want_n.sum() > 4 * len(tag)
    assert set(zip(rows["tag1"].tolist(), rows["tag2"].tolist())) == set(hist)


def test_kinetic_terms_and_the_sign_by_hand():
    """two free spheres far apart, dyadic numbers: m = 2, r = 0.5, v = (1, 2, -0.5), omega = (0, 4, 0)
    ke = 1/2 * 2 * 5.25 = 5.25, erotate = 1/2 * (0.4 * 2 * 0.25) * 16 = 1.6, stress = -m v_a v_b, no contacts"""
    tag = np.array([1, 2], np.int32)
    x = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    v = np.array([[1.0, 2.0, -0.5], [0.0, 0.0, 0.0]])
    w = np.array([[0.0, 4.0, 0.0], [0.0, 0.0, 0.0]])
    mod = am.per_atom([-8.0] * 3, [8.0] * 3, (1, 1, 1), tag, x, np.array([0.5, 0.5]), np.array([2.0, 2.0]), v, w, {},
                      cm.pair_params("hooke", 1024.0, 256.0, 8.0, 4.0, 0.5))
    assert mod["contacts"].tolist() == [0, 0] and not mod["virial"].any()
    assert mod["ke"].tolist() == [5.25, 0.0]
    assert mod["erotate"][0] == pytest.approx(1.6, rel=1e-15) and mod["erotate"][1] == 0.0
    assert am.stress(mod)[0].tolist() == [-2.0, -8.0, -0.5, -4.0, 1.0, 2.0]
    assert not am.stress(mod, ke=False).any()
    assert not am.stress(mod, group=[False, True]).any()
