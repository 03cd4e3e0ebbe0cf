"""tests/contact_model.py -- the NumPy statement of a `compute pair/local` row that tests/test_contacts_gpu.py holds the GPU
rows to -- checked itself: its rows summed per atom are the CPU oracle's pair forces, and a contact of two spheres with
dyadic numbers gives the values worked out by hand below."""
import numpy as np
import pytest

from sedifoam_amd import synthetic
from tests import contact_model as cm
from tests import dem_cases as dc


def bed_inputs(bed):
    r = 0.5 * np.asarray(bed["diameter"])
    m = 4.0 * np.pi / 3.0 * r ** 3 * np.asarray(bed["density"])
    tag = np.arange(1, len(r) + 1, dtype=np.int32) if bed.get("tag") is None else np.asarray(bed["tag"])
    return tag, r, m


@pytest.mark.parametrize("pair", ["hooke", "hertz", "hooke_plain"])
def test_rows_summed_per_atom_are_the_oracles_pair_forces(pair):
    """3 x 3 x 3 fcc cells, periodic in x and z, pair forces only (no wall, no cohesion, g = 0): after setup() the oracle's
    f is the sum of its pair forces, + (f + fs) for tag1 and - for tag2 of every row.  (The oracle has no second evaluation
    with shearupdate = 0 on a state it has advanced, so the comparison after motion is the GPU test's, which feeds the
    engine's own state and history to the model.)"""
    bed = synthetic.fcc_bed((3, 3, 3), seed=3, vmax=0.2)
    bed["omega"] = np.random.default_rng(7).uniform(-50.0, 50.0, size=(len(bed["x"]), 3))
    cfg = dict(pair=pair, kn=1.0e7 if pair == "hertz" else 2.0e4, gamman=0.5 if pair == "hertz" else 50.0, xmu=0.4, g=0.0,
               dt=1.0e-6, skin=0.25e-3, walls=[])
    dem = dc.make_oracle(bed, cfg)
    dem.setup()
    st = dem.get()
    tag, r, m = bed_inputs(bed)
    assert (st["tag"] == tag).all()
    rows = cm.contact_rows(bed["boxlo"], bed["boxhi"], bed["periodic"], tag, st["x"], r, m, st["v"], st["omega"],
                           dem.history(), cm.pair_params(pair, cfg["kn"], None, cfg["gamman"], None, cfg["xmu"]))
    assert set(zip(rows["tag1"].tolist(), rows["tag2"].tolist())) == set(dem.history())
    assert rows["wrapped"].any() and not rows["wrapped"].all()
    err = dc.rel_err(cm.per_atom_sums(rows, tag), st["f"])
    print("model vs oracle (%s): %d rows, rel %.3e" % (pair, len(rows["dist"]), err))
    assert len(rows["dist"]) > 4 * len(tag)
    assert err <= cm.GATE


@pytest.mark.parametrize("xmu,fs,p4", [
    (0.5, (0.0, -12.0, -16.0), 20.0),           # below the Coulomb cap: |fs| = 20 < xmu |force| = 65
    (0.0625, (0.0, -4.875, -6.5), 8.125),       # above it: fs scaled by 8.125 / 20 = 13 / 32
])
def test_two_spheres_by_hand(xmu, fs, p4):
    """gran/hooke/history, every number dyadic so that every operation is exact:
    radii 0.3125, x1 = 0, x2 = (0.5, 0, 0): del = (-0.5, 0, 0), r = 0.5, 1 / r = 2, 1 / rsq = 4, overlap = 0.125
    m1 = m2 = 2: meff = 1;  kn = 1024, kt = 256, gamman = 8, gammat = 4
    v1 - v2 = (0.25, 0.5, 0): vnnr = -0.125, vn = (0.25, 0, 0), vt = vtr = (0, 0.5, 0) (no rotation)
    damp = 1 * 8 * -0.125 * 4 = -4, ccel = 1024 * 0.125 * 2 + 4 = 260, force = 130, f = (-130, 0, 0)
    shear = (0, 10 / 256, 16 / 256): fs = -(256 shear + 1 * 4 * vtr) = (0, -12, -16), |fs| = 20
    fn = xmu * 130: 65 for xmu = 0.5 (no cap), 8.125 for xmu = 0.0625 (fs * 8.125 / 20)"""
    tag = np.array([1, 2], np.int32)
    x = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    v = np.array([[0.25, 0.5, 0.0], [0.0, 0.0, 0.0]])
    rows = cm.contact_rows([-2.0] * 3, [2.0] * 3, (0, 0, 0), tag, x, np.array([0.3125, 0.3125]), np.array([2.0, 2.0]), v,
                           np.zeros((2, 3)), {(1, 2): np.array([0.0, 10.0 / 256.0, 16.0 / 256.0])},
                           cm.pair_params("hooke", 1024.0, 256.0, 8.0, 4.0, xmu))
    assert rows["tag1"].tolist() == [1] and rows["tag2"].tolist() == [2]
    assert rows["dist"][0] == 0.5
    assert rows["force"][0] == 130.0
    assert rows["f"][0].tolist() == [-130.0, 0.0, 0.0]
    assert rows["fs"][0].tolist() == list(fs)
    assert rows["fsmag"][0] == p4
    assert bool(rows["capped"][0]) == (xmu < 0.1)
    # the other way round (the higher tag listed first): the same row
    rev = cm.contact_rows([-2.0] * 3, [2.0] * 3, (0, 0, 0), tag[::-1], x[::-1], np.array([0.3125, 0.3125]),
                          np.array([2.0, 2.0]), v[::-1], np.zeros((2, 3)),
                          {(1, 2): np.array([0.0, 10.0 / 256.0, 16.0 / 256.0])},
                          cm.pair_params("hooke", 1024.0, 256.0, 8.0, 4.0, xmu))
    for k in ("dist", "force", "f", "fs", "fsmag"):
        assert (rev[k] == rows[k]).all()
