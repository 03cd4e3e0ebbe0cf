"""The brute-force neighbour-list reference (tests/neigh_model.py) against known answers, and pinned to the CPU oracle's
pair counts on every input of tests/test_neigh_list_gpu.py -- before any GPU is involved.  The model reads neither the engine
nor the oracle; the oracle bins into cells, the model does not."""
import numpy as np
import pytest

from tests import dem_cases as dc
from tests import neigh_cases as nc
from tests import neigh_model as nm


def test_perfect_fcc_bed_has_twelve_rows_per_atom():
    a = 1.0e-3                                   # nearest-neighbour distance; the second shell is at sqrt(2) a
    edge = a * np.sqrt(2.0)
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(3), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * edge + 0.1 * edge
    n = len(x)
    hi = np.array([4, 3, 5]) * edge
    rows, band = nm.neighbor_rows(x, np.full(n, 0.45e-3), np.zeros(3), hi, (1, 1, 1), 0.2e-3)   # cut 1.1 a
    assert band == 0
    assert len(rows) == 12 * n and (np.bincount(rows[:, 0], minlength=n + 1)[1:] == 12).all()
    assert nm.longest_row(rows) == 12
    # the same lattice between walls: the atoms of the faces lose their outside neighbours and nothing else changes
    rows_c, _ = nm.neighbor_rows(x, np.full(n, 0.45e-3), np.zeros(3), hi, (0, 0, 0), 0.2e-3)
    assert nm.as_set(rows_c) == {r for r in nm.as_set(rows) if r[2:] == (0, 0, 0)}
    # an absolute cutoff beyond the second shell (sqrt(2) a): 12 + 6
    rows_a, _ = nm.neighbor_rows(x, np.full(n, 0.45e-3), np.zeros(3), hi, (1, 1, 1), 0.2e-3, cut_abs=1.5 * a)
    assert len(rows_a) == 18 * n
    # touching: radius 0.45 a does not reach, 0.51 a does
    assert len(nm.neighbor_rows(x, np.full(n, 0.45e-3), np.zeros(3), hi, (1, 1, 1), 0.0, touching=True)[0]) == 0
    assert len(nm.neighbor_rows(x, np.full(n, 0.51e-3), np.zeros(3), hi, (1, 1, 1), 0.0, touching=True)[0]) == 12 * n


@pytest.mark.parametrize("name,extra,cut_abs", nc.CLOUD_RUNS, ids=lambda v: v if isinstance(v, str) else None)
def test_cloud_model_is_symmetric_without_duplicates_and_counts_what_the_oracle_counts(name, extra, cut_abs):
    bed = nc.cloud(name)
    assert bed["n"] >= 300 and bed["n"] % 64 != 0
    rows_set, band, rows = nc.cloud_model(name, cut_abs)
    assert band == 0, "a pair within rounding of the cutoff: choose another seed"
    assert len(rows_set) == len(rows)                                       # no duplicates
    assert {(j, i, -sx, -sy, -sz) for (i, j, sx, sy, sz) in rows_set} == rows_set
    assert not any(i == j and (sx, sy, sz) == (0, 0, 0) for (i, j, sx, sy, sz) in rows_set)
    # the oracle keeps the granular half list (ri + rj + skin) whatever else is defined, and exposes its count: the
    # model with that criterion must count the same
    _, band_g, rows_g = nc.cloud_model(name, 0.0)
    assert band_g == 0
    orc = dc.make_oracle(bed, nc.cloud_cfg(name, extra))
    orc.setup()
    assert orc.npairs == nm.half_count(rows_g)
    if cut_abs > 0.0:
        assert rows_set > nc.cloud_model(name, 0.0)[0]      # the absolute cutoff only adds (small-small pairs)


def test_cloud_shapes_are_what_they_are_for():
    mean = lambda rows, n: len(rows) / n
    for name in ("periodic_5x4x6", "xz_periodic_thin", "closed_4p5"):
        assert 15.0 <= mean(nc.cloud_model(name, 0.0)[2], nc.cloud(name)["n"]) <= 25.0
    assert mean(nc.cloud_model("periodic_3x3x3_exact", 0.0)[2], nc.cloud("periodic_3x3x3_exact")["n"]) > 45.0
    assert 15.0 <= mean(nc.cloud_model("poly_ratio3", nc.CUT)[2], nc.cloud("poly_ratio3")["n"]) <= 25.0
    d = nc.cloud("poly_ratio3")["diameter"]
    assert d.max() / d.min() > 2.9
    dense = nc.cloud_model("dense", 0.0)[2]
    assert mean(dense, nc.cloud("dense")["n"]) > 100.0 and nm.longest_row(dense) > 128
    # closed box: atoms within one radius of every face
    bed = nc.cloud("closed_4p5")
    r = 0.5 * bed["diameter"]
    for k in range(3):
        assert (bed["x"][:, k] - bed["boxlo"][k] < r).any() and (bed["boxhi"][k] - bed["x"][:, k] < r).any()
    # the thin box (2.2 cutoffs: wider than two, so no pair is seen through two images at once): neighbours through
    # every image of the x-z plane, the edge images included, and none through y
    thin = nc.cloud_model("xz_periodic_thin", 0.0)[2]
    assert {tuple(s) for s in thin[:, 2:].tolist()} == {(sx, 0, sz) for sx in (-1, 0, 1) for sz in (-1, 0, 1)}


@pytest.mark.parametrize("lo_name", list(nc.EX_LO))
@pytest.mark.parametrize("box", list(nc.EX_BOXES))
def test_exact_cases_have_their_known_counts(box, lo_name):
    # the lattice alone: every nearest neighbour sits at rsq == cut^2 exactly and is listed; six per atom when periodic
    for size in nc.EX_SIZES:
        rows_set, band, rows = nc.exact_model(box, lo_name, True, size)
        bed = nc.exact_case(box, lo_name, True, size)
        assert len(rows) == len(rows_set) == nc.exact_lattice_rows(box)
        if box == "ppp":
            assert (np.bincount(rows[:, 0])[1:] == 6).all()
        assert band == len(rows)          # every listed pair is AT the cutoff: these cases are exact, not band-free
        orc = dc.make_oracle(bed, nc.exact_cfg(bed))
        orc.setup()
        assert orc.npairs == nm.half_count(rows), size
    # with the displaced lattice, the probe and the atoms on the faces
    rows_set, band, rows = nc.exact_model(box, lo_name)
    bed = nc.exact_case(box, lo_name)
    assert len(rows) == len(rows_set)
    plain = {(i, j) for (i, j, sx, sy, sz) in rows_set if (sx, sy, sz) == (0, 0, 0)}
    assert bed["pairs_at_cutoff"] and all(p in plain and p[::-1] in plain for p in bed["pairs_at_cutoff"])
    anyimg = {(i, j) for (i, j, *_s) in rows_set}
    assert bed["pairs_beyond"] and not any(p in anyimg or p[::-1] in anyimg for p in bed["pairs_beyond"])
    assert len(bed["wrapped"]) == sum(bed["periodic"])
    for t in bed["wrapped"]:
        assert (bed["x"][t - 1] != bed["xw"][t - 1]).sum() == 1
    orc = dc.make_oracle(bed, nc.exact_cfg(bed))
    orc.setup()
    assert orc.npairs == nm.half_count(rows)
    assert np.array_equal(orc.get()["x"], bed["xw"])       # the wrap takes hi to lo, exactly
