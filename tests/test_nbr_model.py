"""tests/nbr_model.py held to answers worked out by hand: four atoms of two types in a box periodic in x and z, a pair at
exactly a bin edge and at exactly the cutoff, a pair seen only through the periodic wrap, an atom slightly outside the box, an
empty group, and the sum rules that tie compute rdf, its counts and compute coord/atom together."""
import numpy as np
import pytest

from tests import nbr_model as nm

LO, HI, PER = (0.0, 0.0, 0.0), (8.0, 8.0, 8.0), (1, 0, 1)
# A and B of type 1, C and D of type 2.  |AB| = 1, |AC| = 2 (a bin edge), |AD| = 1.5 through the periodic wrap in x
# (7.5 - 1 = 6.5 > 4 -> -1.5), |BC| = sqrt 5, |BD| = 2.5 (5.5 > 4 -> -2.5), |CD| = sqrt(1.5^2 + 2^2) = 2.5
X = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 3.0, 1.0], [7.5, 1.0, 1.0]])
T = np.array([1, 1, 2, 2])
ALL = np.ones(4, bool)
PAIRS = (("1", "1"), ("1", "2"), ("*", "*"))


def test_four_atoms_counts_by_hand():
    c = nm.rdf_counts(X, T, ALL, LO, HI, PER, 3, 3.0, PAIRS)   # delr = 1: bins [0, 1) [1, 2) [2, 3)
    assert c["counts"].tolist() == [[0, 2, 0],     # 1 1: AB and BA
                                    [0, 1, 3],     # 1 2: AD | AC BC BD
                                    [0, 4, 8]]     # * *: AB AD twice | AC BC BD CD twice
    assert c["icount"].tolist() == [2, 2, 4]
    assert c["jcount"].tolist() == [2, 2, 4]
    assert c["duplicates"].tolist() == [2, 0, 4]


def test_four_atoms_gr_and_ncoord_by_hand():
    a = nm.rdf(X, T, ALL, LO, HI, PER, 3, 3.0, PAIRS)
    assert a.shape == (3, 7)
    assert a[:, 0].tolist() == [0.5, 1.5, 2.5]
    k = 4.0 * np.pi / (3.0 * 512.0)
    shell = [1.0 * k, 7.0 * k, 19.0 * k]           # constant ((b + 1)^3 - b^3)
    # (counts, icount, normfac = jcount - duplicates / icount) of each pair
    for m, (counts, icount, normfac) in enumerate((([0, 2, 0], 2, 1.0), ([0, 1, 3], 2, 2.0), ([0, 4, 8], 4, 3.0))):
        ncoord = 0.0
        for b in range(3):
            gr = counts[b] / (shell[b] * normfac * icount)
            ncoord += counts[b] / icount
            # (the hand value takes the operations in another order: equal up to a few roundings, stated as such)
            assert a[b, 1 + 2 * m] == pytest.approx(gr, rel=1e-14, abs=0.0), (m, b)
            assert a[b, 2 + 2 * m] == pytest.approx(ncoord, rel=1e-14, abs=0.0), (m, b)
    assert a[2, 6] == pytest.approx(3.0, rel=1e-14)   # every atom has the three others within 3
    assert a[2, 2] == pytest.approx(1.0, rel=1e-14)   # a type-1 atom has one type-1 atom within 3
    assert a[2, 4] == pytest.approx(2.0, rel=1e-14)   # ... and both type-2 atoms


def test_four_atoms_coord_atom_with_two_ranges():
    got = nm.coord_atom(X, T, ALL, LO, HI, PER, 2.2, ("1", "2"))   # sqrt 5 and 2.5 are beyond 2.2
    assert got.tolist() == [[1.0, 2.0], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]
    two = nm.coord_atom(X, T, T == 2, LO, HI, PER, 2.2, ("1", "2"))   # j of any group; i outside the group reads 0
    assert two.tolist() == [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0], [1.0, 0.0]]
    assert nm.coord_atom(X, T, ALL, LO, HI, PER, 2.2).tolist() == [[3.0], [1.0], [1.0], [1.0]]


def test_a_pair_at_exactly_the_cutoff_is_in_neither():
    x = np.array([[1.0, 1.0, 1.0], [4.0, 1.0, 1.0]])
    t = np.array([1, 1])
    c = nm.rdf_counts(x, t, np.ones(2, bool), LO, HI, PER, 3, 3.0)
    assert c["counts"].tolist() == [[0, 0, 0]]        # r delrinv = 3.0 -> ibin = 3 >= Nbin: skipped
    assert nm.coord_atom(x, t, np.ones(2, bool), LO, HI, PER, 3.0).tolist() == [[0.0], [0.0]]   # 9 < 9 is false
    # just inside: the last bin and one neighbour
    x[1, 0] = np.nextafter(4.0, 0.0)
    assert nm.rdf_counts(x, t, np.ones(2, bool), LO, HI, PER, 3, 3.0)["counts"].tolist() == [[0, 0, 2]]
    assert nm.coord_atom(x, t, np.ones(2, bool), LO, HI, PER, 3.0).tolist() == [[1.0], [1.0]]
    # exactly a bin edge belongs to the upper bin
    x[1, 0] = 3.0
    assert nm.rdf_counts(x, t, np.ones(2, bool), LO, HI, PER, 3, 3.0)["counts"].tolist() == [[0, 0, 2]]


def test_a_pair_seen_only_through_the_wrap_and_not_through_a_wall():
    t = np.array([1, 1])
    x = np.array([[0.5, 4.0, 4.0], [7.75, 4.0, 4.0]])    # periodic in x: 7.25 > 4 -> -0.75
    assert nm.rdf_counts(x, t, np.ones(2, bool), LO, HI, PER, 4, 1.0)["counts"].tolist() == [[0, 0, 0, 2]]
    y = np.array([[4.0, 0.5, 4.0], [4.0, 7.75, 4.0]])    # not in y: 7.25 stays
    assert nm.rdf_counts(y, t, np.ones(2, bool), LO, HI, PER, 4, 1.0)["counts"].sum() == 0
    assert nm.coord_atom(x, t, np.ones(2, bool), LO, HI, PER, 1.0).tolist() == [[1.0], [1.0]]
    assert nm.coord_atom(y, t, np.ones(2, bool), LO, HI, PER, 1.0).tolist() == [[0.0], [0.0]]


def test_an_atom_slightly_outside_the_box_is_found():
    t = np.array([1, 1, 1, 1])
    # x = -0.25 lies outside the periodic box: 7.5 - (-0.25) = 7.75 > 4 -> -0.25, so 0.25 apart; y = -0.125 lies below the
    # wall, 0.375 from the atom at y = 0.25 and 4.125 from the one at y = 4
    x = np.array([[-0.25, 4.0, 4.0], [7.5, 4.0, 4.0], [7.5, -0.125, 4.0], [7.5, 0.25, 4.0]])
    assert nm.coord_atom(x, t, np.ones(4, bool), LO, HI, PER, 0.5).tolist() == [[1.0], [1.0], [1.0], [1.0]]
    assert nm.rdf_counts(x, t, np.ones(4, bool), LO, HI, PER, 2, 0.5)["counts"].tolist() == [[0, 4]]


def test_an_empty_group_is_all_zeros_without_a_division_by_zero():
    with np.errstate(all="raise"):
        a = nm.rdf(X, T, np.zeros(4, bool), LO, HI, PER, 3, 3.0, PAIRS)
        c = nm.coord_atom(X, T, np.zeros(4, bool), LO, HI, PER, 3.0, ("1", "*"))
        none = nm.rdf(np.zeros((0, 3)), np.zeros(0, int), np.zeros(0, bool), LO, HI, PER, 3, 3.0)
    assert a[:, 0].tolist() == [0.5, 1.5, 2.5] and not a[:, 1:].any() and np.isfinite(a).all()
    assert not c.any() and c.shape == (4, 2)
    assert not none[:, 1:].any()
    # a pair whose i range holds no atom: icount = 0, all zeros
    b = nm.rdf(X, T, ALL, LO, HI, PER, 3, 3.0, (("3", "*"), ("*", "3")))
    assert not b[:, 1:].any()


def test_a_cutoff_beyond_half_a_periodic_length_is_refused():
    with pytest.raises(ValueError, match="cutoff is longer than half a periodic box length"):
        nm.rdf(X, T, ALL, LO, HI, PER, 3, 4.5)
    with pytest.raises(ValueError, match="cutoff is longer than half a periodic box length"):
        nm.coord_atom(X, T, ALL, LO, HI, PER, 4.001)
    nm.coord_atom(X, T, ALL, LO, HI, (0, 1, 0), 4.0)   # exactly half is taken


def test_sum_rules():
    rng = np.random.default_rng(5)
    n, rc, nbin = 60, 2.5, 13
    x = rng.uniform(0.0, 8.0, size=(n, 3))
    t = rng.integers(1, 4, size=n)
    every = np.ones(n, bool)
    rsq = nm.pair_rsq(x, LO, HI, PER)
    delrinv = 1.0 / (rc / nbin)
    within = (np.sqrt(rsq) * delrinv < nbin) & ~np.eye(n, dtype=bool)
    pairs = (("*", "*"), ("1", "2*3"), ("2", "2"))
    c = nm.rdf_counts(x, t, every, LO, HI, PER, nbin, rc, pairs)
    a = nm.rdf_array(c, LO, HI, nbin, rc)
    for m, (iw, jw) in enumerate(pairs):
        ilo, ihi = nm.type_range(iw)
        jlo, jhi = nm.type_range(jw)
        direct = int((within & ((t >= ilo) & (t <= ihi))[:, None] & ((t >= jlo) & (t <= jhi))[None, :]).sum())
        assert int(c["counts"][m].sum()) == direct
        # the last ncoord times icount is that sum -- up to the rounding of nbin multiplications, divisions and additions
        assert a[-1, 2 + 2 * m] * c["icount"][m] == pytest.approx(direct, rel=1e-13)
    assert int(c["counts"][0].sum()) > 0 and int(c["counts"][2].sum()) > 0
    # a coord/atom column summed over the group `all` is the rdf count sum of the same j range.  (coord/atom compares rsq with
    # rc rc, rdf compares sqrt(rsq) delrinv with Nbin: no random pair lies within a rounding of the cutoff, asserted here)
    assert not np.any(np.abs(np.sqrt(rsq) - rc) < 1e-9)
    col = nm.coord_atom(x, t, every, LO, HI, PER, rc, ("*", "2*3"))
    assert int(col[:, 0].sum()) == int(c["counts"][0].sum())
    only1 = nm.coord_atom(x, t, t == 1, LO, HI, PER, rc, ("2*3",))
    assert int(only1.sum()) == int(c["counts"][1].sum())


def test_mode_vector_text_and_averages():
    words = ["c_g[2]", "c_g[3]"]
    assert nm.vector_header("t", words) == "# Time-averaged data for fix t\n# TimeStep Number-of-rows\n# Row c_g[2] c_g[3]\n"
    assert nm.vector_header("t", words, title3="# r g n") == "# Time-averaged data for fix t\n# TimeStep Number-of-rows\n# r g n\n"
    assert nm.vector_block(10, [[0.5, 1.0], [0.25, 3.0]]) == "10 2\n1 0.5 1\n2 0.25 3\n"
    assert nm.vector_block(20, [[1.0 / 3.0]], " %.10g") == "20 1\n1 0.3333333333\n"
    av = nm.VectorAverager(2, 2, 2, "window", 2)
    outs = []
    for k in range(3):
        av.add_sample([[1.0 * k, 2.0], [3.0, 4.0]])
        av.add_sample([[1.0 * k, 4.0], [5.0, 4.0]])
        outs.append(av.output().tolist())
    assert outs == [[[0.0, 3.0], [4.0, 4.0]], [[0.5, 3.0], [4.0, 4.0]], [[1.5, 3.0], [4.0, 4.0]]]
    one = nm.VectorAverager(1, 1, 1)
    one.add_sample([[7.0]])
    assert one.output().tolist() == [[7.0]]
