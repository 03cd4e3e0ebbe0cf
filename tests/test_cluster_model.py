"""tests/cluster_model.py, the NumPy statement of `compute cluster/atom` and `compute cluster/stats`, held
to answers worked out by hand.  No GPU."""
import numpy as np
import pytest

from tests import cluster_model as cm

OPEN = (0, 0, 0)
LO, HI = np.zeros(3), np.ones(3)


def _line(xs):
    x = np.zeros((len(xs), 3))
    x[:, 0] = xs
    x[:, 1:] = 0.5
    return x


def _run(xs, tags, group=None, cut=0.25, per=OPEN, radius=None, surface=False, hi=HI):
    n = len(xs)
    group = np.ones(n, bool) if group is None else np.asarray(group, bool)
    radius = np.full(n, 0.01) if radius is None else np.asarray(radius, np.float64)
    return cm.cluster_atom(_line(xs), radius, np.asarray(tags), group, LO, hi, per, cut, surface)


def test_a_pair_at_exactly_the_cutoff_is_apart_and_one_ulp_below_is_linked():
    cut = 0.25   # (0.25 and 0.0625 are exact, and so is 0.5 - 0.25)
    at = _run([0.25, 0.5], [1, 2], cut=cut)
    assert at.tolist() == [[1.0, 1.0], [2.0, 1.0]]
    below = _run([0.25, np.nextafter(0.5, 0.0)], [1, 2], cut=cut)
    assert below.tolist() == [[1.0, 2.0], [1.0, 2.0]]
    above = _run([0.25, np.nextafter(0.5, 1.0)], [1, 2], cut=cut)
    assert above.tolist() == at.tolist()


def test_a_chain_through_a_periodic_face():
    xs, tags = [0.05, 0.95, 0.8, 0.4], [7, 3, 9, 5]
    # 0.95 - 0.8 = 0.15 and 0.05 - 0.95 + 1 = 0.1 are links at 0.16; 0.05 to 0.8 is 0.25 through the face; 0.4 is alone
    wrapped = _run(xs, tags, cut=0.16, per=(1, 0, 0))
    assert wrapped.tolist() == [[3.0, 3.0], [3.0, 3.0], [3.0, 3.0], [5.0, 1.0]]
    walled = _run(xs, tags, cut=0.16, per=OPEN)
    assert walled.tolist() == [[7.0, 1.0], [3.0, 2.0], [3.0, 2.0], [5.0, 1.0]]
    ids = wrapped[:, 0]
    assert cm.cluster_stats(ids, np.ones(4, bool)).tolist() == [2.0, 3.0, 4.0]
    assert cm.cluster_stats(walled[:, 0], np.ones(4, bool)).tolist() == [3.0, 2.0, 4.0]
    with pytest.raises(ValueError, match="longer than half a periodic box length"):
        _run(xs, tags, cut=0.51, per=(1, 0, 0))


def test_an_atom_outside_the_group_links_nothing_and_bridges_nothing():
    out = _run([0.1, 0.2, 0.3], [1, 2, 3], group=[True, False, True], cut=0.15)
    assert out.tolist() == [[1.0, 1.0], [0.0, 0.0], [3.0, 1.0]]
    assert _run([0.1, 0.2, 0.3], [1, 2, 3], cut=0.15).tolist() == [[1.0, 3.0]] * 3
    # the stats count the atoms of THEIR group with an ID: a stats group wider than the cluster group sees the 0 and skips it
    assert cm.cluster_stats(out[:, 0], [True, True, True]).tolist() == [2.0, 1.0, 2.0]
    assert cm.cluster_stats(out[:, 0], [True, True, False]).tolist() == [1.0, 1.0, 1.0]
    assert cm.cluster_stats(out[:, 0], [False, True, False]).tolist() == [0.0, 0.0, 0.0]


def test_the_surface_rule_and_the_centre_rule_disagree_on_two_radii():
    # A (r 0.1) - 0.45 - B (r 0.3) - 0.75 - C (r 0.1) - 0.55 - D (r 0.1), gap 0.1
    xs, rad, tags = [0.1, 0.55, 1.3, 1.85], [0.1, 0.3, 0.1, 0.1], [4, 3, 2, 1]
    hi = np.array([4.0, 1.0, 1.0])
    surf = _run(xs, tags, cut=0.1, radius=rad, surface=True, hi=hi)
    # A-B: s = 0.5 > 0.45; B-C: s = 0.5 < 0.75; C-D: s = 0.3 < 0.55
    assert surf.tolist() == [[3.0, 2.0], [3.0, 2.0], [2.0, 1.0], [1.0, 1.0]]
    wide = _run(xs, tags, cut=2 * 0.3 + 0.1, radius=rad, hi=hi)    # the centre rule at the largest reach: C-D joins
    assert wide.tolist() == [[3.0, 2.0], [3.0, 2.0], [1.0, 2.0], [1.0, 2.0]]
    narrow = _run(xs, tags, cut=2 * 0.1 + 0.1, radius=rad, hi=hi)  # ... at the smallest: A-B parts
    assert narrow.tolist() == [[4.0, 1.0], [3.0, 1.0], [2.0, 1.0], [1.0, 1.0]]
    # a gap of zero is touching: overlapping spheres only
    touch = _run([0.1, 0.45, 0.9], [1, 2, 3], cut=0.0, radius=[0.1, 0.3, 0.1], surface=True, hi=hi)
    assert touch.tolist() == [[1.0, 2.0], [1.0, 2.0], [3.0, 1.0]]
    # the grid the engine walks is 2 rmax + CUT wide, and a periodic length must hold two of them
    assert cm.grid_cutoff(0.1, True, 0.3) == 2.0 * 0.3 + 0.1 and cm.grid_cutoff(0.1) == 0.1
    with pytest.raises(ValueError, match="longer than half a periodic box length"):
        cm.cluster_atom(_line(xs), rad, tags, np.ones(4, bool), LO, np.array([1.3, 1.0, 1.0]), (1, 0, 0), 0.1, True)


def test_tags_with_gaps_and_out_of_order():
    out = _run([0.1, 0.2, 0.6, 0.7, 0.9], [250, 40, 7, 1000, 12], cut=0.15)
    assert out.tolist() == [[40.0, 2.0], [40.0, 2.0], [7.0, 2.0], [7.0, 2.0], [12.0, 1.0]]
    assert cm.cluster_stats(out[:, 0], np.ones(5, bool)).tolist() == [3.0, 2.0, 5.0]


def test_a_long_chain_is_one_component_and_no_atoms_are_none():
    n = 300
    xs = 0.5 + 0.99 * 0.25 * np.arange(n)
    order = np.random.default_rng(5).permutation(n)
    tags = order + 10
    out = _run(xs, tags, cut=0.25, hi=np.array([100.0, 1.0, 1.0]))
    assert (out[:, 0] == 10.0).all() and (out[:, 1] == n).all()
    assert _run([], [], cut=0.25).shape == (0, 2)
    assert cm.cluster_stats([], []).tolist() == [0.0, 0.0, 0.0]
