"""tests/chunk_model.py -- the NumPy statement of `compute chunk/atom bin/*` and `fix ave/chunk` that
tests/test_ave_chunk_gpu.py holds the engine to -- against answers worked out by hand: the ragged first and last layers of
every `origin` word on a box whose length is no multiple of delta, `bound` with each `discard`, a coordinate outside a
periodic box and one exactly on an edge, 2-D numbering, the first valid step, the three norms, `ave running` and the text."""
import numpy as np
import pytest

from tests import chunk_model as km

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def _b(args, periodic=(1, 0, 1), box=UNIT):
    return km.bins("compute c all chunk/atom " + args, box[0], box[1], periodic)


@pytest.mark.parametrize("origin,offset,nlayers", [
    ("lower", 0.0, 4),      # 0 | .3 .6 .9 | 1.2: the last layer sticks out
    ("upper", -0.2, 4),     # 1 - 3 x .3 = .1 > 0, so one more below: -.2 .1 .4 .7 | 1
    ("center", -0.1, 4),    # .5 - .3 = .2 > 0 -> -.1;  .5 + .3 = .8 < 1 -> 1.1
    ("0.05", -0.25, 5),     # -.25 .05 .35 .65 .95 | 1.25: both ends ragged
])
def test_layers_of_each_origin_word_on_a_box_that_is_no_multiple_of_delta(origin, offset, nlayers):
    B = _b("bin/1d x %s 0.3 units box" % origin)
    assert B["nlayers"] == [nlayers] and B["nchunk"] == nlayers
    assert B["offset"][0] == pytest.approx(offset, abs=1e-15)
    assert B["volume"] == pytest.approx(0.3)
    assert km.coords(B)[:, 0] == pytest.approx(offset + 0.3 * (np.arange(nlayers) + 0.5), abs=1e-14)
    # every point of the box has a layer, and the first and the last layer are used
    ids = km.assign(B, [[0.0, 0, 0], [0.999, 0, 0]])
    assert ids.tolist() == [1, nlayers]


def test_units_reduced_are_fractions_of_the_box_length():
    B = _b("bin/1d y lower 0.25 units reduced bound y 0.25 upper", box=([0, 1.0, 0], [1, 3.0, 1]))
    assert B["delta"] == [0.5] and B["offset"] == [1.5] and B["nlayers"] == [3] and B["volume"] == 0.5
    assert km.assign(B, [[0, 1.4, 0], [0, 1.5, 0], [0, 2.9, 0]]).tolist() == [0, 1, 3]


@pytest.mark.parametrize("discard,want", [("mixed", [0, 1, 2, 0]), ("yes", [0, 1, 2, 0]), ("no", [1, 1, 2, 2])])
def test_bound_with_each_discard(discard, want):
    B = _b("bin/1d y lower 0.25 units box bound y 0.25 0.75 discard " + discard)
    assert B["nlayers"] == [2] and B["offset"] == [0.25]
    assert km.assign(B, [[0, 0.1, 0], [0, 0.3, 0], [0, 0.6, 0], [0, 0.9, 0]]).tolist() == want


def test_without_a_bound_mixed_clamps_and_yes_discards():
    x = [[0, -0.1, 0], [0, 1.2, 0]]   # (y is not periodic)
    assert km.assign(_b("bin/1d y lower 0.25 units box"), x).tolist() == [1, 4]
    assert km.assign(_b("bin/1d y lower 0.25 units box discard yes"), x).tolist() == [0, 0]


def test_a_coordinate_outside_a_periodic_box_is_remapped_first():
    B = _b("bin/1d x lower 0.25 units box discard yes")
    assert km.assign(B, [[-0.1, 0, 0], [1.05, 0, 0], [1.0, 0, 0]]).tolist() == [4, 1, 1]


def test_a_coordinate_on_an_edge_belongs_to_the_upper_layer():
    B = _b("bin/1d x lower 0.25 units box")
    assert km.assign(B, [[0.0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.75, 0, 0]]).tolist() == [1, 2, 3, 4]


def test_2d_numbering_the_first_dimension_named_varies_slowest():
    B = _b("bin/2d y lower 0.5 x lower 0.25 units box")
    assert B["nlayers"] == [2, 4] and B["nchunk"] == 8 and B["volume"] == 0.125
    assert km.assign(B, [[0.6, 0.7, 0.3], [0.1, 0.2, 0.9]]).tolist() == [1 + 1 * 4 + 2, 1]
    assert km.coords(B)[6].tolist() == [0.75, 0.625]
    # and a group: atoms outside it read 0
    assert km.assign(B, [[0.6, 0.7, 0.3], [0.1, 0.2, 0.9]], in_group=np.array([False, True])).tolist() == [0, 1]


def test_first_valid_step_and_schedule():
    assert km.first_valid(0, 5, 1, 10) == 0 and km.first_valid(20, 10, 1, 10) == 20   # Nrepeat 1 at a multiple: that step
    assert km.first_valid(7, 5, 1, 10) == 10 and km.first_valid(7, 10, 1, 10) == 10
    assert km.first_valid(0, 2, 3, 10) == 6 and km.first_valid(7, 2, 3, 10) == 16      # 6 lies behind step 7
    assert km.schedule(0, 5, 1, 10, 25) == [(0, [0]), (10, [10]), (20, [20])]
    assert km.schedule(7, 2, 3, 10, 67) == [(20, [16, 18, 20]), (30, [26, 28, 30]), (40, [36, 38, 40]), (50, [46, 48, 50]),
                                            (60, [56, 58, 60])]


def _two_outputs(norm, running):
    B = _b("bin/1d y lower 0.5 units box")   # two chunks of volume 0.5
    A = km.Averager(B, ["vx", "density/number", "density/mass"], norm=norm, running=running, nrepeat=2)
    m = np.full(3, 2.0)
    A.add_sample(np.array([1, 1, 2]), dict(vx=np.array([1.0, 3.0, 10.0]), mass=m))
    A.add_sample(np.array([1, 2, 2]), dict(vx=np.array([5.0, 20.0, 30.0]), mass=m))
    first = A.output()
    A.add_sample(np.array([1, 1, 1]), dict(vx=np.ones(3), mass=m))
    A.add_sample(np.array([1, 1, 1]), dict(vx=np.ones(3), mass=m))
    return first, A.output()


def test_the_three_norms():
    for norm, vx in (("all", [3.0, 20.0]), ("sample", [3.5, 17.5]), ("none", [4.5, 30.0])):
        (count, val), (count2, val2) = _two_outputs(norm, False)
        assert count.tolist() == [1.5, 1.5] and val[:, 0].tolist() == vx
        assert val[:, 1].tolist() == [3.0, 3.0] and val[:, 2].tolist() == [6.0, 6.0]
        assert count2.tolist() == [3.0, 0.0] and val2[:, 0].tolist() == {"all": [1.0, 0.0], "sample": [1.0, 0.0], "none": [3.0, 0.0]}[norm]


def test_ave_running():
    (_, _), (count, val) = _two_outputs("all", True)
    assert count.tolist() == [2.25, 0.75]                      # the mean of the per-output Ncount
    assert val[:, 0] == pytest.approx([15.0 / 9.0, 20.0], rel=1e-15)   # sums and counts accumulate before the division
    assert val[:, 1].tolist() == [4.5, 1.5] and val[:, 2].tolist() == [9.0, 3.0]
    (_, _), (count, val) = _two_outputs("none", True)
    assert val[:, 0].tolist() == [3.75, 15.0]
    (_, _), (count, val) = _two_outputs("sample", True)
    assert val[:, 0].tolist() == [2.25, 8.75]


def test_the_file_text():
    B = _b("bin/2d y lower 0.5 x lower 0.5 units box")
    assert km.header("p", "all", B, ["vx", "c_s[1]"]) == (
        "# Chunk-averaged data for fix p and group all\n# Timestep Number-of-chunks Total-count\n"
        "# Chunk Coord1 Coord2 Ncount vx c_s[1]\n")
    assert km.header("p", "all", B, ["vx"], titles=("a b", None, "c")) == "a b\n# Timestep Number-of-chunks Total-count\nc\n"
    count = np.array([1.5, 0.0, 2.0, 1.0])
    val = np.array([[1.0 / 3.0], [0.0], [-2.5e-7], [1234567.0]])
    assert km.text(40, B, count, val) == ("40 4 4.5\n  1 0.25 0.25 1.5 0.333333\n  2 0.25 0.75 0 0\n"
                                          "  3 0.75 0.25 2 -2.5e-07\n  4 0.75 0.75 1 1.23457e+06\n")
    assert km.text(40, B, count, val, fmt="%.10g").splitlines()[1] == "  1 0.25 0.25 1.5 0.3333333333"
