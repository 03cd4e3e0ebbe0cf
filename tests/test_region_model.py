"""tests/region_model.py held to hand-computed answers: the primitives at and around their surfaces, side, union and
intersect of matches, the command line of a region, and the schedule of a dynamic group."""
import numpy as np

from tests import region_model as rm


def test_block_is_closed_and_inf_is_big():
    b = ("block", 0.0, 1.0, 0.0, 2.0, -rm.BIG, rm.BIG, "in")
    p = [[0.0, 0.0, 5.0], [1.0, 2.0, -1e19], [1.0000000000000002, 1.0, 0.0], [0.5, -1e-300, 0.0], [0.5, 1.0, 1e21]]
    assert rm.match(b, p).tolist() == [True, True, False, False, False]
    assert rm.on_boundary(b, p).tolist() == [True, True, False, False, False]
    assert rm.match(b[:-1] + ("out",), p).tolist() == [False, False, True, True, True]
    assert rm.command("r", b) == "region r block 0 1 0 2 INF INF side in units box"


def test_sphere_on_pythagorean_quadruples():
    s = ("sphere", 1.0, 1.0, 1.0, 3.0, "in")
    # 1 + 4 + 4 = 9: exactly on.  dx = 1 + 2^-49: dx^2 rounds to 1 + 2^-48, the sum 9 + 2^-48 is a double and its root
    # 3 + 2^-48 / 6 rounds to 3 + 2^-51: outside.  dx = 1 - 2^-49: the sum is 9 - 2^-48, its root below 3: inside
    p = np.array([[2.0, 3.0, 3.0], [2.0 + 2.0 ** -49, 3.0, 3.0], [2.0 - 2.0 ** -49, 3.0, 3.0], [1.0, 1.0, 1.0], [4.0, 1.0, 1.0],
                  [4.0, 1.0, 1.0 + 2.0 ** -20]])
    assert rm.match(s, p).tolist() == [True, False, True, True, True, False]
    assert rm.on_boundary(s, p).tolist() == [True, False, False, False, True, False]
    # 4 + 9 + 36 = 49
    s7 = ("sphere", 0.0, 0.0, 0.0, 7.0, "out")
    assert rm.match(s7, [[2.0, 3.0, 6.0], [2.0, 3.0, 6.5], [0.0, 0.0, 0.0]]).tolist() == [False, True, False]


def test_cylinder_axes_take_lammps_order():
    # axis y: c1 c2 are x z; 9 + 16 = 25
    c = ("cylinder", "y", 1.0, 2.0, 5.0, 0.0, 1.0, "in")
    p = [[4.0, 0.0, 6.0], [4.0, 1.0, 6.0], [4.0, 1.5, 6.0], [4.0, 0.5, 6.5], [1.0, 0.5, 2.0]]
    assert rm.match(c, p).tolist() == [True, True, False, False, True]
    assert rm.on_boundary(c, p).tolist() == [True, True, False, False, False]
    # the same numbers about x are another set: c1 c2 are y z
    cx = ("cylinder", "x", 1.0, 2.0, 5.0, 0.0, 1.0, "in")
    assert rm.match(cx, [[0.5, 4.0, 6.0], [4.0, 0.5, 6.0]]).tolist() == [True, False]
    cz = ("cylinder", "z", 1.0, 2.0, 5.0, 0.0, 1.0, "in")
    assert rm.match(cz, [[4.0, 6.0, 0.5], [4.0, 0.5, 6.0]]).tolist() == [True, False]
    assert rm.command("c", c) == "region c cylinder y 1 2 5 0 1 side in units box"


def test_plane_normal_is_normalised_and_the_plane_itself_is_inside():
    pl = ("plane", 1.0, 0.0, 0.0, 2.0, 0.0, 0.0, "in")
    p = [[1.0, 5.0, 5.0], [1.5, 0.0, 0.0], [0.5, 0.0, 0.0]]
    assert rm.match(pl, p).tolist() == [True, True, False]
    assert rm.on_boundary(pl, p).tolist() == [True, False, False]
    # a normal along -y of length 4: inside is y <= 1
    down = ("plane", 0.0, 1.0, 0.0, 0.0, -4.0, 0.0, "in")
    assert rm.match(down, [[9.0, 1.0, 9.0], [0.0, 1.5, 0.0], [0.0, 0.5, 0.0]]).tolist() == [True, False, True]
    # 3 4 0 has length 5, and 3 / 5, 4 / 5 are rounded: 4 * 0.6 = 2.3999999999999999 (exact), 3 * 0.8 rounds up to
    # 2.4000000000000004, so (4, -3, 0), which lies on the plane, is not inside by one ulp -- and (-4, 3, 0) is
    tilt = ("plane", 0.0, 0.0, 0.0, 3.0, 4.0, 0.0, "in")
    assert rm.match(tilt, [[4.0, -3.0, 9.0], [-4.0, 3.0, 9.0]]).tolist() == [False, True]


def test_union_and_intersect_combine_matches_not_insides():
    a = ("block", 0.0, 2.0, 0.0, 2.0, 0.0, 2.0, "in")
    hole = ("sphere", 1.0, 1.0, 1.0, 0.5, "out")                 # matches outside the ball
    both = ("intersect", [a, hole], "in")                         # the block without the ball
    p = [[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [1.75, 1.0, 1.0], [3.0, 1.0, 1.0]]
    assert rm.match(both, p).tolist() == [False, False, True, False]
    far = ("block", 2.5, 3.5, 0.0, 2.0, 0.0, 2.0, "in")
    nest = ("union", [both, far], "out")
    assert rm.match(nest, p).tolist() == [True, True, False, False]


def test_dynamic_group_needs_the_parent():
    a = ("block", 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, "in")
    x = [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [2.0, 0.5, 0.5]]
    assert rm.dynamic_group([True, False, True], a, x).tolist() == [True, False, False]


def test_schedule_of_a_dynamic_group():
    # run pieces that do not end on multiples of 4: the setup of each run decides at its start, then the multiples of 4
    assert rm.deciding_steps(0, [("run", 3), ("run", 3), ("run", 5), ("run", 0), ("run", 1)], 4) == [0, 4, 8, 11, 12]
    # step() pieces have no setup: only the multiples of 4 (and the first piece after the definition)
    assert rm.deciding_steps(0, [("step", 3), ("step", 3), ("step", 5), ("step", 0), ("step", 1)], 4) == [0, 4, 8, 8, 12]
    assert rm.deciding_steps(5, [("step", 2), ("step", 1), ("run", 1), ("step", 2)], 4) == [5, 8, 8, 8]
    assert rm.deciding_steps(5, [("step", 2), ("step", 1)], 4, defined_before_first=False) == [None, 8]
    assert rm.deciding_steps(6, [("run", 1), ("step", 0), ("run", 0)], 1) == [7, 7, 7]
    assert rm.deciding_steps(2, [("run", 0)], 100) == [2]
