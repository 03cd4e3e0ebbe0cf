"""The rules of the cloud's add / delete schedules as tests/feed_model.py states them, checked on the CPU: the generator
against libc, the region predicate, the add cells and the timer against values worked by hand."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from tests import feed_model as fm


def _libc():
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.srand48.argtypes = [ctypes.c_long]
    libc.srand48.restype = None
    libc.drand48.restype = ctypes.c_double
    return libc


@pytest.mark.parametrize("seed", [1, 7, 4096, 10 ** 6, 2 ** 32 + 7])        # (srand48 takes the low 32 bits of its seed)
def test_generator_and_skip_ahead_equal_libc_drand48(seed):
    libc = _libc()
    libc.srand48(seed)
    want = [libc.drand48() for _ in range(50)]
    g = fm.Lcg48(seed)
    assert [g.next() for _ in range(50)] == want                      # the recurrence, draw for draw
    assert [fm.Lcg48.draw(seed, j) for j in range(50)] == want        # every draw reached by skip-ahead
    g = fm.Lcg48(seed).skip(17)
    assert [g.next() for _ in range(3)] == want[17:20]                # a lane's three draws: skip, then step


def test_positions_use_draws_3i_plus_c():
    libc = _libc()
    libc.srand48(1372)
    u = [libc.drand48() for _ in range(6)]
    c = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    p = fm.positions(c, 0.25, 1372)
    for i in range(2):
        for k in range(3):
            assert p[i, k] == c[i, k] + 0.25 * (0.5 - u[3 * i + k])
    assert np.all(np.abs(p - c) <= 0.125)


def test_point_in_region_box_and_the_product_rule():
    box = (0.0, 1.0, -1.0, 1.0, 2.0, 4.0, 0.0, 0.0, 0.0)
    ecc = (0.0, 0.0, 0.0)
    assert fm.point_in_region(1, box, ecc, (0.5, 0.0, 3.0))
    assert not fm.point_in_region(1, box, ecc, (1.5, 0.0, 3.0))
    assert not fm.point_in_region(1, box, ecc, (0.5, -1.5, 3.0))
    assert not fm.point_in_region(1, box, ecc, (0.5, 0.0, 4.5))
    # exactly on a face, an edge, a corner: the product is 0 < 1e-150
    for p in [(0.0, 0.0, 3.0), (1.0, 0.0, 3.0), (0.5, -1.0, 3.0), (0.5, 1.0, 4.0), (1.0, 1.0, 4.0), (0.0, -1.0, 2.0)]:
        assert fm.point_in_region(1, box, ecc, p), p
    # one ulp outside a face: the product is positive and far above 1e-150
    assert not fm.point_in_region(1, box, ecc, (np.nextafter(1.0, 2.0), 0.0, 3.0))
    # the rule is `< 1e-150`, not `<= 0`: just outside a box thinner than 1e-75 still counts as inside
    tiny = (0.0, 1.0e-80, -1.0, 1.0, 2.0, 4.0, 0.0, 0.0, 0.0)
    assert (2.0e-80 - 0.0) * (2.0e-80 - 1.0e-80) < 1.0e-150
    assert fm.point_in_region(1, tiny, ecc, (2.0e-80, 0.0, 3.0))
    # region kinds 0 and 3: nowhere
    assert not fm.point_in_region(0, box, ecc, (0.5, 0.0, 3.0))
    assert not fm.point_in_region(3, box, ecc, (0.5, 0.0, 3.0))


def test_point_in_region_hollow_cylinder_with_eccentricity():
    # axis (0,0,0)-(0,0,2), r1 = 1, r2 = 3; the inner cylinder is shifted by (0.5, 0, 0)
    cyl = (0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 3.0, 0.0)
    ecc, none = (0.5, 0.0, 0.0), (0.0, 0.0, 0.0)
    assert fm.point_in_region(2, cyl, ecc, (2.0, 0.0, 1.0))          # dsq 4 < 9, dsqE 2.25 > 1
    # (1.2, 0, 1): 1.44 > 1 clears the centred inner cylinder, 0.49 < 1 lies inside the shifted one
    assert fm.point_in_region(2, cyl, none, (1.2, 0.0, 1.0)) and not fm.point_in_region(2, cyl, ecc, (1.2, 0.0, 1.0))
    # (-0.8, 0, 1): the other way round (0.64 < 1, 1.69 > 1)
    assert not fm.point_in_region(2, cyl, none, (-0.8, 0.0, 1.0)) and fm.point_in_region(2, cyl, ecc, (-0.8, 0.0, 1.0))
    # the end planes belong (dot = 0 and dot = h^2 pass), a point beyond does not
    assert fm.point_in_region(2, cyl, ecc, (2.0, 0.0, 0.0)) and fm.point_in_region(2, cyl, ecc, (2.0, 0.0, 2.0))
    assert not fm.point_in_region(2, cyl, ecc, (2.0, 0.0, -1.0e-9))
    assert not fm.point_in_region(2, cyl, ecc, (2.0, 0.0, 2.0 + 1.0e-9))
    # the surfaces themselves do not (strict comparisons): dsq = 9 on the outer one, dsqE = 1 on the shifted inner one
    assert not fm.point_in_region(2, cyl, ecc, (3.0, 0.0, 1.0))
    assert not fm.point_in_region(2, cyl, ecc, (1.5, 0.0, 1.0)) and fm.point_in_region(2, cyl, ecc, (1.5000001, 0.0, 1.0))


def test_cell_centres_uniform_graded_and_labelled():
    c = fm.cell_centres((1.0, 0.0, -1.0), (0.5, 1.0, 2.0), (2, 1, 1))
    assert np.array_equal(c, [[1.25, 0.5, 0.0], [1.75, 0.5, 0.0]])
    c = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1), faces=([0.0, 0.25, 1.0], None, None))
    assert np.array_equal(c, [[0.125, 0.5, 0.5], [0.625, 0.5, 0.5]])
    c = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1), labels=[1, 0])
    assert np.array_equal(c, [[1.5, 0.5, 0.5], [0.5, 0.5, 0.5]])


@pytest.mark.parametrize("factor,want", [(1, [0, 1, 2, 3, 4, 5, 6, 7, 8]), (2, [0, 2, 6, 8]), (3, [0])])
def test_add_cells_3x3x1(factor, want):
    """nine cells inside: nLine = int(9 ** 0.5) = 3; cell i is kept when i % f == 0 and (i // 3) % f == 0"""
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 3, 1))
    box = (0.0, 3.0, 0.0, 3.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    assert fm.add_cells(1, box, (0, 0, 0), centres, factor).tolist() == want


@pytest.mark.parametrize("factor,want", [(1, [16, 17, 18, 19, 36, 37, 38, 39, 56, 57, 58, 59, 76, 77, 78, 79]),
                                         (2, [16, 18, 56, 58]), (3, [16, 19, 76, 79])])
def test_add_cells_top_layer_of_4x5x4(factor, want):
    """the y layer iy = 4 of a 4x5x4 grid: 16 cells with the labels 16 + ix + 20 iz, met in the order i = ix + 4 iz;
    nLine = 4.  Factor 2: i even and iz even.  Factor 3: i in {0, 3, 6, 9, 12, 15} with i // 4 in {0, 3}: i = 0, 3, 12, 15"""
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 5, 4))
    box = (0.0, 4.0, 4.0, 5.0, 0.0, 4.0, 0.0, 0.0, 0.0)
    assert fm.add_cells(1, box, (0, 0, 0), centres, factor).tolist() == want


@pytest.mark.parametrize("factor", [1, 2, 3])
def test_add_cells_whole_4x5x4(factor):
    """all 80 cells: nLine = int(80 ** 0.5) = 8, which is not a row of the grid -- the reference's thinning is by position in
    the list, not by geometry"""
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 5, 4))
    box = (0.0, 4.0, 0.0, 5.0, 0.0, 4.0, 0.0, 0.0, 0.0)
    want = [i for i in range(80) if i % factor == 0 and (i // 8) % factor == 0]
    assert fm.add_cells(1, box, (0, 0, 0), centres, factor).tolist() == want
    assert len(want) == {1: 80, 2: 20, 3: 12}[factor]


def test_timer_over_twelve_sub_cycles():
    """deltaT 1, addParticleTimeStep 2.5: the timer reads 2.5, 1.5, 0.5, -0.5 in front of sub-cycles 1-4, so the fourth one
    adds and resets it; then every fourth"""
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1))
    keys = dict(addParticle=1, addParticleTimeStep=2.5, randomPerturb=0.0, addParticleInfo=(1e-3, 2650.0, 1),
                addParticleBox=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0, 0, 0))
    s = fm.Schedule(keys, centres, 1.0)
    x = np.zeros((0, 3)); tag = np.zeros(0, np.int32); typ = np.zeros(0, np.int32)
    added, timer = [], []
    for k in range(1, 13):
        out = s.sub_cycle(x, tag, typ)
        timer.append(s.time_to_add)
        if out["add"] is not None:
            added.append(k)
            x = np.vstack([x, out["add"]["pos"]]); tag = np.append(tag, out["add"]["tags"]); typ = np.append(typ, 1)
    assert added == [4, 8, 12]
    assert timer == [1.5, 0.5, -0.5, 2.5, 1.5, 0.5, -0.5, 2.5, 1.5, 0.5, -0.5, 2.5]
    assert tag.tolist() == [1, 2, 3] and s.totalAdd == 3 and s.totalDelete == 0


def test_tags_follow_the_largest_tag_left_after_the_clearing():
    """maxTag is found anew at every add, after the clearing: the tag of a cleared grain is handed out again.  A grain the
    clearing took is not counted as deleted as well, although it also lies in deleteParticleBox"""
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
    keys = dict(addParticle=1, deleteParticle=1, deleteBeforeAdd=1, addParticleTimeStep=0.0, randomPerturb=0.0,
                addParticleInfo=(1e-3, 2650.0, 2), addParticleBox=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0, 0, 0, 0),
                clearInitialBox=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0, 0, 0, 0), deleteParticleBox=(0.0, 2.0, 0.0, 5.0, 0.0, 1.0, 0, 0, 0))
    s = fm.Schedule(keys, centres, 1.0)
    s.time_to_add = 0.0
    x = np.array([[0.5, 0.5, 0.5], [0.5, 3.0, 0.5], [0.5, 0.5, 0.5], [0.5, 9.0, 0.5]])
    tag = np.array([9, 4, 2, 5]); typ = np.array([1, 1, 2, 1])
    out = s.sub_cycle(x, tag, typ)
    assert out["clear"].tolist() == [9]                    # type 1 inside clearInitialBox; the type-2 grain there stays
    assert out["add"]["tags"].tolist() == [6, 7]           # the largest tag left is 5
    assert out["delete"].tolist() == [4]
    assert (s.totalAdd, s.totalDelete, s.totalDeleteBeforeAdd) == (2, 1, 1)
    # seed: 4 grains - 1 cleared + 2 added - 1 deleted
    assert np.array_equal(out["add"]["pos"], fm.positions(centres, 0.0, 4))


def test_reference_quirks_of_the_switches():
    centres = fm.cell_centres((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1))
    x = np.array([[0.5, 0.5, 0.5]]); tag = np.array([1]); typ = np.array([1])
    everywhere = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0, 0, 0)
    # deleteParticle with addParticle 0: pointInRegion is false for region kind 0
    s = fm.Schedule(dict(deleteParticle=1, deleteParticleBox=everywhere), centres, 1.0)
    assert s.sub_cycle(x, tag, typ)["delete"].size == 0 and s.time_to_add > 1e149
    # deleteBeforeAdd with deleteParticle 0 clears nothing
    s = fm.Schedule(dict(addParticle=1, deleteBeforeAdd=1, clearInitialBox=everywhere, addParticleTimeStep=0.0,
                         randomPerturb=0.0, addParticleInfo=(1e-3, 2650.0, 1), addParticleBox=everywhere), centres, 1.0)
    s.time_to_add = 0.0
    out = s.sub_cycle(x, tag, typ)
    assert out["clear"].size == 0 and out["add"]["tags"].tolist() == [2]
