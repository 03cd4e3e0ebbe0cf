"""tests/displace_model.py on the CPU, with dyadic inputs so that every sum and product is exact in IEEE double: the image
bookkeeping undoes the wrap bit for bit, and msd / com of a four-atom case have the values worked out by hand."""
import numpy as np

from tests import displace_model as dm


def test_wrap_and_unmap_give_the_unwrapped_trajectory_bit_for_bit():
    lo, hi = np.array([0.0, -2.0, 1.0]), np.array([4.0, 2.0, 9.0])
    prd = hi - lo
    periodic = (1, 1, 0)
    rng = np.random.default_rng(7)
    n = 64
    x0 = lo + prd * rng.integers(0, 64, (n, 3)) / 64.0           # on a dyadic grid inside the box
    x0[:, 2] = 2.0 + rng.integers(0, 16, n) / 16.0               # z is not periodic and never leaves
    v = rng.choice([-4.0, -1.0, 0.0, 1.0, 2.0], (n, 3))
    v[:, 2] = 0.0
    dt = 2.0 ** -3
    x, image = x0.copy(), np.zeros((n, 3), np.int32)
    seen = np.zeros((n, 3), bool)
    for step in range(1, 257):
        x = x + dt * v                                           # free flight: exact
        if step % 4 == 0:                                        # a rebuild: |dt v| * 4 = 2 < every box length
            before = image.copy()
            x, image = dm.wrap(x, image, lo, hi, periodic)
            seen |= image != before
            assert ((x[:, :2] >= lo[:2]) & (x[:, :2] < hi[:2])).all()
            want = x0 + (step * dt) * v
            got = dm.unmap(x, image, prd)
            assert got.tobytes() == want.tobytes(), step
    assert seen[:, :2].any() and not image[:, 2].any()
    assert image.max() >= 3 and image.min() <= -3                # both directions, several box lengths
    assert abs(dm.unmap(x, image, prd) - x).max() > prd[:2].min()


def test_wrap_moves_one_box_length_per_pass_and_counts_it():
    lo, hi, per = np.zeros(3), np.array([4.0, 4.0, 4.0]), (1, 1, 1)
    x = np.array([[-0.5, 4.0, 3.999], [9.0, -5.0, 0.0]])
    y, im = dm.wrap(x, np.zeros((2, 3), np.int32), lo, hi, per)
    assert y.tolist() == [[3.5, 0.0, 3.999], [5.0, -1.0, 0.0]]    # (the second atom is still outside: one length per pass)
    assert im.tolist() == [[-1, 1, 0], [1, -1, 0]]
    assert dm.unmap(y, im, hi - lo).tolist() == x.tolist()


def test_msd_and_com_of_four_atoms_by_hand():
    prd = np.array([4.0, 4.0, 4.0])
    x = np.array([[1.0, 1.0, 1.0], [3.0, 0.5, 2.0], [0.5, 3.5, 0.25], [2.0, 2.0, 2.0]])
    image = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 2], [0, 0, 0]], np.int32)
    xu = dm.unmap(x, image, prd)
    assert xu.tolist() == [[1.0, 1.0, 1.0], [7.0, 0.5, 2.0], [-3.5, 3.5, 8.25], [2.0, 2.0, 2.0]]
    x0 = np.array([[1.0, 1.0, 1.0], [3.0, 0.5, 2.0], [0.5, 3.5, 0.25], [1.0, 2.0, 4.0]])
    d = dm.displace(xu, x0)
    assert d[:, :3].tolist() == [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [-4.0, 0.0, 8.0], [1.0, 0.0, -2.0]]
    assert d[:, 3].tolist() == [0.0, 4.0, np.sqrt(80.0), np.sqrt(5.0)]
    # means over four atoms: dx^2 (0 + 16 + 16 + 1) / 4, dy^2 0, dz^2 (64 + 4) / 4, their sum
    assert dm.msd(xu, x0).tolist() == [8.25, 0.0, 17.0, 25.25]
    # masses 1 1 2 4: sum m = 8, sum m xu = (1 + 7 - 7 + 8, 1 + 0.5 + 7 + 8, 1 + 2 + 16.5 + 8)
    mass = np.array([1.0, 1.0, 2.0, 4.0])
    assert dm.com(xu, mass).tolist() == [9.0 / 8.0, 16.5 / 8.0, 27.5 / 8.0]
    # com yes: x0 relative to the centre of mass then (cm0), the positions relative to the one now (cm1)
    cm0 = np.array([0.5, 0.5, 0.5])
    cm1 = np.array([1.5, 0.5, 0.0])
    got = dm.msd(xu, x0 - cm0, cm=cm1)
    dd = (xu - cm1) - (x0 - cm0)           # = d - (1, 0, -0.5)
    assert dd.tolist() == [[-1.0, 0.0, 0.5], [3.0, 0.0, 0.5], [-5.0, 0.0, 8.5], [0.0, 0.0, -1.5]]
    assert got.tolist() == [35.0 / 4.0, 0.0, (0.25 + 0.25 + 72.25 + 2.25) / 4.0, (35.0 + 75.0) / 4.0]
    # a group selects the atoms; no atoms: zeros, not NaN
    g = np.array([True, False, False, True])
    assert dm.msd(xu, x0, in_group=g).tolist() == [0.5, 0.0, 2.0, 2.5]
    assert dm.com(xu, mass, in_group=g).tolist() == [9.0 / 5.0, 9.0 / 5.0, 9.0 / 5.0]
    assert dm.displace(xu, x0, in_group=g)[1].tolist() == [0.0, 0.0, 0.0, 0.0]
    none = np.zeros(4, bool)
    assert dm.msd(xu, x0, in_group=none).tolist() == [0.0] * 4 and dm.com(xu, mass, in_group=none).tolist() == [0.0] * 3
