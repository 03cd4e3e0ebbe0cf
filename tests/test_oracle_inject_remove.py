"""Known answers of the oracle's particle injection and removal (oracle/orc_dem.c: orc_dem_add_atoms,
orc_dem_delete_atoms), which do not go through the engine.  The contract is the product's: the survivors' history is
kept by partner tag and the lists are rebuilt at the call, before the next force -- not the reference's stale list
(library.cpp:587-592, :611).  Pairs that never meet cannot influence each other, and a one-pair list has no summation
order to change: a pair that survives a removal, or that was there before an injection, must go on bit for bit as if it
had always been alone."""
import numpy as np
import pytest

from oracle import binding as ob

R = 0.5e-3
RHO = 2500.0
LO, HI = [0.0, 0.0, 0.0], [20e-3, 10e-3, 10e-3]
KEYS = ("x", "v", "omega", "f", "torque")


def _mass(r, rho):
    return 4.0 * np.pi / 3.0 * r ** 3 * rho


def _oracle(x, v, omega, tag):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    dem = ob.OracleDem(x, np.full(n, R), np.full(n, _mass(R, RHO)), LO, HI, periodic=(0, 0, 0), v=v, omega=omega, tag=tag)
    dem.pair_gran("hertz", 1.0e7, None, 0.5, None, 0.4, 1)
    dem.fix_fdrag(0.0)
    dem.neighbor(0.25e-3)
    dem.timestep(1.0e-6)
    return dem


def _pair(x0, tags, spin):
    """two grains overlapping by 0.02 mm along x, offset in y, counter-rotating: the contact slides from the first step"""
    x = [[x0, 5.0e-3, 5.0e-3], [x0 + 0.98e-3 * np.cos(0.2), 5.0e-3 + 0.98e-3 * np.sin(0.2), 5.0e-3]]
    v = [[0.05, 0.0, 0.01], [-0.05, 0.02, 0.0]]
    om = [[0.0, 30.0, spin], [10.0, 0.0, spin]]
    return dict(x=x, v=v, omega=om, tag=list(tags))


def _join(*parts):
    return {k: sum((p[k] for p in parts), []) for k in ("x", "v", "omega", "tag")}


def _rows(state, tags):
    sel = np.isin(state["tag"], tags)
    return {k: state[k][sel] for k in KEYS + ("tag",)}


def _same(a, b):
    assert np.array_equal(a["tag"], b["tag"])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("dead", [(1, 2), (3, 4)], ids=["first_pair_leaves", "last_pair_leaves"])
def test_two_pairs_far_apart_deletion(dead):
    pa, pb = _pair(2.0e-3, (1, 2), 40.0), _pair(12.0e-3, (3, 4), -25.0)
    keep = (3, 4) if dead == (1, 2) else (1, 2)
    both = _oracle(**_join(pa, pb))
    solo = _oracle(**(pb if dead == (1, 2) else pa))
    both.setup(); solo.setup()
    both.run(20); solo.run(20)
    h0 = both.history()
    assert set(h0) == {(1, 2), (3, 4)} and all(np.all(s != 0.0) for s in h0.values())
    nb = both.nbuilds
    assert both.delete_particle(list(dead)) == 2
    assert both.nlocal == 2 and both.nbuilds == nb + 1
    h1 = both.history()
    assert set(h1) == {keep} and np.array_equal(h1[keep], h0[keep])
    _same(both.get(), solo.get())                   # nothing moved at the call
    both.run(50); solo.run(50)
    _same(both.get(), solo.get())
    hs = solo.history()
    assert set(both.history()) == set(hs) == {keep} and np.array_equal(both.history()[keep], hs[keep])


def test_two_pairs_far_apart_injection():
    """The created pair: two grains of another size and density, each created by its own call (one velocity per call), a
    0.004 mm gap apart and closing at 0.2 m/s off-centre: not touching at the creation, so that a fresh oracle's setup
    evaluation gives the zero force the created atoms start with; in contact, sliding, within the 50 steps."""
    pa = _pair(2.0e-3, (1, 2), 40.0)
    run, ref = _oracle(**pa), _oracle(**pa)
    run.setup(); ref.setup()
    run.run(20); ref.run(20)
    d, rho = 0.8e-3, 2000.0
    xn = np.array([[12.0e-3, 5.0e-3, 5.0e-3], [12.0e-3 + 0.804e-3 * np.cos(0.3), 5.0e-3 + 0.804e-3 * np.sin(0.3), 5.0e-3]])
    vn = np.array([[0.1, 0.0, 0.0], [-0.1, 0.0, 0.0]])
    nb = run.nbuilds
    h0 = run.history()
    run.create_particle(xn[0], [7], d, rho, 1, vn[0])
    run.create_particle(xn[1], [9], d, rho, 1, vn[1])
    assert run.nlocal == 4 and run.nbuilds == nb + 2
    h1 = run.history()
    assert set(h1) == {(1, 2)} and np.array_equal(h1[(1, 2)], h0[(1, 2)])
    r = 0.5 * d
    m = 4.0 * 3.14159265358917323846 / 3.0 * r * r * r * rho        # library.cpp:460, its literal
    fresh = ob.OracleDem(xn, [r, r], [m, m], LO, HI, periodic=(0, 0, 0), v=vn, tag=[7, 9])
    fresh.pair_gran("hertz", 1.0e7, None, 0.5, None, 0.4, 1)
    fresh.fix_fdrag(0.0); fresh.neighbor(0.25e-3); fresh.timestep(1.0e-6)
    fresh.setup()
    assert np.all(fresh.get()["f"] == 0.0)
    run.run(50); ref.run(50); fresh.run(50)
    st = run.get()
    _same(_rows(st, [1, 2]), ref.get())
    _same(_rows(st, [7, 9]), fresh.get())
    h, hf = run.history(), fresh.history()
    assert set(h) == {(1, 2), (7, 9)} and set(hf) == {(7, 9)}
    assert np.any(hf[(7, 9)] != 0.0) and np.array_equal(h[(7, 9)], hf[(7, 9)])
    assert np.array_equal(h[(1, 2)], ref.history()[(1, 2)])


@pytest.mark.parametrize("dead,keep", [(3, (1, 2)), (1, (2, 3))], ids=["last_leaves", "first_leaves_rows_shift"])
def test_chain_of_three_sliding_contacts(dead, keep):
    x = [[2.0e-3, 5.0e-3, 5.0e-3], [2.98e-3, 5.0e-3, 5.0e-3], [3.96e-3, 5.0e-3, 5.0e-3]]
    om = [[0.0, 40.0, 20.0], [0.0, -30.0, 10.0], [15.0, 25.0, -20.0]]
    v = [[0.0, 0.02, 0.0], [0.0, -0.02, 0.01], [0.0, 0.0, -0.03]]
    dem = _oracle(x, v, om, [1, 2, 3])
    dem.setup()
    dem.run(25)
    h0 = dem.history()
    assert set(h0) == {(1, 2), (2, 3)}
    assert all(np.all(s != 0.0) for s in h0.values())            # three live shear components per contact
    nb = dem.nbuilds
    before = dem.get()
    assert dem.delete_particle([dead]) == 1
    assert dem.nlocal == 2 and dem.nbuilds == nb + 1
    h1 = dem.history()
    assert set(h1) == {keep} and np.array_equal(h1[keep], h0[keep])
    _same(dem.get(), _rows(before, list(keep)))                 # records and stored forces travel with their atoms
    dem.run(10)
    assert set(dem.history()) == {keep}


def test_unknown_and_duplicate_tags():
    dem = _oracle(**_join(_pair(2.0e-3, (1, 2), 40.0), _pair(12.0e-3, (3, 4), -25.0)))
    dem.setup()
    dem.run(10)
    nb, h0, s0 = dem.nbuilds, dem.history(), dem.get()
    assert dem.delete_particle([77, 1000]) == 0
    assert dem.nbuilds == nb and dem.nlocal == 4
    _same(dem.get(), s0)
    assert dem.delete_particle([4, 4, 77]) == 1
    assert dem.nlocal == 3 and dem.get()["tag"].tolist() == [1, 2, 3]
    assert set(dem.history()) == {(1, 2)} and np.array_equal(dem.history()[(1, 2)], h0[(1, 2)])


def test_before_setup_atoms_only_join_and_leave():
    """no list yet: nothing is built at the call; the first setup sees the resulting set"""
    dem = _oracle(**_join(_pair(2.0e-3, (1, 2), 40.0), _pair(12.0e-3, (3, 4), -25.0)))
    assert dem.delete_particle([1, 2]) == 2
    dem.create_particle([[6.0e-3, 5.0e-3, 5.0e-3]], [11], 0.8e-3, 2000.0, 1, [0.0, 0.0, 0.0])
    assert dem.nbuilds == 0 and dem.nlocal == 3 and dem.get()["tag"].tolist() == [3, 4, 11]
    solo = _oracle(**_pair(12.0e-3, (3, 4), -25.0))
    dem.setup(); solo.setup()
    dem.run(30); solo.run(30)
    _same(_rows(dem.get(), [3, 4]), solo.get())
    assert dem.nbuilds >= 1


def test_mass_of_a_created_atom_is_the_literal_product():
    dem = _oracle(**_pair(2.0e-3, (1, 2), 40.0))
    d, rho = 0.8e-3, 2000.0
    dem.create_particle([[8.0e-3, 5.0e-3, 5.0e-3]], [5], d, rho, 1, [0.0, 0.0, 0.0])
    r = 0.5 * d
    want = 4.0 * 3.14159265358917323846 / 3.0 * r * r * r * rho
    true_pi = 4.0 * np.pi / 3.0 * r * r * r * rho
    assert want != true_pi and abs(want / true_pi - 1.0) < 1e-12      # the bound of 1e-12 cannot tell them apart, == can
    m = dem.mass()
    assert m[2] == want and m[0] == _mass(R, RHO)
