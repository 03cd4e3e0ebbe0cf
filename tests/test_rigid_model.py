"""Self-checks of tests/rigid_model.py, the float64 restatement of the fix rigid/nve rules the GPU tests compare with
(tests/test_rigid_gpu.py).  CPU only."""
import numpy as np

from tests import rigid_cases as rc
from tests.rigid_model import RigidModel


def _asymmetric_body(dtype):
    # five spheres, no symmetry: three distinct principal moments
    x = np.array([[0.0, 0.0, 0.0], [0.31, 0.02, -0.05], [-0.07, 0.27, 0.11], [0.13, -0.22, 0.29], [-0.25, -0.09, -0.19]])
    r = np.array([0.05, 0.08, 0.06, 0.09, 0.07])
    m = 4.0 * np.pi / 3.0 * r ** 3 * 2500.0
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, (5, 3))
    w = rng.uniform(-20.0, 20.0, (5, 3))
    return RigidModel(x + 5.0, v, w, r, m, np.zeros(5, int), [0, 0, 0], [10, 10, 10], (0, 0, 0), 1e-4, dtype=dtype)


def test_force_free_asymmetric_body_conserves_angular_momentum_and_rotational_energy():
    """10^4 force-free steps.  The splitting keeps |angmom| up to rounding and the rotational energy up to its own O(dt^2)
    oscillation.  Tolerance: what the same model shows in np.longdouble (the scheme's error, rounding 2^-11 of float64's)
    plus a rounding allowance for float64 of 10 roundings per step, steps x 10 x eps -- reasoning, not a fit."""
    nsteps, chunk = 10000, 100
    drift = {}
    for T in (np.longdouble, np.float64):
        m = _asymmetric_body(T)
        assert np.all(m.I > 0) and len(set(np.round(np.asarray(m.I[0], float) / float(m.I.max()), 6))) == 3
        zero = np.zeros((5, 3))
        m.setup_forces(zero, [0, 0, 0])
        L0, E0 = np.sqrt(np.sum(m.L ** 2)), m.rotational_energy()[0]
        dL = dE = 0.0
        for _ in range(nsteps // chunk):
            m.step(chunk, zero, [0, 0, 0])
            dL = max(dL, float(abs(np.sqrt(np.sum(m.L ** 2)) - L0) / L0))
            dE = max(dE, float(abs(m.rotational_energy()[0] - E0) / E0))
        drift[T] = (dL, dE)
    allowance = nsteps * 10 * np.finfo(np.float64).eps
    print("drift |L|, E: longdouble %.3e %.3e  float64 %.3e %.3e  allowance %.3e" % (drift[np.longdouble] + drift[np.float64] + (allowance,)))
    assert drift[np.float64][0] <= drift[np.longdouble][0] + allowance
    assert drift[np.float64][1] <= drift[np.longdouble][1] + allowance
    assert drift[np.longdouble][1] < 1e-6   # (the scheme itself: energy oscillates, it does not run away)


def test_free_fall_is_exact():
    """gravity alone: the centre of mass follows the scalar velocity-Verlet recurrence bit for bit, and the parabola to
    n eps; the body does not start to turn"""
    case = rc.clumps(3, seed=2)
    case["v"][:] = [0.3, -0.2, 0.1]
    case["omega"][:] = 0.0
    dt, n, g = 1e-4, 500, np.array([0.0, -9.81, 0.0])
    m = rc.model_of(case, dt)
    zero = np.zeros((case["n"], 3))
    m.setup_forces(zero, g)
    x0, v0, M = m.xcm.copy(), m.vcm.copy(), m.M.copy()
    fcm0 = m.fcm.copy()
    m.step(n, zero, g)
    x, v = x0.copy(), v0.copy()
    for _ in range(n):
        v = v + 0.5 * dt * fcm0 / M[:, None]
        x = x + dt * v
        v = v + 0.5 * dt * fcm0 / M[:, None]
    assert np.array_equal(m.fcm, fcm0)
    assert np.array_equal(m.xcm, x) and np.array_equal(m.vcm, v)
    t = n * dt
    exact = x0 + v0 * t + 0.5 * g * t * t
    assert np.max(np.abs(m.xcm - exact)) <= n * np.finfo(float).eps * np.max(np.abs(exact))
    assert np.max(np.abs(m.om)) <= n * np.finfo(float).eps * 1.0   # (torque of gravity about the centre of mass: rounding)


def test_the_model_does_not_depend_on_the_order_of_the_atoms_beyond_rounding():
    """the measurement behind ORDER_DIFF of tests/test_rigid_gpu.py, on a short run (the 2000-step figure is recorded
    there and in DESIGN.md section 11)"""
    case = rc.clumps(40, seed=11, nfree=3)
    g = np.array([0.0, -9.81, 0.0])
    res = []
    for order in (None, np.arange(case["n"])[::-1]):
        m = rc.model_of(case, 1e-4, order)
        m.setup_forces(case["fext"][m.order], g)
        m.step(200, case["fext"][m.order], g)
        res.append(rc.model_results(m))
    d = rc.rel_diff(res[1], res[0])
    print(d)
    assert max(d.values()) < 1e-12
