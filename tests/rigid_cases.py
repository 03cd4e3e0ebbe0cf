"""Systems for the fix rigid/nve tests (tests/test_rigid_model.py, tests/test_rigid_gpu.py): bodies of non-touching spheres
far apart from each other, so that gravity and constant per-atom forces are all that acts on them."""
import numpy as np

DENSITY = 2500.0


def clumps(nbody, seed, nfree=0, nmin=3, nmax=8, spacing=2.0):
    """`nbody` bodies of nmin..nmax spheres (radius 0.05-0.1, centres at least 2.5 radii apart inside a body, so that they
    never touch and the principal moments are distinct) on a cubic grid of `spacing`, then `nfree` free spheres on the next
    grid points; random velocities and spins per ATOM (the set-up makes them rigid); constant random forces per atom.
    Molecule IDs are 1..nbody for body atoms and 0 for the free ones; tags 1..n in creation order."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil((nbody + nfree) ** (1.0 / 3.0)))
    x, r, mol = [], [], []
    for b in range(nbody + nfree):
        c = spacing * (np.array([b % side, (b // side) % side, b // (side * side)], dtype=float) + 0.5)
        if b >= nbody:
            x.append(c)
            r.append(rng.uniform(0.05, 0.1))
            mol.append(0)
            continue
        na = int(rng.integers(nmin, nmax + 1))
        pts, rad = [], []
        while len(pts) < na:
            p = rng.uniform(-0.3, 0.3, 3)
            rr = rng.uniform(0.05, 0.1)
            if all(np.linalg.norm(p - q) > 2.5 * 0.1 for q in pts):
                pts.append(p)
                rad.append(rr)
        x += [c + p for p in pts]
        r += rad
        mol += [b + 1] * na
    x, r, mol = np.array(x), np.array(r), np.array(mol, dtype=np.int32)
    n = len(r)
    L = spacing * side
    # (gravity pulls along -y for 0.2 s: room below)
    lo, hi = np.array([0.0, -2.0, 0.0]), np.array([L, L, L])
    return dict(n=n, x=x, v=rng.uniform(-0.5, 0.5, (n, 3)), omega=rng.uniform(-3.0, 3.0, (n, 3)), diameter=2.0 * r,
                density=np.full(n, DENSITY), mol=mol, tag=np.arange(1, n + 1, dtype=np.int32),
                type=np.where(mol > 0, 1, 2).astype(np.int32), boxlo=lo, boxhi=hi, periodic=(0, 0, 0),
                fext=rng.uniform(-1.0, 1.0, (n, 3)) * (4.0 / 3.0 * np.pi * r ** 3 * DENSITY * 9.81)[:, None])


def mass_of(case):
    r = 0.5 * case["diameter"]
    # (the engine's expression, DemEngine::create_atoms: 4 pi / 3 r r r density)
    return 4.0 * np.pi / 3.0 * r * r * r * case["density"]


def model_of(case, dt, order=None, body=None, dtype=np.float64):
    """tests/rigid_model.RigidModel of a case with the atoms handed over in `order` (default: as created); body: per-atom
    body index (default: molecule ID - 1)"""
    from tests.rigid_model import RigidModel
    o = np.arange(case["n"]) if order is None else np.asarray(order)
    b = (case["mol"].astype(np.int64) - 1) if body is None else np.asarray(body)
    m = RigidModel(case["x"][o], case["v"][o], case["omega"][o], 0.5 * case["diameter"][o], mass_of(case)[o], b[o],
                   case["boxlo"], case["boxhi"], case["periodic"], dt, dtype=dtype, tag=case["tag"][o])
    m.order = o
    return m


def model_results(m):
    """what the tests compare, atoms back in creation order"""
    inv = np.argsort(m.order)
    return dict(x=m.x[inv], v=m.v[inv], omega=m.w[inv], xcm=m.xcm, vcm=m.vcm, fcm=m.fcm, torque=m.tq, angmom=m.L,
                omega_body=m.om, masstotal=m.M, inertia_space=m.inertia_space())


def rel_diff(a, b):
    """the largest difference over the largest magnitude, per quantity"""
    out = {}
    for k in b:
        s = float(np.max(np.abs(np.asarray(b[k], dtype=np.float64))))
        out[k] = float(np.max(np.abs(np.asarray(a[k], dtype=np.float64) - np.asarray(b[k], dtype=np.float64)))) / (s if s > 0 else 1.0)
    return out
