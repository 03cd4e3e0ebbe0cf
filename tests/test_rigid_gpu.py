"""fix rigid/nve on the GPU (csrc/sf_rigid.hip) against the float64 model of its rules (tests/rigid_model.py), against the
oracle's fix nve/sphere for bodies of one sphere, and against the invariants of a rigid body.  Tolerances and where
they come from are next to the constants."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import binding as ob
from sedifoam_amd import Lammps, SfError, synthetic
from tests import dem_cases as dc
from tests import rigid_cases as rc

pytestmark = pytest.mark.gpu

G = np.array([0.0, -9.81, 0.0])
# Model against GPU.  Summation order is the engine's freedom, so the yardstick is the model against itself with the atoms
# in two orders: clumps(500, seed=11, nfree=20), dt 1e-4, 2000 steps, creation order against reversed order -- the largest
# relative difference (largest difference over largest magnitude, per quantity) was 6.9e-14, in omega (a random permutation
# gave 5.2e-14).  Times 10 for the engine's fused multiply-adds, folded constants and v_rcp / v_rsq seeds.
ORDER_DIFF = 6.9e-14
MODEL_TOL = 10.0 * ORDER_DIFF
# Bodies of one sphere against the oracle's fix nve/sphere: the yardstick is what the fix nve/sphere path of the same library
# (the code a script without the fix runs, unchanged by this fix) differs from the oracle by on the same bed over the same
# 100 sub-steps, times 10 because the rigid path rounds about ten times as often per step.  The test measures that
# difference in the same process and prints both figures.


def _engine(case, dt=1e-4, skin=0.05, pair="gran/hooke/history 2.0e5 NULL 50.0 NULL 0.5 0", order=None, args=None):
    o = np.arange(case["n"]) if order is None else np.asarray(order)
    lmp = Lammps(args=args)
    lmp.set_box(case["boxlo"], case["boxhi"])
    lmp.create_atoms(case["x"][o], case["diameter"][o], case["density"][o], v=case["v"][o], omega=case["omega"][o],
                     type_=case["type"][o], tag=case["tag"][o])
    for line in ("atom_style sphere", "boundary %s %s %s" % tuple("p" if q else "f" for q in case["periodic"]),
                 "newton off", "communicate single vel yes", "neighbor %.17g bin" % skin, "neigh_modify delay 0",
                 "pair_style " + pair, "pair_coeff * *", "timestep %.17g" % dt):
        lmp.command(line)
    return lmp


def _forces_on(lmp, case, g=9.81):
    lmp.command("fix grav all gravity %.17g vector 0 -1 0" % g)
    lmp.command("fix drag all fdrag")
    lmp.put_local_info(case["fext"], case["tag"])


def _gpu_results(lmp):
    st, rb = lmp.get_state(), lmp.rigid_bodies()
    ex = np.empty((len(rb["quat"]), 3, 3))
    w, x, y, z = rb["quat"].T
    ex[:, :, 0] = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y)], axis=1)
    ex[:, :, 1] = np.stack([2 * (x * y - w * z), w * w - x * x + y * y - z * z, 2 * (y * z + w * x)], axis=1)
    ex[:, :, 2] = np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z], axis=1)
    return dict(x=st["x"], v=st["v"], omega=st["omega"], xcm=rb["xcm"], vcm=rb["vcm"], fcm=rb["fcm"], torque=rb["torque"],
                angmom=rb["angmom"], omega_body=rb["omega"], masstotal=rb["masstotal"],
                inertia_space=np.einsum("bik,bk,bjk->bij", ex, rb["inertia"], ex))


def _against_model(lmp, case, body, nsteps, dt=1e-4):
    m = rc.model_of(case, dt, body=body)
    m.setup_forces(case["fext"], G)
    m.step(nsteps, case["fext"], G)
    d = rc.rel_diff(_gpu_results(lmp), rc.model_results(m))
    print("GPU against the model, relative:", {k: "%.2e" % v for k, v in d.items()})
    return d


def test_500_molecule_bodies_and_free_atoms_follow_the_model():
    """500 bodies of 3-8 spheres under `molecule`, 20 free spheres under fix nve/sphere, gravity and constant per-atom
    forces through fix fdrag, 2000 steps across several list rebuilds"""
    case = rc.clumps(500, seed=11, nfree=20)
    lmp = _engine(case)
    lmp.command("fix molprop all property/atom mol")
    lmp.set_molecule(case["tag"], case["mol"])
    lmp.command("group clump type 1")
    lmp.command("group free type 2")
    lmp.command("fix 1 clump rigid/nve molecule")
    lmp.command("fix 2 free nve/sphere")
    _forces_on(lmp, case)
    lmp.setup()
    b0 = lmp.info().nbuilds
    lmp.step(2000)
    rb = lmp.rigid_bodies()
    assert len(rb["natoms"]) == 500 and rb["natoms"].tolist() == np.bincount(case["mol"])[1:].tolist()
    print("list builds during the run:", lmp.info().nbuilds - b0)
    assert lmp.info().nbuilds - b0 >= 4
    d = _against_model(lmp, case, case["mol"].astype(np.int64) - 1, 2000)
    assert max(d.values()) <= MODEL_TOL, d


def test_three_group_bodies_follow_the_model():
    case = rc.clumps(3, seed=21)
    case["type"] = case["mol"].copy()
    lmp = _engine(case)
    for k in (1, 2, 3):
        lmp.command("group b%d type %d" % (k, k))
    lmp.command("fix 1 all rigid/nve group 3 b1 b2 b3")
    _forces_on(lmp, case)
    lmp.step(2000)
    d = _against_model(lmp, case, case["mol"].astype(np.int64) - 1, 2000)
    assert max(d.values()) <= MODEL_TOL, d


def test_one_single_body_follows_the_model():
    case = rc.clumps(1, seed=31, nmin=8, nmax=8)
    lmp = _engine(case)
    lmp.command("fix 1 all rigid/nve single")
    _forces_on(lmp, case)
    lmp.step(2000)
    d = _against_model(lmp, case, np.zeros(case["n"], np.int64), 2000)
    assert max(d.values()) <= MODEL_TOL, d


def _hertz_bed():
    bed = synthetic.fcc_bed((6, 5, 6), seed=2024)
    cfg = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6, skin=0.25e-3,
               walls=[(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))])
    return bed, cfg


def test_single_sphere_bodies_equal_fix_nve_sphere():
    """Every atom of a small Hertz bed its own molecule under `rigid/nve molecule` against the oracle's fix nve/sphere
    over 100 sub-steps: the body-mass pair law with body mass = own mass, the force hand-off, walls.
    The bound is ten times what fix nve/sphere itself differs from the oracle by, measured here on the same bed."""
    bed, cfg = _hertz_bed()
    n = len(bed["x"])
    orc = dc.make_oracle(bed, cfg)
    orc.setup(); orc.run(100)
    ref = orc.get()
    par = dc.make_hip(bed, cfg)
    par.step(100)
    a = par.get_state()
    pdx, pdf = float(np.max(np.abs(a["x"] - ref["x"]))), dc.rel_err(a["f"], ref["f"])
    pdv, pdw = dc.rel_err(a["v"], ref["v"]), dc.rel_err(a["omega"], ref["omega"])
    lmp = Lammps()
    lmp.set_box(bed["boxlo"], bed["boxhi"])
    lmp.create_atoms(bed["x"], bed["diameter"], bed["density"], v=bed["v"], omega=bed.get("omega"))
    lmp.set_molecule(np.arange(1, n + 1), np.arange(1, n + 1))
    for line in dc.script_lines(bed, cfg):
        lmp.command("fix 1 all rigid/nve molecule" if line == "fix 1 all nve/sphere" else line)
    lmp.step(100)
    b = lmp.get_state()
    rdx, rdf = float(np.max(np.abs(b["x"] - ref["x"]))), dc.rel_err(b["f"], ref["f"])
    rdv, rdw = dc.rel_err(b["v"], ref["v"]), dc.rel_err(b["omega"], ref["omega"])
    print("fix nve/sphere against the oracle: max|dx| %.3e m, rel|df| %.3e, rel|dv| %.3e, rel|domega| %.3e ; rigid/nve "
          "molecule: max|dx| %.3e m, rel|df| %.3e, rel|dv| %.3e, rel|domega| %.3e" % (pdx, pdf, pdv, pdw, rdx, rdf, rdv, rdw))
    assert lmp.rigid_bodies()["natoms"].tolist() == [1] * n
    assert rdx <= 10.0 * pdx and rdf <= 10.0 * pdf
    assert rdv <= 10.0 * pdv and rdw <= 10.0 * pdw


def _two_bodies():
    """two rows of four spheres along x (2.5 r apart inside a row: not touching), approaching head-on along x; the two
    lead spheres overlap by 1 % of a radius"""
    r = 0.05
    xs = np.array([-(0.995 * r) - 2.5 * r * k for k in range(4)] + [(0.995 * r) + 2.5 * r * k for k in range(4)])
    x = np.stack([xs + 2.0, np.full(8, 1.0), np.full(8, 1.0)], axis=1)
    v = np.zeros((8, 3))
    v[:4, 0], v[4:, 0] = 0.7, -0.4
    return dict(n=8, x=x, v=v, omega=np.zeros((8, 3)), diameter=np.full(8, 2 * r), density=np.full(8, rc.DENSITY),
                mol=np.array([1] * 4 + [2] * 4, np.int32), tag=np.arange(1, 9, dtype=np.int32), type=np.ones(8, np.int32),
                boxlo=np.zeros(3), boxhi=np.array([4.0, 2.0, 2.0]), periodic=(0, 0, 0))


def test_a_body_atom_collides_with_the_mass_of_its_body():
    """the contact force of the first overlap against the oracle's pair function with the body masses substituted the way
    tests/test_reference_pins.py does it; the same spheres free against the same function with their own masses.  Hooke
    with velocity damping: meff enters through gamman.  1e-12: a handful of operations at 1-2 ulp each."""
    case = _two_bodies()
    kn, gn = 2.0e5, 500.0
    pair = "gran/hooke/history %.17g NULL %.17g NULL 0.5 1" % (kn, gn)
    m = rc.mass_of(case)
    L = ob.lib()
    p = ob.GranParams()
    assert L.orc_gran_settings(C.byref(p), kn, 1, 0.0, gn, 1, 0.0, 0.5, 1, 1.0) == 0

    def oracle_force(mass):
        ij = np.array([0, 4])   # the two lead spheres
        first, jl, ilist = np.array([0, 1, 1], np.int32), np.array([1], np.int32), np.arange(2, dtype=np.int32)
        touch, shear = np.zeros(1, np.int32), np.zeros(3)
        nl = ob.NeighList(2, ob.P(ilist), ob.P(first), ob.P(jl), ob.P(touch), ob.P(shear))
        f, tq = np.zeros((2, 3)), np.zeros((2, 3))
        L.orc_pair_gran_hooke_history(C.byref(p), 1e-6, 0, 2, ob.P(ob.f64(case["x"][ij])), ob.P(ob.f64(case["v"][ij])),
                                      ob.P(ob.f64(case["omega"][ij])), ob.P(ob.f64(0.5 * case["diameter"][ij])),
                                      ob.P(ob.f64(mass)), ob.P(ob.i32(np.ones(2))), 0, C.byref(nl), ob.P(f), ob.P(tq))
        return f

    rigid = _engine(case, dt=1e-6, skin=0.01, pair=pair)
    rigid.set_molecule(case["tag"], case["mol"])
    rigid.command("fix 1 all rigid/nve molecule")
    rigid.setup()
    free = _engine(case, dt=1e-6, skin=0.01, pair=pair)
    free.command("fix 1 all nve/sphere")
    free.setup()
    fr, ff = rigid.get_state()["f"][[0, 4]], free.get_state()["f"][[0, 4]]
    er, ef = oracle_force(np.array([m[:4].sum(), m[4:].sum()])), oracle_force(m[[0, 4]])
    print("force on the lead sphere: bodies %.17g (oracle %.17g), free %.17g (oracle %.17g)" % (fr[0, 0], er[0, 0], ff[0, 0], ef[0, 0]))
    assert abs(er[0, 0] - ef[0, 0]) > 0.1 * abs(ef[0, 0])   # (the masses matter in this set-up)
    assert dc.rel_err(fr, er) <= 1e-12 and dc.rel_err(ff, ef) <= 1e-12
    assert np.allclose(rigid.rigid_bodies()["fcm"][:, 0], [fr[0, 0], fr[1, 0]], rtol=1e-12)


def _block(nx=33, ny=20, nz=33):
    """a lattice block like cases/development-testing/fallingBlock_porosity03: spacing 0.000606, d 0.0005, rho 2650"""
    s, d = 0.000606, 0.0005
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    x = np.stack([i.ravel() * s + 0.003, j.ravel() * s + 0.5 * d + 2.0e-6, k.ravel() * s + 0.003], axis=1)
    n = len(x)
    v = np.zeros((n, 3))
    v[:, 1] = -0.05
    return dict(n=n, x=x, v=v, omega=np.zeros((n, 3)), diameter=np.full(n, d), density=np.full(n, 2650.0),
                mol=np.ones(n, np.int32), tag=np.arange(1, n + 1, dtype=np.int32), type=np.ones(n, np.int32),
                boxlo=np.array([0.0, -0.001, 0.0]), boxhi=np.array([0.026, 0.02, 0.026]), periodic=(0, 0, 0),
                fext=np.zeros((n, 3)))


def _rigid_invariants(st, om, pairs, dist0, vtol=1e-12):
    x, v = st["x"], st["v"]
    dist = np.linalg.norm(x[pairs[:, 0]] - x[pairs[:, 1]], axis=1)
    e_d = float(np.max(np.abs(dist - dist0) / dist0))
    assert np.array_equal(st["omega"], np.broadcast_to(om, st["omega"].shape))   # omega_i = omega, exactly
    dv = v[pairs[:, 0]] - v[pairs[:, 1]] - np.cross(om, x[pairs[:, 0]] - x[pairs[:, 1]])
    e_v = float(np.max(np.abs(dv)) / max(np.max(np.abs(v)), 1e-300))
    return e_d, e_v


def test_falling_block_of_21780_spheres_stays_rigid_through_a_bounce():
    case = _block()
    assert case["n"] == 21780
    dt = 1.0e-6
    lmp = _engine(case, dt=dt, skin=0.0002, pair="gran/hooke/history 150.0 NULL 0.0 NULL 0.4 0")
    lmp.command("fix 1 all rigid/nve single")
    _forces_on(lmp, case)
    lmp.command("fix w all wall/gran 150.0 NULL 0.0 NULL 0.4 0 yplane 0.0 NULL")
    lmp.setup()
    rb0 = lmp.rigid_bodies()
    x0, v0 = rb0["xcm"][0].copy(), rb0["vcm"][0].copy()
    rng = np.random.default_rng(3)
    pairs = rng.integers(0, case["n"], (200, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    st0 = lmp.get_state()
    dist0 = np.linalg.norm(st0["x"][pairs[:, 0]] - st0["x"][pairs[:, 1]], axis=1)
    # before first wall contact (2 um gap at 0.05 m/s: 40 steps): free fall
    n = 30
    lmp.step(n)
    rb = lmp.rigid_bodies()
    t, eps = n * dt, np.finfo(float).eps
    ex_x = x0 + v0 * t + 0.5 * G * t * t
    ex_v = v0 + G * t
    print("free fall: |dx| / |x| %.3e  |dv| / |v| %.3e  (n eps %.3e)" % (
        np.max(np.abs(rb["xcm"][0] - ex_x)) / np.max(np.abs(ex_x)), np.max(np.abs(rb["vcm"][0] - ex_v)) / np.max(np.abs(ex_v)), n * eps))
    assert np.max(np.abs(rb["xcm"][0] - ex_x)) <= n * eps * np.max(np.abs(ex_x))
    assert np.max(np.abs(rb["vcm"][0] - ex_v)) <= n * eps * np.max(np.abs(ex_v))
    # through the bounce
    worst = (0.0, 0.0)
    for _ in range(6):
        lmp.step(250)
        e = _rigid_invariants(lmp.get_state(), lmp.rigid_bodies()["omega"][0], pairs, dist0)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    rb = lmp.rigid_bodies()
    print("after the bounce: vcm_y %.4g, pair distances %.3e relative, v_i - v_j against omega x (x_i - x_j) %.3e" % (
        rb["vcm"][0, 1], worst[0], worst[1]))
    assert rb["vcm"][0, 1] > 0.0   # it came back up
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


def _periodic_case():
    case = rc.clumps(2, seed=41)
    case["boxlo"], case["boxhi"], case["periodic"] = np.array([0.0, -2.0, 0.0]), np.array([4.0, 4.0, 4.0]), (1, 0, 1)
    case["x"][:, 0] += 4.0 - 0.05 - case["x"][:, 0].max()   # (the second clump ends 0.05 short of the +x face)
    case["v"][:] = [5.0, 0.0, 0.3]
    return case


def test_a_body_crossing_a_periodic_face_stays_rigid_and_inside_the_box():
    case = _periodic_case()
    lmp = _engine(case)
    lmp.set_molecule(case["tag"], case["mol"])
    lmp.command("fix 1 all rigid/nve molecule")
    _forces_on(lmp, case, g=0.0)
    st0 = lmp.get_state()
    same = np.array([(i, j) for i in range(case["n"]) for j in range(i) if case["mol"][i] == case["mol"][j]])
    prd = case["boxhi"] - case["boxlo"]

    def dists(x):
        d = x[same[:, 0]] - x[same[:, 1]]
        d -= np.where(np.array(case["periodic"], bool), prd * np.rint(d / prd), 0.0)
        return np.linalg.norm(d, axis=1)

    d0 = dists(st0["x"])
    crossed = False
    for _ in range(10):
        lmp.step(100)
        x = lmp.get_state()["x"]
        assert np.all(x[:, 0] >= case["boxlo"][0]) and np.all(x[:, 0] < case["boxhi"][0])
        assert np.all(x[:, 2] >= case["boxlo"][2]) and np.all(x[:, 2] < case["boxhi"][2])
        assert np.max(np.abs(dists(x) - d0) / d0) <= 1e-12
        crossed = crossed or bool(np.any(x[:, 0] < 1.0))
    assert crossed


def _dyadic_rows(shift):
    """_two_bodies with every length a multiple of 2^-10, so that a shift by half the box and the wrap back are exact:
    r = 1/16, 5/32 between the centres of a row, the lead spheres overlap by r / 64"""
    r = 0.0625
    half = r - r / 128.0
    xs = np.array([-half - 0.15625 * k for k in range(4)] + [half + 0.15625 * k for k in range(4)]) + 2.0 + shift
    case = _two_bodies()
    case["x"][:, 0] = np.where(xs >= 4.0, xs - 4.0, xs)
    case["diameter"][:] = 2 * r
    return case


def test_two_bodies_in_contact_across_a_periodic_face():
    """the pair of test_a_body_atom_collides_with_the_mass_of_its_body moved so that the contact lies on the periodic +x
    face: the partner is an image, whose body mass is gathered through its root.  Every coordinate is dyadic, so the
    minimum image is exact and the forces must be those of the same pair in the middle of the box: 1e-14 leaves room for
    the one rounding of x_i - x_j + L against x_i - x_j."""
    pair = "gran/hooke/history 2.0e5 NULL 500.0 NULL 0.5 1"
    out = []
    for shift, per in ((0.0, (0, 0, 0)), (2.0, (1, 0, 0))):
        case = _dyadic_rows(shift)
        case["periodic"] = per
        lmp = _engine(case, dt=1e-6, skin=0.01, pair=pair)
        lmp.set_molecule(case["tag"], case["mol"])
        lmp.command("fix 1 all rigid/nve molecule")
        lmp.setup()
        out.append((lmp.get_state()["f"].copy(), lmp.rigid_bodies()["fcm"].copy()))
        if per[0]:
            x0 = lmp.get_state()["x"]
            assert x0[:4, 0].min() > 3.0 and x0[4:, 0].max() < 1.0   # (the two rows sit on either side of the face)
            lmp.step(50)
            x = lmp.get_state()["x"]
            assert np.all(x[:, 0] >= 0.0) and np.all(x[:, 0] < 4.0)
            d = x[:, None, :] - x[None, :, :]
            d[..., 0] -= 4.0 * np.rint(d[..., 0] / 4.0)
            dist = np.linalg.norm(d, axis=2)
            d0 = x0[:, None, :] - x0[None, :, :]
            d0[..., 0] -= 4.0 * np.rint(d0[..., 0] / 4.0)
            dist0 = np.linalg.norm(d0, axis=2)
            for blk in (slice(0, 4), slice(4, 8)):
                assert np.max(np.abs(dist[blk, blk] - dist0[blk, blk])) <= 1e-12 * np.max(dist0[blk, blk])
    (f0, fcm0), (f1, fcm1) = out
    print("contact force in the box %.17g, across the face %.17g" % (f0[0, 0], f1[0, 0]))
    assert abs(f0[0, 0]) > 0.0
    assert dc.rel_err(f1, f0) <= 1e-14 and dc.rel_err(fcm1, fcm0) <= 1e-14


def _query_run(query):
    case = rc.clumps(6, seed=91)
    lmp = _engine(case)
    lmp.set_molecule(case["tag"], case["mol"])
    lmp.command("fix 1 all rigid/nve molecule")
    _forces_on(lmp, case)
    lmp.step(20)
    lmp.command("velocity all set 0.1 -0.2 0.3 units box")
    rb = lmp.rigid_bodies() if query else None
    lmp.step(20)
    return lmp, rb


def test_asking_for_the_bodies_between_velocity_set_and_a_step_changes_nothing():
    """rigid_bodies() derives the bodies again after `velocity set`; they must carry the forces of the last evaluation, as
    the bodies a step derives do: the same bits with and without the question, and the question shows those forces"""
    (a, _), (b, rb) = _query_run(False), _query_run(True)
    case = rc.clumps(6, seed=91)
    f = case["fext"] + rc.mass_of(case)[:, None] * G
    fcm = np.array([f[case["mol"] == k + 1].sum(axis=0) for k in range(6)])
    assert np.max(np.abs(rb["fcm"] - fcm)) <= 1e-13 * np.max(np.abs(fcm))   # (sums of at most 8 terms)
    assert np.allclose(rb["vcm"], [0.1, -0.2, 0.3], rtol=1e-14) and np.any(rb["torque"] != 0.0)
    assert _bits(a) == _bits(b)


def _data_file(path, case, molecules=True, nmol=None):
    with open(path, "w") as f:
        f.write("bodies of spheres\n\n%d atoms\n1 atom types\n\n" % case["n"])
        for k, c in enumerate("xyz"):
            f.write("%.17g %.17g %slo %shi\n" % (case["boxlo"][k], case["boxhi"][k], c, c))
        f.write("\nAtoms\n\n")
        for i in range(case["n"]):
            f.write("%d 1 %.17g %.17g %.17g %.17g %.17g\n" % ((case["tag"][i], case["diameter"][i], case["density"][i]) + tuple(case["x"][i])))
        f.write("\nVelocities\n\n")
        for i in range(case["n"]):
            f.write("%d 0 0 0 0 0 0\n" % case["tag"][i])
        if molecules:
            f.write("\nMolecules\n\n")
            for i in range(case["n"] if nmol is None else nmol):
                f.write("%d %d\n" % (case["tag"][i], case["mol"][i]))


def test_read_data_with_a_molecules_section(tmp_path):
    """`read_data FILE fix ID NULL Molecules` after `fix ID all property/atom mol` (the form of cases/example-cases/irregular):
    the bodies of `rigid/nve molecule` are the molecules of the file; the two refusals of that line"""
    case = rc.clumps(5, seed=95)
    head = ("atom_style sphere", "boundary f f f", "newton off", "communicate single vel yes")
    good, short = str(tmp_path / "good.in"), str(tmp_path / "short.in")
    _data_file(good, case)
    _data_file(short, case, nmol=case["n"] - 1)
    lmp = Lammps()
    for line in head + ("fix molprop all property/atom mol", "read_data %s fix molprop NULL Molecules" % good, "neighbor 0.05 bin",
                        "pair_style gran/hooke/history 2.0e5 NULL 50.0 NULL 0.5 0", "pair_coeff * *", "timestep 1e-4",
                        "fix 1 all rigid/nve molecule", "fix grav all gravity 9.81 vector 0 -1 0"):
        lmp.command(line)
    lmp.step(10)
    rb = lmp.rigid_bodies()
    assert rb["natoms"].tolist() == np.bincount(case["mol"])[1:].tolist()
    m = rc.mass_of(case)
    assert np.allclose(rb["masstotal"], [m[case["mol"] == k + 1].sum() for k in range(5)], rtol=1e-14)
    lmp = Lammps()
    for line in head:
        lmp.command(line)
    with pytest.raises(SfError, match="Fix ID for read_data does not exist"):
        lmp.command("read_data %s fix molprop NULL Molecules" % good)
    lmp.command("fix molprop all property/atom mol")
    with pytest.raises(SfError, match="does not list every atom"):
        lmp.command("read_data %s fix molprop NULL Molecules" % short)


def test_a_decomposed_domain_refuses_the_fix():
    case = rc.clumps(3, seed=81)
    lmp = _engine(case)
    assert lmp.L.sf_dem_set_subdomain(lmp.ptr, 0, 1, float(case["boxlo"][0]), float(case["boxhi"][0])) == 0
    with pytest.raises(SfError, match="no decomposed domain"):
        lmp.command("fix 1 all rigid/nve single")


def _bits(lmp):
    st, rb = lmp.get_state(), lmp.rigid_bodies()
    return [st[k].tobytes() for k in ("x", "v", "omega", "f")] + [rb[k].tobytes() for k in ("xcm", "vcm", "quat", "angmom")]


def _clump_run(order=None, steps=(300,)):
    case = rc.clumps(60, seed=51, nfree=5)
    lmp = _engine(case, order=order)
    lmp.set_molecule(case["tag"], case["mol"])
    lmp.command("group clump type 1")
    lmp.command("group free type 2")
    lmp.command("fix 1 clump rigid/nve molecule")
    lmp.command("fix 2 free nve/sphere")
    _forces_on(lmp, case)
    for s in steps:
        lmp.step(s)
    return lmp


def test_a_run_in_two_pieces_gives_the_same_bits():
    assert _bits(_clump_run(steps=(300,))) == _bits(_clump_run(steps=(100, 200)))


def test_the_same_bits_run_to_run_and_for_atoms_fed_in_reverse():
    a = _bits(_clump_run())
    assert a == _bits(_clump_run())
    assert a == _bits(_clump_run(order=np.arange(rc.clumps(60, seed=51, nfree=5)["n"])[::-1]))


def test_dump_custom_after_a_rigid_run_shows_the_state(tmp_path):
    case = rc.clumps(20, seed=61)
    lmp = _engine(case)
    lmp.set_molecule(case["tag"], case["mol"])
    lmp.command("fix 1 all rigid/nve molecule")
    _forces_on(lmp, case)
    lmp.command("dump d all custom 50 %s id x y z vx vy vz omegax omegay omegaz" % (tmp_path / "r.dump"))
    lmp.command("dump_modify d sort id")
    lmp.step(100)
    lmp.sync()
    lines = open(tmp_path / "r.dump").read().splitlines()
    start = max(i for i, l in enumerate(lines) if l.startswith("ITEM: ATOMS"))
    rows = np.array([[float(t) for t in l.split()] for l in lines[start + 1:start + 1 + case["n"]]])
    st = lmp.get_state()
    assert rows[:, 0].astype(int).tolist() == st["tag"].tolist()
    # (the dump prints %g: six significant digits)
    for cols, key in ((slice(1, 4), "x"), (slice(4, 7), "v"), (slice(7, 10), "omega")):
        assert np.allclose(rows[:, cols], st[key], rtol=2e-5, atol=1e-5 * np.max(np.abs(st[key])))


def test_restart_then_the_fix_line_again_keeps_the_body_rigid(tmp_path):
    case = rc.clumps(1, seed=71, nmin=8, nmax=8)
    lmp = _engine(case)
    lmp.command("fix 1 all rigid/nve single")
    _forces_on(lmp, case)
    lmp.step(200)
    F = str(tmp_path / "rigid.sfr")
    lmp.write_restart(F)
    new = Lammps()
    new.read_restart(F)
    for line in ("newton off", "neighbor 0.05 bin", "pair_style gran/hooke/history 2.0e5 NULL 50.0 NULL 0.5 0", "pair_coeff * *",
                 "fix 1 all rigid/nve single"):
        new.command(line)
    _forces_on(new, case)
    # the bodies are derived again from the atoms: the same body up to the rounding of the atoms' positions
    a, b = lmp.rigid_bodies(), new.rigid_bodies()
    assert np.allclose(a["xcm"], b["xcm"], rtol=1e-13) and np.allclose(a["vcm"], b["vcm"], rtol=1e-11, atol=1e-13)
    assert np.allclose(np.sort(a["inertia"]), np.sort(b["inertia"]), rtol=1e-11)
    st0 = new.get_state()
    pairs = np.array([(i, j) for i in range(8) for j in range(i)])
    d0 = np.linalg.norm(st0["x"][pairs[:, 0]] - st0["x"][pairs[:, 1]], axis=1)
    new.step(300)
    e_d, e_v = _rigid_invariants(new.get_state(), new.rigid_bodies()["omega"][0], pairs, d0)
    assert e_d <= 1e-12 and e_v <= 1e-12
    assert new.info().nsteps == 500


def test_refusals(tmp_path):
    case = rc.clumps(3, seed=81)

    def fresh(**kw):
        return _engine(case, **kw)

    for line, msg in (("fix 1 all rigid/nve custom", "bodystyle custom is not supported"),
                      ("fix 1 all rigid/nve single langevin 1.0 1.0 1.0 428984", "keyword langevin is not supported"),
                      ("fix 1 all rigid/nve single force 1 off off off", "keyword force is not supported"),
                      ("fix 1 all rigid/nve single torque 1 off off off", "keyword torque is not supported"),
                      ("fix 1 all rigid/nve single infile bodies.txt", "keyword infile is not supported"),
                      ("fix 1 all rigid/nve molecule", "no molecule IDs"),
                      ("fix 1 all rigid/small molecule", "Unknown fix style"),
                      ("fix 1 all rigid single", "Unknown fix style")):
        with pytest.raises(SfError, match=msg):
            fresh().command(line)
    lmp = fresh()
    lmp.command("fix 1 all rigid/nve single")
    with pytest.raises(SfError, match="More than one fix rigid/nve"):
        lmp.command("fix 2 all rigid/nve single")
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.create_particle(np.array([[1.0, 1.0, 1.0]]), [1000.0], 0.1, 2500.0, 1, np.zeros(3))
    with pytest.raises(SfError, match="not while fix rigid/nve exists"):
        lmp.delete_particle([1])
    lmp = fresh()
    lmp.command("fix 1 all nve/sphere")
    lmp.command("fix 2 all rigid/nve single")
    with pytest.raises(SfError, match="also in the group of fix nve/sphere"):
        lmp.setup()
    wide = dict(case)
    wide["periodic"] = (1, 0, 0)
    lmp = _engine(wide)
    lmp.command("fix 1 all rigid/nve single")   # three clumps two apart in a box of four: wider than half of it
    with pytest.raises(SfError, match="wider than half the periodic box"):
        lmp.setup()
    # thermo lines that count degrees of freedom, while a log is open
    lmp = fresh(args=["-log", str(tmp_path / "log.lammps"), "-screen", "none"])
    lmp.command("fix 1 all rigid/nve single")
    lmp.command("thermo 10")
    with pytest.raises(SfError, match="degrees of freedom of the rigid bodies"):
        lmp.step(10)
    lmp.command("thermo_style custom step atoms fmax")
    lmp.step(10)
    # more than one rank
    L = Lammps().L
    h = C.c_void_p()
    assert L.sf_lammps_open_world(0, None, 0, 0, 2, b"x" * 128, C.byref(h)) == 0
    try:
        err = L.sf_lammps_command(h, b"fix 1 all rigid/nve single")
        assert err is not None and b"one rank" in err
    finally:
        L.sf_lammps_close(h)
