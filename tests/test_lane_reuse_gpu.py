"""Lane reuse in the sub-step kernel (sf_dem_kernels.h, lane_up / sf_lane_reuse_variant): a neighbour's records are taken
from the next lane's registers where that lane holds them, instead of being gathered again.  The change moves data only --
the same records into the same arithmetic in the same order -- so an engine with SF_LANE_REUSE=1 must end in the bits of
one with SF_LANE_REUSE=0, through rebuilds, on every kind of bed and in every kernel of the family: the kernels that do
not take the path (sf_lane_reuse_variant) are one and the same instantiation under both settings."""
import math

import numpy as np
import pytest

from sedifoam_amd import synthetic
from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

BASE = dict(pair="hertz", kn=1.0e7, gamman=0.5, xmu=0.4, g=9.81, dt=1.0e-6)   # the headline script's settings (bench.py, KW)
N = 4000
C5 = dict(cohesive=(1.0e-13, 1.0e-7, 1.0e-7, 1.0e-4, 1), lub=(1.0e-3, 1, 1, 1.001e-3, 1.1e-3, 1, 1))
FLUIDISED = dict(jitter=0.3, spacing=1.1)   # bench.py --bed fluidised


def _walls(bed):
    w = [(1, float(bed["boxlo"][1]), float(bed["boxhi"][1]))]
    for dim in (0, 2):
        if not bed["periodic"][dim]:
            w.append((dim, float(bed["boxlo"][dim]), float(bed["boxhi"][dim])))
    return w


def _packed(closed=False, **kw):
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(N), seed=12345 + 3, vmax=0.8, **kw)
    if closed:   # three wall pairs, the lattice one radius inside
        bed["periodic"] = (0, 0, 0)
        bed["x"][:, 0] += 0.3e-3
        bed["x"][:, 2] += 0.3e-3
        bed["boxhi"][0] += 0.6e-3
        bed["boxhi"][2] += 0.6e-3
    return bed


def _both_arms(bed, cfg, steps, monkeypatch, stat_after_first_step=False):
    """setup + `steps` sub-steps with SF_LANE_REUSE=0 and =1 -> [(state, history, nbuilds, statistic)] of the two engines"""
    outs = []
    for reuse in ("0", "1"):
        monkeypatch.setenv("SF_LANE_REUSE", reuse)
        lmp = dc.make_hip(bed, dict(cfg, walls=_walls(bed)))
        lmp.setup()
        lmp.step(1)
        stat = lmp.lane_reuse_fraction() if stat_after_first_step else None
        lmp.step(steps - 1)
        outs.append((lmp.get_state(), lmp.history(), lmp.info().nbuilds, stat))
        lmp.close()
    return outs


def _assert_same_bits(outs, rebuilds=3):
    (a, ha, na, _), (b, hb, nb, _) = outs
    print("list builds: %d / %d" % (na, nb))
    assert na == nb and na >= 1 + rebuilds          # (the first list + at least three rebuilds)
    for k in ("tag", "x", "v", "omega", "f", "torque"):
        assert np.array_equal(a[k], b[k]), k
    assert ha.keys() == hb.keys() and len(ha) > 0
    for k in ha:
        assert np.array_equal(ha[k], hb[k]), k


@pytest.mark.parametrize("policy", ["1", "0"], ids=["half_wave_gather", "plain_gather"])
def test_packed_periodic_bed_same_bits_and_the_path_is_taken(policy, monkeypatch):
    """Case 1: the packed FCC bed under the headline script, periodic in x and z on a y wall.  Rows of 10 atoms: six row
    ends per wave, lane 63, the periodic wrap in x.  Through the half-wave gather (policy 1, forced onto the small bed) and
    the plain gather (policy 0).  The list statistic after the first sub-step: the CPU emulation of this bed gives 0.31;
    0.15 guards against a test that never takes the path."""
    monkeypatch.setenv("SF_LPA", "1")
    monkeypatch.setenv("SF_NT_POLICY", policy)
    bed = _packed()
    assert bed["n"] == N
    outs = _both_arms(bed, dict(BASE, skin=0.04e-3), 100, monkeypatch, stat_after_first_step=True)
    _assert_same_bits(outs)
    print("lane reuse fraction: %.4f / %.4f" % (outs[0][3], outs[1][3]))
    assert outs[0][3] == outs[1][3] and outs[1][3] >= 0.15


def test_closed_box_partly_filled_last_wave_and_uneven_counts(monkeypatch):
    """Case 2: the same lattice between three wall pairs, N no multiple of 64: the last wave is partly filled (its other
    lanes sit on atom 0), atoms at faces, edges and corners list 3 to 12 neighbours (uneven counts inside a wave, the tail
    slot behind the loop unrolled by two)."""
    monkeypatch.setenv("SF_LPA", "1")
    monkeypatch.setenv("SF_NT_POLICY", "1")
    bed = _packed(closed=True)
    assert bed["n"] % 64 != 0
    _assert_same_bits(_both_arms(bed, dict(BASE, skin=0.04e-3), 100, monkeypatch))


def test_loose_disordered_bed(monkeypatch):
    """Case 3: a loose disordered bed (the kernel that asks for v, omega of touching pairs only): reuse almost never fires,
    and where the roots match the next lane need not hold the v, omega this lane wants.  The statistic need only be finite."""
    monkeypatch.setenv("SF_LPA", "1")
    monkeypatch.setenv("SF_NT_POLICY", "1")
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(N), seed=12345 + 3, vmax=0.5, **FLUIDISED)
    outs = _both_arms(bed, dict(BASE, skin=0.04e-3), 100, monkeypatch, stat_after_first_step=True)
    _assert_same_bits(outs)
    print("lane reuse fraction: %.4f" % outs[1][3])
    assert math.isfinite(outs[1][3]) and outs[0][3] == outs[1][3]


def test_polydisperse_bed_with_cohesion_and_lubrication(monkeypatch):
    """Case 4: a polydisperse bed with hybrid/overlay ... lubricate/poly and fix cohesive: the two-arm kernel, which gathers
    by half waves (it measured neutral with the path and is left out of sf_lane_reuse_variant: whatever that rule says,
    the knob must not change a bit)."""
    monkeypatch.setenv("SF_LPA", "1")
    monkeypatch.setenv("SF_NT_POLICY", "1")
    bed = synthetic.fcc_bed(synthetic.fcc_cells_for(N), seed=15, vmax=0.5, poly=(0.85e-3, 1.0e-3), spacing=0.95)
    _assert_same_bits(_both_arms(bed, dict(BASE, skin=0.03e-3, **C5), 120, monkeypatch))


def test_packed_bed_with_a_frozen_slab(monkeypatch):
    """Case 5: case 1 with `fix freeze` on a slab of atoms: the frozen mark travels in the omega record."""
    monkeypatch.setenv("SF_LPA", "1")
    monkeypatch.setenv("SF_NT_POLICY", "1")
    bed = _packed()
    bed["type"] = np.where(bed["x"][:, 1] < 2.5e-3, 2, 1).astype(np.int32)
    assert 0 < (bed["type"] == 2).sum() < bed["n"] // 2
    bed["v"][bed["type"] == 2] = 0.0
    outs = _both_arms(bed, dict(BASE, skin=0.04e-3, frozen_types=[2]), 100, monkeypatch)
    _assert_same_bits(outs)
    a = outs[1][0]
    bottom = bed["type"][a["tag"] - 1] == 2
    assert np.array_equal(a["x"][bottom], bed["x"][a["tag"] - 1][bottom])      # frozen atoms never move
