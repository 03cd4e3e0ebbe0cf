"""Every neighbour-list build of the engine against a brute-force pair set (tests/neigh_model.py): the list read back word
by word (Lammps.neighbors) must be the model's set of (tag_i, tag_j, image) exactly -- after setup() on random clouds in every
list-build form the engine has, on lattices whose pairs sit exactly at the cutoff, and after every leg of runs that rebuild.
The comparison is set equality, no tolerance: every input is chosen (on the CPU, tests/test_neigh_model.py) so that no
candidate pair lies within rounding of its cutoff."""
import numpy as np
import pytest

from tests import dem_cases as dc
from tests import neigh_cases as nc
from tests import neigh_model as nm

pytestmark = pytest.mark.gpu

# every form of the list build: the knobs are read in the constructor, so each variant makes fresh engines
VARIANTS = {
    "default": {},
    "ghost_atoms": {"SF_GHOST_FREE": "0"},
    "sub1": {"SF_SUB": "1"},
    "sub2": {"SF_SUB": "2"},
    "quad0": {"SF_BUILD_QUAD": "0"},
    "quad2": {"SF_BUILD_QUAD": "2"},
    "quad4": {"SF_BUILD_QUAD": "4"},
    "quad8": {"SF_BUILD_QUAD": "8"},
    "park_in_memory": {"SF_BUILD_LDS": "0"},
    "staged_history": {"SF_HIST_IN_PLACE": "0"},
    "staged_history_park_in_memory": {"SF_HIST_IN_PLACE": "0", "SF_BUILD_LDS": "0"},
    "park_margin_negative": {"SF_PARK_MARGIN": "-6"},
    "touch_first0": {"SF_TOUCH_FIRST": "0"},
    "touch_first1": {"SF_TOUCH_FIRST": "1"},
    "tile8_sub2": {"SF_TILE": "8", "SF_SUB": "2"},
    "lds_tile4_sub1": {"SF_LDS": "1", "SF_TILE": "4", "SF_SUB": "1"},     # index-mode words
    "rank_permute0": {"SF_RANK_PERMUTE": "0"},
    "scan_min1": {"SF_SCAN_MIN": "1"},
    "rocprim_scan": {"SF_ROCPRIM_SCAN": "1"},
    "hist_copies1": {"SF_HIST_COPIES": "1"},
    "hist_copies2": {"SF_HIST_COPIES": "2"},
}
COPIES = {"hist_copies1": 1, "hist_copies2": 2}
# What a setup() cannot reach: the first list has no old list behind it, so the history re-injection (read in place or staged),
# the touching-first placement, the parking rows sized from the previous list (SF_PARK_MARGIN < 0: too few, F_PARK_OVER and a
# second attempt) and the sort-cell choice only act from the second list on.  These variants therefore also run the hot beds.
RUN_VARIANTS = ["default", "ghost_atoms", "sub1", "sub2", "quad0", "quad8", "park_in_memory", "staged_history",
                "staged_history_park_in_memory", "park_margin_negative", "touch_first0", "touch_first1", "hist_copies1",
                "hist_copies2"]


def _check_list(lmp, model, copies=None, what=""):
    """(b) the words are the model's set, without duplicates; (c) their count and the longest row are what info() says;
    (d) the touching words are the pairs history() reports; (e) who stores a touching pair's history: one side of a
    pair of two owned atoms, both sides of a pair with an image"""
    rows, flags = lmp.neighbors()
    got = nm.as_set(rows)
    missing, extra = model - got, got - model
    print("%s: %d words, model %d, missing %d, extra %d" % (what, len(rows), len(model), len(missing), len(extra)))
    assert not missing and not extra, (what, sorted(missing)[:5], sorted(extra)[:5])
    assert len(got) == len(rows), what + ": duplicate words"
    info = lmp.info()
    assert len(rows) == info.npairs_full
    assert nm.longest_row(rows) == info.max_neigh_used
    touch = (flags & 1) != 0
    own = (flags & 2) != 0
    pairs = {(min(i, j), max(i, j)) for i, j in rows[touch][:, :2].tolist()}
    assert pairs == set(lmp.history()), what
    img = np.any(rows[:, 2:] != 0, axis=1)
    assert own[touch & img].all(), what + ": a pair with an image keeps a history copy on each side"
    sides = {}
    for (i, j), o in zip(rows[touch & ~img][:, :2].tolist(), own[touch & ~img].tolist()):
        s = sides.setdefault((min(i, j), max(i, j)), [0, 0])
        s[0] += 1
        s[1] += int(o)
    assert all(s[0] == 2 for s in sides.values()), what + ": a pair touches from both sides or from neither"
    # One copy per contact (the lower index stores it) or one per side: the same choice for the whole list.  The partner
    # side finds the owner's copy through a five-bit slot number, so a pair of which either atom has more than 32
    # neighbours may keep a copy on each side whatever the choice (k_back_slots)
    rowlen = np.bincount(rows[:, 0])
    short = {s[1] for (i, j), s in sides.items() if rowlen[i] <= 32 and rowlen[j] <= 32}
    assert len(short) <= 1 and short <= {1, 2}, (what, short)
    if copies and short:
        assert short == {copies}, (what, short)
    assert all(min(short, default=1) <= s[1] <= 2 for s in sides.values()), what
    return rows, flags


def _build_positions_by_tag(lmp):
    x, tag = lmp.build_positions()
    o = np.argsort(tag, kind="stable")
    return x[o], tag[o]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_random_clouds_list_is_the_brute_force_set(variant, monkeypatch):
    """Uniform random clouds (tests/neigh_cases.py: a periodic box that takes the ghost-free build, one of exactly three
    cutoffs, a thin x-z periodic one with ghost atoms, a closed one, diameters 1/3 .. 1 mm alone / with fix cohesive / with
    lubricate/poly, and a dense one with rows beyond 128) after setup(), in one form of the list build."""
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    for name, extra, cut_abs in nc.CLOUD_RUNS:
        bed = nc.cloud(name)
        model, band, _ = nc.cloud_model(name, cut_abs)
        assert band == 0
        lmp = dc.make_hip(bed, nc.cloud_cfg(name, extra))
        lmp.setup()
        what = "%s %s %s" % (variant, name, "+".join(extra) or "granular")
        xb, tagb = _build_positions_by_tag(lmp)
        st = lmp.get_state()
        assert np.array_equal(tagb, st["tag"]) and np.array_equal(xb, st["x"]), what      # (a)
        assert np.array_equal(xb, bed["x"]), what                                          # nothing to wrap
        rows, _ = _check_list(lmp, model, COPIES.get(variant), what)
        if name == "closed_4p5":
            assert lmp.info().nghost == 0
        if name == "poly_ratio3" and not extra:
            # small-small pairs inside the cell stencil but beyond ri + rj + skin are absent: the list is shorter than
            # the absolute-cutoff one of the same cloud
            assert len(rows) < len(nc.cloud_model(name, nc.CUT)[0])
        del lmp


@pytest.mark.parametrize("ghost_free", ["0", "1"])
@pytest.mark.parametrize("sub", ["1", "2"])
def test_pairs_exactly_at_the_cutoff_and_atoms_on_the_faces(sub, ghost_free, monkeypatch):
    """Lengths that are integer multiples of 2^-14 m: rsq and cut^2 are exact on both sides, so pairs AT the cutoff must be
    listed (rsq <= cutsq) and the pair one unit beyond must not, with every atom of the lattice on a cell corner, the box an
    exact multiple of the cutoff, atoms at exactly lo / hi of periodic and of walled dimensions, lo at and off the origin."""
    monkeypatch.setenv("SF_SUB", sub)
    monkeypatch.setenv("SF_GHOST_FREE", ghost_free)
    for box in nc.EX_BOXES:
        for lo_name in nc.EX_LO:
            for lattice_only, size in ((True, "cut20"), (True, "cut49"), (False, "cut20")):
                bed = nc.exact_case(box, lo_name, lattice_only, size)
                model, _, mrows = nc.exact_model(box, lo_name, lattice_only, size)
                lmp = dc.make_hip(bed, nc.exact_cfg(bed))
                lmp.setup()
                what = "sub%s ghost_free%s %s %s %s%s" % (sub, ghost_free, box, lo_name, size, " lattice" * lattice_only)
                xb, tagb = _build_positions_by_tag(lmp)
                assert np.array_equal(xb, bed["xw"]), what + ": the wrap takes hi to lo exactly, a wall's hi stays"
                assert np.array_equal(xb, lmp.get_state()["x"]), what
                rows, _ = _check_list(lmp, model, None, what)
                if lattice_only:
                    assert len(rows) == nc.exact_lattice_rows(box), what
                    if box == "ppp":
                        assert (np.bincount(rows[:, 0])[1:] == 6).all(), what
                else:
                    got = {(i, j) for i, j in rows[:, :2].tolist()}
                    assert all(p in got and p[::-1] in got for p in bed["pairs_at_cutoff"]), what
                    assert not any(p in got or p[::-1] in got for p in bed["pairs_beyond"]), what
                del lmp


@pytest.mark.parametrize("variant", RUN_VARIANTS)
@pytest.mark.parametrize("name", ["loose_periodic", "closed", "poly_cohesive_lubricate"])
def test_lists_built_inside_a_run(name, variant, monkeypatch):
    """The lists a run rebuilds carry the history re-injection, the touching-first placement and the sort-cell switch of the
    second list: after every leg the list is the model's set at the positions it was built from, no atom is beyond
    skin / 2 of them, every touching pair is listed, and the rebuild count is the oracle's."""
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    bed, cfg, leg = nc.hot_bed(name)
    radius = 0.5 * np.asarray(bed["diameter"])
    cut_abs = nc.hot_cut_abs(bed, cfg)
    lmp = dc.make_hip(bed, cfg)
    orc = dc.make_oracle(bed, cfg)
    lmp.setup()
    orc.setup()
    legs = 0
    while lmp.info().nbuilds < 4 or legs < 3:     # (a hot bed reaches four lists within one leg: three legs at least)
        assert legs < 12, "the bed does not rebuild"
        lmp.step(leg)
        orc.run(leg)
        legs += 1
        what = "%s %s leg %d (%d builds)" % (variant, name, legs, lmp.info().nbuilds)
        assert lmp.info().nbuilds == orc.nbuilds, what
        xb, tagb = _build_positions_by_tag(lmp)
        r = radius[tagb - 1]
        rows, band = nm.neighbor_rows(xb, r, bed["boxlo"], bed["boxhi"], bed["periodic"], cfg["skin"], cut_abs, tag=tagb)
        assert band == 0, what + ": a pair within rounding of the cutoff, change the leg length"
        got, _ = _check_list(lmp, nm.as_set(rows), COPIES.get(variant), what)
        st = lmp.get_state()
        assert np.array_equal(st["tag"], tagb)
        moved = nm.min_image_sq(st["x"] - xb, bed["boxlo"], bed["boxhi"], bed["periodic"])
        print("%s: max displacement^2 / (skin/2)^2 = %.6f" % (what, moved.max() / (0.5 * cfg["skin"]) ** 2))
        assert moved.max() <= (0.5 * cfg["skin"]) ** 2, what
        # (the engine leaves an atom that left the box where it is until the next rebuild: images as at the build)
        touching, _ = nm.neighbor_rows(st["x"], r, bed["boxlo"], bed["boxhi"], bed["periodic"], 0.0, tag=tagb, touching=True)
        assert len(touching) > 0 and nm.as_set(touching) <= nm.as_set(got), what
    assert lmp.info().nbuilds >= 4


def test_reading_the_list_changes_nothing():
    """neighbors() and build_positions() are passive: an engine that is read between the legs of a run that rebuilds ends
    in the same bits -- state, forces and history -- as one that is not."""
    bed, cfg, leg = nc.hot_bed("loose_periodic")
    outs = []
    for look in (True, False):
        lmp = dc.make_hip(bed, cfg)
        lmp.setup()
        for _ in range(3):
            if look:
                lmp.neighbors()
                lmp.build_positions()
            lmp.step(leg)
        if look:
            lmp.neighbors()
            lmp.build_positions()
        st = lmp.get_state()
        st["hist"] = lmp.history()
        st["nbuilds"] = lmp.info().nbuilds
        outs.append(st)
    a, b = outs
    assert a["nbuilds"] == b["nbuilds"] >= 2
    for k in ("x", "v", "omega", "f", "torque"):
        assert np.array_equal(a[k], b[k]), k
    assert set(a["hist"]) == set(b["hist"]) and len(a["hist"]) > 0
    assert all(np.array_equal(a["hist"][k], b["hist"][k]) for k in a["hist"])


def test_a_decomposed_domain_is_refused():
    from sedifoam_amd._lib import SfError
    bed = nc.cloud("closed_4p5")
    lmp = dc.make_hip(bed, nc.cloud_cfg("closed_4p5", {}))
    lo, hi = float(bed["boxlo"][0]), float(bed["boxhi"][0])
    assert lmp.L.sf_dem_set_subdomain(lmp.ptr, 0, 2, lo, 0.5 * (lo + hi)) == 0
    for call in (lmp.neighbors, lmp.build_positions):
        with pytest.raises(SfError, match="single domain"):
            call()
