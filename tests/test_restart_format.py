"""The checkpoint file format, version 1, through sedifoam_amd/restart.py alone (numpy, no library, no GPU): round trips,
every refusal DESIGN.md section 10 names, and a file the engine wrote on an MI355X that pins the version for good."""
import os

import numpy as np
import pytest

from sedifoam_amd import restart

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _state(n=40, seed=1):
    rng = np.random.default_rng(seed)
    tag = np.sort(rng.choice(np.arange(1, 4 * n), n, replace=False)).astype(np.int32)
    count = np.zeros(n, np.int32)
    partner = []
    for i in range(n - 1):
        higher = tag[i + 1:]
        k = int(rng.integers(0, min(4, len(higher)) + 1))
        count[i] = k
        partner += sorted(rng.choice(higher, k, replace=False).tolist())
    nc = len(partner)
    v3 = lambda: rng.normal(size=(n, 3))
    walls = []
    for wid, m in (("ywall", 7), ("w1", 0), ("a_longer_fix_id", 3)):
        walls.append(dict(id=wid, tag=np.sort(rng.choice(tag, m, replace=False)).astype(np.int32), shear=rng.normal(size=(m, 3))))
    return dict(step=123456, max_tag=int(tag.max()) + 5, dt=2.5e-7, boxlo=np.array([0.0, -1.0, 0.5]),
                boxhi=np.array([1.0, 2.0, 3.5]), periodic=(1, 0, 1), units="si",
                groups=[("all", 1), ("bottom", 2), ("active", 4)], tag=tag,
                type=rng.integers(1, 3, n).astype(np.int32), mask=rng.integers(1, 8, n).astype(np.int32),
                foamCpuId=rng.integers(0, 16, n).astype(np.int32), x=v3(), radius=rng.random(n), v=v3(), rmass=rng.random(n),
                omega=v3(), fdrag=v3(), DuDt=v3(), vOld=v3(), contact_count=count,
                contact_partner=np.array(partner, np.int32), contact_shear=rng.normal(size=(nc, 3)), walls=walls)


def _same(a, b):
    for k in ("step", "max_tag", "dt", "units", "groups"):
        assert a[k] == b[k], k
    assert tuple(a["periodic"]) == tuple(b["periodic"])
    for k in ("boxlo", "boxhi", "tag", "type", "mask", "foamCpuId", "x", "radius", "v", "rmass", "omega", "fdrag", "DuDt",
              "vOld", "contact_count", "contact_partner", "contact_shear"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype or k in ("boxlo", "boxhi"), k
    assert [w["id"] for w in a["walls"]] == [w["id"] for w in b["walls"]]
    for p, q in zip(a["walls"], b["walls"]):
        assert np.array_equal(p["tag"], q["tag"]) and np.array_equal(p["shear"], q["shear"])


def test_write_read_write(tmp_path):
    st = _state()
    f, g = str(tmp_path / "f"), str(tmp_path / "g")
    restart.write(f, st)
    assert not os.path.exists(f + ".tmp")
    back = restart.read(f)
    _same(st, back)
    restart.write(g, back)
    assert open(f, "rb").read() == open(g, "rb").read()
    h = restart.header(f)
    assert h["natoms"] == 40 and h["ncontacts"] == len(st["contact_partner"]) and h["step"] == 123456
    assert h["walls"] == [("ywall", 7), ("w1", 0), ("a_longer_fix_id", 3)] and h["file_bytes"] == os.path.getsize(f)
    empty = restart.without_history(st)
    restart.write(g, empty)
    e = restart.read(g)
    assert e["contact_count"].sum() == 0 and all(len(w["tag"]) == 0 for w in e["walls"])
    assert np.array_equal(e["x"], st["x"])


def test_bytes_depend_on_the_state_only():
    a, b = _state(seed=4), _state(seed=4)
    b["x"] = np.asfortranarray(b["x"])                 # memory layout and integer width of the arrays do not matter
    b["tag"] = b["tag"].astype(np.int64)
    assert restart.to_bytes(a) == restart.to_bytes(b)
    b["v"][3, 1] = np.nextafter(b["v"][3, 1], 1.0)     # one bit of the state does
    assert restart.to_bytes(a) != restart.to_bytes(b)


def test_refusals(tmp_path):
    data = restart.to_bytes(_state())
    h = restart.from_bytes(data) and restart._parse_header(data, "f")[0]
    cuts = [0, 10, 100, h["header_bytes"] - 1]
    for name, off, nb in h["sections"]:
        cuts += [off, off + nb // 2] if nb else [off]
    cuts.append(len(data) - 1)
    for c in sorted(set(cuts)):
        with pytest.raises(restart.RestartError, match="is truncated"):
            restart.from_bytes(data[:c], "f")
    flips = [20, 70, restart.FIXED_BYTES + 3, h["header_bytes"] - 20]   # fixed part, group table, section table
    flips += [off + nb // 2 for name, off, nb in h["sections"] if nb]
    for pos in flips:
        bad = bytearray(data)
        bad[pos] ^= 0x04
        with pytest.raises(restart.RestartError, match="is corrupted"):
            restart.from_bytes(bytes(bad), "f")
    with pytest.raises(restart.RestartError, match="is corrupted"):
        restart.from_bytes(data + b"\0" * 8, "f")
    with pytest.raises(restart.RestartError, match="not a sedifoam_amd restart file"):
        restart.from_bytes(b"LAMMPS  " + data[8:], "f")
    newer = bytearray(data)
    newer[8] = 2
    with pytest.raises(restart.RestartError, match="format version 2, this code reads up to version 1"):
        restart.from_bytes(bytes(newer), "f")
    swapped = bytearray(data)
    swapped[12:16] = swapped[12:16][::-1]
    with pytest.raises(restart.RestartError, match="other byte order"):
        restart.from_bytes(bytes(swapped), "f")
    unsorted = _state()
    unsorted["tag"] = unsorted["tag"][::-1].copy()
    with pytest.raises(restart.RestartError, match="ascending tag order"):
        restart.to_bytes(unsorted)
    p = str(tmp_path / "cut")
    open(p, "wb").write(data[:200])
    with pytest.raises(restart.RestartError, match="Restart file %s is truncated" % p):
        restart.read(p)


def test_golden_file_written_by_the_engine():
    """tests/golden/restart_v1_small.sfr: 500 grains in a closed box with a sliding floor after 120 sub-steps, written by
    `write_restart` on an MI355X; the .npz holds what get_state(), history() and wall_shear() returned at that moment."""
    path = os.path.join(GOLDEN, "restart_v1_small.sfr")
    st = restart.read(path)
    ref = np.load(os.path.join(GOLDEN, "restart_v1_small.npz"))
    assert st["version"] == 1 and st["step"] == int(ref["step"]) == 120 and st["dt"] == float(ref["dt"])
    assert st["groups"] == [("all", 1), ("lower", 2)] and (st["mask"] == 3).all()
    assert np.array_equal(st["boxlo"], ref["boxlo"]) and np.array_equal(st["boxhi"], ref["boxhi"])
    assert np.array_equal(st["tag"], ref["tag"]) and len(st["tag"]) == 500
    for k in ("x", "v", "omega"):
        assert np.array_equal(st[k], ref[k]), k
    saved = restart.contacts(st)
    assert len(saved) == len(ref["pair"]) >= 100
    for (a, b), s in zip(ref["pair"], ref["shear"]):
        assert np.array_equal(saved[(int(a), int(b))], s)
    assert [w["id"] for w in st["walls"]] == ["w0", "w1", "w2"]
    for w in range(3):
        assert np.array_equal(restart.wall_rows(st, w), ref["wall%d" % w])
    assert restart.to_bytes(st) == open(path, "rb").read()


def test_reading_checks_the_order_writing_checks():
    """what to_bytes refuses to write, from_bytes refuses to read (the engine's reader makes the same checks)"""
    st = _state()
    i = int(np.nonzero(st["contact_count"] >= 2)[0][0])
    e = int(st["contact_count"][:i].sum())
    for change in ("swap", "own", "wall"):
        bad = dict(st)
        if change == "wall":
            bad["walls"] = [dict(w, tag=w["tag"][::-1].copy()) for w in st["walls"]]
        else:
            cp = st["contact_partner"].copy()
            if change == "swap":
                cp[e], cp[e + 1] = cp[e + 1], cp[e]
            else:
                cp[e] = st["tag"][i]
            bad["contact_partner"] = cp
        with pytest.raises(restart.RestartError):
            restart.to_bytes(bad)
        with pytest.raises(restart.RestartError, match="is corrupted"):
            restart.from_bytes(restart.to_bytes(bad, check=False), "f")
