"""The checkpoint file of `write_restart` / `restart` / `read_restart`, format version 1: the executable specification
(numpy only; importable without libsedifoam_amd.so).  The engine (csrc/sf_restart.hip) and this module agree byte for
byte: the bytes depend on the state and on nothing else.  DESIGN.md section 10 has the layout as a table.

    read(path) -> dict        write(path, state)        header(path) -> dict

A state is a dict:
    step, max_tag (int)  dt (float)  boxlo, boxhi (3 floats)  periodic (3 ints)  units ("si" | "lj")
    groups   [(name, bit), ...] in ascending bit order ("all" = 1 first)
    tag, type, mask, foamCpuId   int32[n], atoms in ascending tag order
    x, v, omega, fdrag, DuDt, vOld   float64[n, 3];  radius, rmass   float64[n]
    contact_count int32[n] -- touching partners with a HIGHER tag, per atom;  contact_partner int32[nc] -- their tags,
    ascending within an atom;  contact_shear float64[nc, 3] -- the shear history as the lower tag sees it
    walls    [dict(id=fix ID, tag=int32[m] ascending, shear=float64[m, 3]), ...] in the order of the fix lines
"""
import os
import struct
import zlib

import numpy as np

MAGIC = b"SFRESTRT"
VERSION = 1
BOM = 0x01020304
FIXED_BYTES = 152          # the fixed part of the header; its last word is the CRC-32 of the 148 bytes before it
GROUP_BYTES = 64           # name[60] + int32 bit
WALL_BYTES = 64            # fix ID[56] + int64 count
SECTION_BYTES = 48         # name[24] + uint32 dtype + uint32 crc32 + uint64 offset + uint64 nbytes
DTYPE_I32, DTYPE_F64 = 1, 2
_FIXED = "<8sIIQQqqqqd3d3d3iiIII"   # ... then the uint32 CRC of these bytes

_ATOM_SECTIONS = (("tag", DTYPE_I32, 1), ("type", DTYPE_I32, 1), ("mask", DTYPE_I32, 1), ("foamCpuId", DTYPE_I32, 1),
                  ("x", DTYPE_F64, 3), ("radius", DTYPE_F64, 1), ("v", DTYPE_F64, 3), ("rmass", DTYPE_F64, 1),
                  ("omega", DTYPE_F64, 3), ("fdrag", DTYPE_F64, 3), ("DuDt", DTYPE_F64, 3), ("vOld", DTYPE_F64, 3))


class RestartError(Exception):
    pass


def _pad8(n):
    return (n + 7) & ~7


def _name(s, width):
    b = s.encode()
    if len(b) >= width:
        raise RestartError("name %r does not fit %d bytes" % (s, width - 1))
    return b + b"\0" * (width - len(b))


def _columns(a, dtype, rows, n, what):
    """[n] or [n, rows] -> component-major bytes (all x, then all y, then all z)"""
    np_t = "<i4" if dtype == DTYPE_I32 else "<f8"
    a = np.asarray(a)
    if a.size != n * rows:
        raise RestartError("%s: %d values for %d x %d" % (what, a.size, n, rows))
    a = a.reshape(n, rows) if rows > 1 else a.reshape(n, 1)
    return np.ascontiguousarray(a.T.astype(np_t, copy=False)).tobytes()


def _sections(state):
    n = len(np.asarray(state["tag"]))
    nc = len(np.asarray(state["contact_partner"]))
    out = []
    for name, dt, rows in _ATOM_SECTIONS:
        out.append((name, dt, _columns(state[name], dt, rows, n, name)))
    out.append(("contact_count", DTYPE_I32, _columns(state["contact_count"], DTYPE_I32, 1, n, "contact_count")))
    out.append(("contact_partner", DTYPE_I32, _columns(state["contact_partner"], DTYPE_I32, 1, nc, "contact_partner")))
    out.append(("contact_shear", DTYPE_F64, _columns(state["contact_shear"], DTYPE_F64, 3, nc, "contact_shear")))
    for k, w in enumerate(state["walls"]):
        m = len(np.asarray(w["tag"]))
        out.append(("wall%d.tag" % k, DTYPE_I32, _columns(w["tag"], DTYPE_I32, 1, m, "wall tag")))
        out.append(("wall%d.shear" % k, DTYPE_F64, _columns(w["shear"], DTYPE_F64, 3, m, "wall shear")))
    return n, nc, out


def _order_ok(state):
    """what both readers require: ascending tags, counts >= 0 that sum to the contacts, partners above the atom's own tag
    and ascending within an atom, ascending wall tags; the text of what is wrong, or None"""
    tag = np.asarray(state["tag"], dtype=np.int64)
    if len(tag) > 1 and not (np.diff(tag) > 0).all():
        return "atoms must be in strictly ascending tag order"
    cc = np.asarray(state["contact_count"], dtype=np.int64)
    cp = np.asarray(state["contact_partner"], dtype=np.int64)
    if (cc < 0).any() or int(cc.sum()) != len(cp):
        return "contact_count does not sum to the number of contacts"
    if len(cp):
        own = np.repeat(tag, cc)
        first = np.zeros(len(cp), bool)
        first[(np.cumsum(cc) - cc)[cc > 0]] = True
        prev = np.where(first, own, np.concatenate(([0], cp[:-1])))
        if not (cp > prev).all():
            return "contact partners must be above the atom's own tag and ascending within an atom"
    for w in state["walls"]:
        wt = np.asarray(w["tag"], dtype=np.int64)
        if len(wt) > 1 and not (np.diff(wt) > 0).all():
            return "wall rows must be in strictly ascending tag order"
    return None


def to_bytes(state, check=True):
    """the file of a state (check=False: without the order checks, to make files a reader must refuse)"""
    bad = _order_ok(state) if check else None
    if bad:
        raise RestartError(bad)
    n, nc, secs = _sections(state)
    groups = list(state["groups"])
    walls = list(state["walls"])
    header_bytes = FIXED_BYTES + GROUP_BYTES * len(groups) + WALL_BYTES * len(walls) + SECTION_BYTES * len(secs) + 8
    off = header_bytes
    table = b""
    body = b""
    for name, dt, data in secs:
        table += _name(name, 24) + struct.pack("<IIQQ", dt, zlib.crc32(data) & 0xffffffff, off, len(data))
        body += data + b"\0" * (_pad8(len(data)) - len(data))
        off += _pad8(len(data))
    units = {"si": 0, "lj": 1}[state["units"]]
    fixed = struct.pack(_FIXED, MAGIC, VERSION, BOM, header_bytes, off, n, nc, int(state["step"]),
                        int(state["max_tag"]), float(state["dt"]), *[float(v) for v in state["boxlo"]],
                        *[float(v) for v in state["boxhi"]], *[int(v) for v in state["periodic"]], units, len(groups),
                        len(walls), len(secs))
    assert len(fixed) == FIXED_BYTES - 4
    head = fixed + struct.pack("<I", zlib.crc32(fixed) & 0xffffffff)
    for name, bit in groups:
        head += _name(name, 60) + struct.pack("<i", int(bit))
    for w in walls:
        head += _name(w["id"], 56) + struct.pack("<q", len(np.asarray(w["tag"])))
    head += table
    head += struct.pack("<II", zlib.crc32(head) & 0xffffffff, 0)
    assert len(head) == header_bytes
    return head + body


def write(path, state):
    """write `state` to `path` (through path + ".tmp" and a rename, like the engine)"""
    data = to_bytes(state)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _cstr(b):
    return b.split(b"\0", 1)[0].decode()


def _parse_header(data, path):
    """-> (dict, section table) of the file whose first bytes (at least the whole header, if the file has one) are `data`"""
    if len(data) < 16:
        raise RestartError("Restart file %s is truncated" % path)
    if data[:8] != MAGIC:
        raise RestartError("%s is not a sedifoam_amd restart file (bad magic)" % path)
    version, bom = struct.unpack("<II", data[8:16])
    if bom != BOM:
        if struct.unpack(">I", data[12:16])[0] == BOM:
            raise RestartError("Restart file %s was written with the other byte order" % path)
        raise RestartError("Restart file %s is corrupted" % path)
    if version > VERSION or version < 1:
        raise RestartError("Restart file %s has format version %d, this code reads up to version %d"
                           % (path, version, VERSION))
    if len(data) < FIXED_BYTES:
        raise RestartError("Restart file %s is truncated" % path)
    fixed = data[:FIXED_BYTES - 4]
    if struct.unpack("<I", data[FIXED_BYTES - 4:FIXED_BYTES])[0] != (zlib.crc32(fixed) & 0xffffffff):
        raise RestartError("Restart file %s is corrupted" % path)
    f = struct.unpack(_FIXED, fixed)
    header_bytes, file_bytes, n, nc, step, max_tag, dt = f[3:10]
    boxlo, boxhi, periodic = f[10:13], f[13:16], f[16:19]
    units, ngroups, nwalls, nsec = f[19:23]
    if header_bytes != FIXED_BYTES + GROUP_BYTES * ngroups + WALL_BYTES * nwalls + SECTION_BYTES * nsec + 8:
        raise RestartError("Restart file %s is corrupted" % path)
    if len(data) < header_bytes:
        raise RestartError("Restart file %s is truncated" % path)
    if struct.unpack("<I", data[header_bytes - 8:header_bytes - 4])[0] != (zlib.crc32(data[:header_bytes - 8]) & 0xffffffff):
        raise RestartError("Restart file %s is corrupted" % path)
    p = FIXED_BYTES
    groups = []
    for _ in range(ngroups):
        groups.append((_cstr(data[p:p + 60]), struct.unpack("<i", data[p + 60:p + 64])[0]))
        p += GROUP_BYTES
    walls = []
    for _ in range(nwalls):
        walls.append((_cstr(data[p:p + 56]), struct.unpack("<q", data[p + 56:p + 64])[0]))
        p += WALL_BYTES
    table = []
    for _ in range(nsec):
        dtp, crc, off, nb = struct.unpack("<IIQQ", data[p + 24:p + 48])
        table.append((_cstr(data[p:p + 24]), dtp, crc, off, nb))
        p += SECTION_BYTES
    h = dict(version=version, header_bytes=header_bytes, file_bytes=file_bytes, natoms=n, ncontacts=nc, step=step,
             max_tag=max_tag, dt=dt, boxlo=np.array(boxlo), boxhi=np.array(boxhi), periodic=tuple(periodic),
             units="lj" if units else "si", groups=groups, walls=walls,
             sections=[(t[0], t[3], t[4]) for t in table])
    return h, table


def header(path):
    """the header of a file: counts, step, box, units, groups, wall IDs with their row counts, the section table"""
    with open(path, "rb") as f:
        data = f.read(FIXED_BYTES)
        if len(data) == FIXED_BYTES and data[:8] == MAGIC:
            data += f.read(max(0, struct.unpack("<Q", data[16:24])[0] - FIXED_BYTES) if len(data) >= 24 else 0)
    return _parse_header(data, path)[0]


def from_bytes(data, path="<bytes>"):
    h, table = _parse_header(data, path)
    if len(data) < h["file_bytes"]:
        raise RestartError("Restart file %s is truncated" % path)
    if len(data) > h["file_bytes"]:
        raise RestartError("Restart file %s is corrupted" % path)
    n, nc = h["natoms"], h["ncontacts"]
    expect = [(nm, dt, rows * n) for nm, dt, rows in _ATOM_SECTIONS]
    expect += [("contact_count", DTYPE_I32, n), ("contact_partner", DTYPE_I32, nc), ("contact_shear", DTYPE_F64, 3 * nc)]
    for k, (_, m) in enumerate(h["walls"]):
        expect += [("wall%d.tag" % k, DTYPE_I32, m), ("wall%d.shear" % k, DTYPE_F64, 3 * m)]
    if len(expect) != len(table):
        raise RestartError("Restart file %s is corrupted" % path)
    arrays = {}
    end = h["header_bytes"]
    for (nm, dt, count), (name, dtp, crc, off, nb) in zip(expect, table):
        size = 4 if dt == DTYPE_I32 else 8
        # (a later version may append sections after these; the ones of version 1 keep their names, types and order)
        if name != nm or dtp != dt or nb != size * count or off != end or off + nb > len(data):
            raise RestartError("Restart file %s is corrupted" % path)
        raw = data[off:off + nb]
        if (zlib.crc32(raw) & 0xffffffff) != crc:
            raise RestartError("Restart file %s is corrupted" % path)
        arrays[name] = np.frombuffer(raw, dtype="<i4" if dt == DTYPE_I32 else "<f8")
        end = off + _pad8(nb)

    def rows3(a, m):
        return np.ascontiguousarray(a.reshape(3, m).T)

    st = dict(version=h["version"], step=h["step"], max_tag=h["max_tag"], dt=h["dt"], boxlo=h["boxlo"], boxhi=h["boxhi"],
              periodic=h["periodic"], units=h["units"], groups=h["groups"])
    for nm, dt, rows in _ATOM_SECTIONS:
        st[nm] = rows3(arrays[nm], n) if rows == 3 else arrays[nm].copy()
    st["contact_count"] = arrays["contact_count"].copy()
    st["contact_partner"] = arrays["contact_partner"].copy()
    st["contact_shear"] = rows3(arrays["contact_shear"], nc)
    st["walls"] = [dict(id=wid, tag=arrays["wall%d.tag" % k].copy(), shear=rows3(arrays["wall%d.shear" % k], m))
                   for k, (wid, m) in enumerate(h["walls"])]
    if _order_ok(st):
        raise RestartError("Restart file %s is corrupted" % path)
    return st


def read(path):
    """the state in a file; RestartError names what is wrong with a file that is not read"""
    with open(path, "rb") as f:
        data = f.read()
    return from_bytes(data, path)


def contacts(state):
    """{(tag_i, tag_j): shear[3]} with tag_i < tag_j, the form Lammps.history() returns"""
    ti = np.repeat(np.asarray(state["tag"]), np.asarray(state["contact_count"]))
    return {(int(a), int(b)): s.copy() for a, b, s in zip(ti, state["contact_partner"], state["contact_shear"])}


def wall_rows(state, k):
    """wall k's shear as a dense [n, 3] array in tag order (zero where the atom does not touch), like Lammps.wall_shear()"""
    out = np.zeros((len(state["tag"]), 3))
    w = state["walls"][k]
    out[np.searchsorted(state["tag"], w["tag"])] = w["shear"]
    return out


def without_history(state):
    """a copy of `state` with the contact and wall sections emptied (what a checkpoint that dropped them would hold)"""
    st = dict(state)
    st["contact_count"] = np.zeros(len(state["tag"]), np.int32)
    st["contact_partner"] = np.zeros(0, np.int32)
    st["contact_shear"] = np.zeros((0, 3))
    st["walls"] = [dict(id=w["id"], tag=np.zeros(0, np.int32), shear=np.zeros((0, 3))) for w in state["walls"]]
    return st
