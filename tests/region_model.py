"""The NumPy statement of regions and of the groups made of them: the primitives, `side`, union and
intersect, and the schedule of a dynamic group.  Every expression is written operation for operation as the rules give it;
nothing here is fused, so the comparisons have the bits the device's region_match() has.

A region is a tuple:
    ("block", xlo, xhi, ylo, yhi, zlo, zhi, side)          side: "in" | "out"
    ("sphere", x, y, z, r, side)
    ("cylinder", axis, c1, c2, r, lo, hi, side)            axis: "x" | "y" | "z"; c1 c2: y z for x, x z for y, x y for z
    ("plane", px, py, pz, nx, ny, nz, side)                the normal as typed: it is normalised here as at the definition
    ("union", [regions], side) / ("intersect", [regions], side)
INF is -+BIG; EDGE is the caller's box bound."""
import numpy as np

BIG = 1.0e20


def inside(region, p):
    """the primitive's own `inside`, before side; p: (n, 3) float64 (a square that overflows is inf, and inf <= r is false)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _inside(region, p)


def _inside(region, p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    style = region[0]
    if style == "block":
        xlo, xhi, ylo, yhi, zlo, zhi = [np.float64(v) for v in region[1:7]]
        return (x >= xlo) & (x <= xhi) & (y >= ylo) & (y <= yhi) & (z >= zlo) & (z <= zhi)
    if style == "sphere":
        cx, cy, cz, r = [np.float64(v) for v in region[1:5]]
        dx, dy, dz = x - cx, y - cy, z - cz
        return np.sqrt((dx * dx + dy * dy) + dz * dz) <= r
    if style == "cylinder":
        axis = region[1]
        c1, c2, r, lo, hi = [np.float64(v) for v in region[2:7]]
        u, v, a = {"x": (y, z, x), "y": (x, z, y), "z": (x, y, z)}[axis]
        d1, d2 = u - c1, v - c2
        return (np.sqrt(d1 * d1 + d2 * d2) <= r) & (a >= lo) & (a <= hi)
    if style == "plane":
        px, py, pz, nx, ny, nz = [np.float64(v) for v in region[1:7]]
        length = np.sqrt(nx * nx + ny * ny + nz * nz)
        n0, n1, n2 = nx / length, ny / length, nz / length
        return ((x - px) * n0 + (y - py) * n1) + (z - pz) * n2 >= 0.0
    raise ValueError(style)


def match(region, p):
    """inside for side in, not inside for side out; union / intersect: any / all of the sub-regions' MATCHES, then this side"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    style, side = region[0], region[-1]
    assert side in ("in", "out")
    if style in ("union", "intersect"):
        subs = [match(r, p) for r in region[1]]
        assert len(subs) >= 2
        m = np.any(subs, axis=0) if style == "union" else np.all(subs, axis=0)
    else:
        m = inside(region, p)
    return ~m if side == "out" else m


def on_boundary(region, p):
    """exactly on the surface of a primitive (the equality of its own comparison holds)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _on_boundary(region, p)


def _on_boundary(region, p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    style = region[0]
    if style == "block":
        b = [np.float64(v) for v in region[1:7]]
        face = (x == b[0]) | (x == b[1]) | (y == b[2]) | (y == b[3]) | (z == b[4]) | (z == b[5])
        return face & inside(region, p)
    if style == "sphere":
        dx, dy, dz = x - region[1], y - region[2], z - region[3]
        return np.sqrt((dx * dx + dy * dy) + dz * dz) == np.float64(region[4])
    if style == "cylinder":
        u, v, a = {"x": (y, z, x), "y": (x, z, y), "z": (x, y, z)}[region[1]]
        d1, d2 = u - region[2], v - region[3]
        return (np.sqrt(d1 * d1 + d2 * d2) == np.float64(region[4])) & (a >= region[5]) & (a <= region[6])
    if style == "plane":
        nx, ny, nz = [np.float64(v) for v in region[4:7]]
        length = np.sqrt(nx * nx + ny * ny + nz * nz)
        return ((x - region[1]) * (nx / length) + (y - region[2]) * (ny / length)) + (z - region[3]) * (nz / length) == 0.0
    raise ValueError(style)


def command(rid, region):
    """the input-script line of a primitive region (its numbers with 17 digits: read back to the same bits)"""
    style, side = region[0], region[-1]
    words = []
    for v in region[1:-1]:
        if isinstance(v, str):
            words.append(v)
        elif abs(v) == BIG:
            words.append("INF")
        else:
            words.append("%.17g" % v)
    return "region %s %s %s side %s units box" % (rid, style, " ".join(words), side)


def dynamic_group(mask_parent, region, x):
    """(mask & parentbit) && match"""
    return np.asarray(mask_parent, bool) & match(region, x)


def deciding_steps(start, pieces, every, defined_before_first=True):
    """Which step's positions decide the membership seen after each piece of running.

    start: the step counter at the beginning; pieces: [("run" | "step", n), ...]; every: N.  A dynamic group is evaluated
      * at every step t of a piece with t % N == 0 (the end-of-step state of t),
      * at the setup of a `run` piece (its first step, whatever it is),
      * at the beginning of the first piece after its definition, `run` or `step`;
    a `step` piece has no setup, and a cut of the run is not one.  Returns the deciding step after each piece (None while the
    group has never been evaluated)"""
    t = int(start)
    last = None
    fresh = bool(defined_before_first)
    out = []
    for kind, n in pieces:
        assert kind in ("run", "step") and n >= 0
        if kind == "run" or fresh:
            last = t
        fresh = False
        end = t + n
        m = (end // every) * every          # the last multiple of N in (t, end]
        if m > t:
            last = m
        t = end
        out.append(last)
    return out
