"""NumPy statement of `compute chunk/atom c_CID` and of the per-chunk computes property/chunk, com/chunk, vcm/chunk and
gyration/chunk: what the GPU path is held to.  Chunk IDs, Nchunk, the originals and the counts are
integers and compare with ==; the sums are made in atom order, one addition after the other, and the GPU's differ from them
by the order of summation only (tests/chunk_model.py GATE)."""
import numpy as np

from tests.chunk_model import GATE   # noqa: F401  (1e-13 per entry against the column's scale, as in tests/chunk_model.py)


def chunk_ids(value, in_group, compress=False, nchunk=None):
    """(chunk int32 [n], Nchunk, ids int32 [Nchunk]) from a per-atom column.  A grain outside the group gets chunk 0;
    otherwise raw = (int)value, a C cast (toward zero), and raw < 1 gives chunk 0.  compress no: the chunk is raw, Nchunk the
    largest raw -- or `nchunk`, what an earlier evaluation fixed under nchunk once -- and raw > Nchunk gives chunk 0; ids is
    1 .. Nchunk.  compress yes: the distinct positive raw values in ascending order become chunks 1 .. Nchunk; ids lists them"""
    value = np.asarray(value, np.float64)
    raw = np.where(np.asarray(in_group, bool), np.trunc(value), 0.0).astype(np.int64)
    raw[raw < 1] = 0
    if compress:
        ids = np.unique(raw[raw > 0])
        chunk = np.where(raw > 0, np.searchsorted(ids, raw) + 1, 0)
        return chunk.astype(np.int32), int(len(ids)), ids.astype(np.int32)
    n = int(raw.max()) if nchunk is None and len(raw) else int(nchunk or 0)
    chunk = np.where(raw > n, 0, raw)
    return chunk.astype(np.int32), n, np.arange(1, n + 1, dtype=np.int32)


def _sum(chunk, nchunk, weights):
    """per chunk 1 .. nchunk, added in atom order"""
    return np.bincount(chunk, weights=weights, minlength=nchunk + 1)[1:nchunk + 1]


def per_chunk(chunk, nchunk, member, mass, xu, v):
    """dict(count [N], com [N, 3], vcm [N, 3], rg [N], tensor [N, 6]) over the grains with member and chunk > 0; xu: the
    unwrapped positions x + image * L.  A chunk without such a grain reads 0 everywhere.  The centre that gyration subtracts
    is com's; a chunk of one grain has that grain as its centre, so its Rg and tensor are exactly 0.
    "scale": a dict of the same four arrays computed from the |products| (sum m |xu| / sum m, ..., sum m |dx dy| / sum m):
    what the gate is taken against, as tests/chunk_model.py takes its scale from an Averager fed |columns|"""
    chunk = np.where(np.asarray(member, bool), np.asarray(chunk, np.int64), 0)
    mass, xu, v = np.asarray(mass, np.float64), np.asarray(xu, np.float64).reshape(-1, 3), np.asarray(v, np.float64).reshape(-1, 3)
    count = _sum(chunk, nchunk, np.ones(len(chunk)))
    m = _sum(chunk, nchunk, mass)
    safe = np.where(m > 0, m, 1.0)
    com = np.stack([_sum(chunk, nchunk, mass * xu[:, a]) for a in range(3)], axis=1) / safe[:, None]
    vcm = np.stack([_sum(chunk, nchunk, mass * v[:, a]) for a in range(3)], axis=1) / safe[:, None]
    com[m == 0], vcm[m == 0] = 0.0, 0.0
    centre = np.vstack([np.zeros((1, 3)), com])[chunk]
    single = np.concatenate([[False], count == 1])[chunk]
    d = np.where(single[:, None], 0.0, xu - centre)
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    tensor = np.stack([_sum(chunk, nchunk, mass * (d[:, i] * d[:, j])) for i, j in pairs], axis=1)
    rg = np.sqrt(((tensor[:, 0] + tensor[:, 1]) + tensor[:, 2]) / safe)
    tensor = tensor / safe[:, None]
    rg[m == 0], tensor[m == 0] = 0.0, 0.0
    scale = dict(com=np.stack([_sum(chunk, nchunk, mass * np.abs(xu[:, a])) for a in range(3)], axis=1) / safe[:, None],
                 vcm=np.stack([_sum(chunk, nchunk, mass * np.abs(v[:, a])) for a in range(3)], axis=1) / safe[:, None],
                 tensor=np.stack([_sum(chunk, nchunk, mass * np.abs(d[:, i] * d[:, j])) for i, j in pairs], axis=1) / safe[:, None],
                 rg=rg)
    return dict(count=count, com=com, vcm=vcm, rg=rg, tensor=tensor, scale=scale)


def within_gate(got, want, scale=None):
    """every entry of `got` within GATE of `want`, taken against the largest entry of its column in `scale` -- the same column
    as the model computes it from the |products| (default: |want| itself, which is that where nothing cancels); a column whose
    scale is 0 is exact.  Returns the largest error in units of the gate (0 where a column's scale is 0 and it is met)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    g2, w2 = got.reshape(len(want), -1), want.reshape(len(want), -1)
    s2 = np.abs(w2) if scale is None else np.abs(np.asarray(scale, np.float64)).reshape(len(want), -1)
    worst = 0.0
    for c in range(w2.shape[1]):
        scale = s2[:, c].max()
        err = np.abs(g2[:, c] - w2[:, c]).max()
        assert err <= GATE * scale, (c, err, scale)
        if scale > 0:
            worst = max(worst, err / (GATE * scale))
    return worst
