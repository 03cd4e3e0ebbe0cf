"""tests/pchunk_model.py, the NumPy statement of `compute chunk/atom c_CID` and of the per-chunk computes (DESIGN.md section
22), held to answers computed by hand."""
import numpy as np

from tests import pchunk_model as pm


def test_three_grains_in_two_chunks():
    # chunk 1: masses 1 and 3 at x = 0 and 4 -> com 3, Rg^2 = (1 * 9 + 3 * 1) / 4 = 3; chunk 2: one grain
    chunk, n, ids = pm.chunk_ids([1.0, 1.0, 2.0], [True] * 3)
    assert chunk.tolist() == [1, 1, 2] and n == 2 and ids.tolist() == [1, 2]
    xu = np.array([[0.0, 1.0, 0.0], [4.0, 1.0, 0.0], [7.0, -2.0, 5.0]])
    v = np.array([[2.0, 0.0, 0.0], [-2.0, 4.0, 0.0], [1.0, 1.0, 1.0]])
    r = pm.per_chunk(chunk, n, [True] * 3, [1.0, 3.0, 0.5], xu, v)
    assert r["count"].tolist() == [2.0, 1.0]
    assert r["com"].tolist() == [[3.0, 1.0, 0.0], [7.0, -2.0, 5.0]]
    assert r["vcm"].tolist() == [[-1.0, 3.0, 0.0], [1.0, 1.0, 1.0]]
    assert r["rg"].tolist() == [np.sqrt(3.0), 0.0]
    assert r["tensor"].tolist() == [[3.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0] * 6]


def test_a_gap_chunk_reads_zero_and_a_grain_outside_the_group_does_not_count():
    chunk, n, ids = pm.chunk_ids([1.0, 3.0, 3.0, 2.0], [True, True, True, False])
    assert chunk.tolist() == [1, 3, 3, 0] and n == 3 and ids.tolist() == [1, 2, 3]
    xu = np.array([[1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0], [9.0, 9, 9]])
    r = pm.per_chunk(chunk, n, [True, True, False, True], [2.0, 1.0, 1.0, 1.0], xu, xu)
    assert r["count"].tolist() == [1.0, 0.0, 1.0]            # the third grain is not in the per-chunk compute's group
    assert r["com"].tolist() == [[1.0, 0, 0], [0.0, 0, 0], [2.0, 0, 0]]
    assert r["vcm"][1].tolist() == [0.0] * 3 and r["rg"].tolist() == [0.0] * 3


def test_the_cast_truncates_toward_zero():
    chunk, n, _ = pm.chunk_ids([2.9, -0.5, 0.99, 1.0, -3.2, 3.999], [True] * 6)
    assert chunk.tolist() == [2, 0, 0, 1, 0, 3] and n == 3


def test_compression_sorts_the_distinct_ids():
    chunk, n, ids = pm.chunk_ids([7.0, 3.0, 7.0, 12.0], [True] * 4, compress=True)
    assert chunk.tolist() == [2, 1, 2, 3] and n == 3 and ids.tolist() == [3, 7, 12]
    chunk, n, ids = pm.chunk_ids([7.0, 3.0, 7.0, 12.0], [True, False, True, True], compress=True)
    assert chunk.tolist() == [1, 0, 1, 2] and n == 2 and ids.tolist() == [7, 12]
    chunk, n, ids = pm.chunk_ids([7.0, 0.2], [False, True], compress=True)
    assert chunk.tolist() == [0, 0] and n == 0 and ids.tolist() == []


def test_nchunk_once_discards_what_lies_above_it():
    chunk, n, ids = pm.chunk_ids([1.0, 5.0, 2.0], [True] * 3, nchunk=2)
    assert chunk.tolist() == [1, 0, 2] and n == 2 and ids.tolist() == [1, 2]
    chunk, n, ids = pm.chunk_ids([], [], compress=False)
    assert chunk.tolist() == [] and n == 0


def test_the_gate_is_taken_per_column():
    want = np.array([[1.0, 0.0], [2.0, 0.0]])
    assert pm.within_gate(want, want) == 0.0
    assert pm.within_gate(want + [[1e-13, 0.0], [0.0, 0.0]], want) <= 1.0
    for bad in (want + [[3e-13, 0.0], [0.0, 0.0]], want + [[0.0, 1e-300], [0.0, 0.0]]):
        try:
            pm.within_gate(bad, want)
        except AssertionError:
            continue
        raise AssertionError("a miss went through")
    # a sum that cancels is held against its terms
    assert pm.within_gate([[1e-9 + 1e-14]], [[1e-9]], scale=[[1.0]]) <= 1.0


def test_the_scale_is_made_of_the_absolute_products():
    r = pm.per_chunk([1, 1], 1, [True, True], [1.0, 1.0], [[-1.0, 0, 0], [1.0, 0, 0]], [[2.0, 0, 0], [-2.0, 0, 0]])
    assert r["com"].tolist() == [[0.0, 0.0, 0.0]] and r["scale"]["com"].tolist() == [[1.0, 0.0, 0.0]]
    assert r["vcm"].tolist() == [[0.0, 0.0, 0.0]] and r["scale"]["vcm"].tolist() == [[2.0, 0.0, 0.0]]
    assert r["scale"]["tensor"].tolist() == r["tensor"].tolist() == [[1.0, 0, 0, 0, 0, 0]] and r["scale"]["rg"].tolist() == [1.0]
