"""tests/histo_model.py (the NumPy statement of the rules of fix ave/histo) against answers computed by
hand."""
import numpy as np
import pytest

from tests import histo_model as hm

VALUES = [1, 2, 1, 1, 2, 0.5, 3.0, 1.25, 1.999999]


@pytest.mark.parametrize("beyond,count,total,missing", [
    ("ignore", [3, 1, 0, 3], 7, 2),
    ("end", [4, 1, 0, 4], 9, 0),
    ("extra", [1, 3, 1, 0, 1, 3], 9, 0),   # (the two values equal to hi sit in the top extra bin)
])
def test_the_hand_computed_histograms(beyond, count, total, missing):
    bins = hm.Bins(1, 2, 4, beyond)
    b = hm.bin_values(bins, VALUES)
    assert b.count.tolist() == count and b.total == total and b.missing == missing
    assert b.min == 0.5 and b.max == 3.0   # (values beyond the range are included)
    assert b.frac.tolist() == [c / total for c in count]


def test_bins_and_coordinates():
    bins = hm.Bins(1, 2, 4)
    assert bins.nbins == 4 and bins.binsize == 0.25 and bins.bininv == 4.0
    assert bins.coord.tolist() == [1.125, 1.375, 1.625, 1.875]
    extra = hm.Bins(1, 2, 4, "extra")
    assert extra.nbins == 6 and extra.coord.tolist() == [1.0, 1.125, 1.375, 1.625, 1.875, 2.0]
    assert hm.Bins(-1, 1, 3, "end").coord.tolist() == [-1 + 0.5 * (2 / 3), -1 + 1.5 * (2 / 3), -1 + 2.5 * (2 / 3)]


def test_an_empty_input():
    bins = hm.Bins(1, 2, 4)
    b = hm.bin_values(bins, [])
    assert b.total == 0 and b.missing == 0 and b.min == 1.0e20 and b.max == -1.0e20 and not b.count.any()
    assert not b.frac.any()
    assert hm.text(30, bins, b) == ("30 4 0 0 1e+20 -1e+20\n1 1.125 0 0\n2 1.375 0 0\n3 1.625 0 0\n4 1.875 0 0\n")


def test_samples_accumulate_in_a_block_without_division():
    bins = hm.Bins(0, 10, 2, "end")
    b = hm.bin_values(bins, [1, 6])
    hm.bin_values(bins, [7, 8, 11], b)
    hm.bin_values(bins, [-3], b)
    assert b.count.tolist() == [2, 4] and b.total == 6 and b.missing == 0 and b.min == -3 and b.max == 11


def test_the_three_averages_over_four_blocks():
    bins = hm.Bins(0, 4, 4)
    data = [[0.5, 1.5], [2.5, 9.0], [3.5, 3.5, -1.0], [0.5]]
    blocks = [hm.bin_values(bins, d) for d in data]
    one, run, win = hm.Averager(4), hm.Averager(4, "running"), hm.Averager(4, "window", 2)
    got = [[a.output(b) for b in blocks] for a in (one, run, win)]
    assert [o.count.tolist() for o in got[0]] == [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 2], [1, 0, 0, 0]]
    assert [(o.total, o.missing, o.min, o.max) for o in got[0]] == [(2, 0, 0.5, 1.5), (1, 1, 2.5, 9.0), (2, 1, -1.0, 3.5), (1, 0, 0.5, 0.5)]
    assert [o.count.tolist() for o in got[1]] == [[1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 1, 2], [2, 1, 1, 2]]
    assert [(o.total, o.missing, o.min, o.max) for o in got[1]] == [(2, 0, 0.5, 1.5), (3, 1, 0.5, 9.0), (5, 2, -1.0, 9.0), (6, 2, -1.0, 9.0)]
    assert [o.count.tolist() for o in got[2]] == [[1, 1, 0, 0], [1, 1, 1, 0], [0, 0, 1, 2], [1, 0, 0, 2]]
    assert [(o.total, o.missing, o.min, o.max) for o in got[2]] == [(2, 0, 0.5, 1.5), (3, 1, 0.5, 9.0), (3, 2, -1.0, 9.0), (3, 1, -1.0, 3.5)]


def test_the_file_text():
    bins = hm.Bins(1, 2, 4, "extra")
    b = hm.bin_values(bins, VALUES)
    assert hm.header("h") == ("# Histogrammed data for fix h\n"
                              "# TimeStep Number-of-bins Total-counts Missing-counts Min-value Max-value\n"
                              "# Bin Coord Count Count/Total\n")
    assert hm.header("h", "# a b", None, "# c") == ("# a b\n# TimeStep Number-of-bins Total-counts Missing-counts Min-value "
                                                    "Max-value\n# c\n")
    assert hm.text(100, bins, b) == ("100 6 9 0 0.5 3\n1 1 1 0.111111\n2 1.125 3 0.333333\n3 1.375 1 0.111111\n4 1.625 0 0\n"
                                     "5 1.875 1 0.111111\n6 2 3 0.333333\n")


def test_every_value_on_an_edge():
    """ids 1 .. 108 in 107 bins of width 1: value k sits on the lower edge of bin k - 1, and the last bin also holds 108"""
    b = hm.bin_values(hm.Bins(1, 108, 107), np.arange(1, 109))
    assert b.count.tolist() == [1] * 106 + [2] and b.total == 108 and b.missing == 0
