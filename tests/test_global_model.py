"""tests/global_model.py against answers computed by hand (no GPU, no engine)."""
import numpy as np
import pytest

from tests import global_model as gm

COL = [3.0, -1.0, 4.0, -1.5, 2.0]
HALF = [1, 0, 1, 0, 1]


@pytest.mark.parametrize("mode,want", [("sum", 6.5), ("min", -1.5), ("max", 4.0), ("ave", 1.3), ("sumsq", 32.25),
                                       ("avesq", 6.45)])
def test_a_five_value_column_under_each_mode(mode, want):
    assert gm.reduce(mode, COL) == want
    assert gm.reduce(mode, COL, [1] * 5) == want


@pytest.mark.parametrize("mode,want", [("sum", 9.0), ("min", 2.0), ("max", 4.0), ("ave", 3.0), ("sumsq", 29.0),
                                       ("avesq", 29.0 / 3.0)])
def test_a_group_mask_selects_the_elements(mode, want):
    assert gm.reduce(mode, COL, HALF) == want


@pytest.mark.parametrize("mode,want", [("sum", 0.0), ("min", 1.0e20), ("max", -1.0e20), ("ave", 0.0), ("sumsq", 0.0),
                                       ("avesq", 0.0)])
def test_an_empty_set_gives_the_initial_values_and_does_not_divide(mode, want):
    assert gm.reduce(mode, COL, [0] * 5) == want
    assert gm.reduce(mode, []) == want
    assert gm.gate(mode, COL, [0] * 5) == 0.0


def test_the_gate_is_twice_n_half_ulps_of_the_sum_of_magnitudes():
    assert gm.gate("sum", COL) == 2 * 5 * 2.0 ** -53 * 11.5
    assert gm.gate("sumsq", COL, HALF) == 2 * 3 * 2.0 ** -53 * 29.0
    assert gm.gate("min", COL) == 0.0 and gm.gate("max", COL) == 0.0
    assert gm.gate("ave", COL) == 2 * 5 * 2.0 ** -53 * 11.5 / 5 + 2 * 2.0 ** -53 * 1.3
    assert gm.extensive("sum") and gm.extensive("sumsq")
    assert not any(gm.extensive(m) for m in ("min", "max", "ave", "avesq"))


def test_output_steps_of_2_3_10():
    assert gm.schedule(0, 2, 3, 10, 30) == [(10, [6, 8, 10]), (20, [16, 18, 20]), (30, [26, 28, 30])]
    assert gm.schedule(7, 2, 3, 10, 30) == [(20, [16, 18, 20]), (30, [26, 28, 30])]


def test_output_steps_of_10_1_10():
    assert gm.schedule(0, 10, 1, 10, 25) == [(0, [0]), (10, [10]), (20, [20])]
    assert gm.schedule(7, 10, 1, 10, 25) == [(10, [10]), (20, [20])]


def test_start_25_with_5_2_10():
    assert gm.first_valid(0, 5, 2, 10, start=25) == 25
    assert gm.schedule(0, 5, 2, 10, 50, start=25) == [(30, [25, 30]), (40, [35, 40]), (50, [45, 50])]
    # defined at step 30, an output step: the next one
    assert gm.schedule(30, 5, 2, 10, 50, start=25) == [(40, [35, 40]), (50, [45, 50])]
    # start at or before the first output changes nothing
    assert gm.schedule(0, 5, 2, 10, 30, start=10) == gm.schedule(0, 5, 2, 10, 30)


def _run(ave, window=0):
    a = gm.TimeAverager(1, 2, ave, window)
    out = []
    for block in (1.0, 2.0, 4.0, 8.0):   # two samples each, block - 0.5 and block + 0.5
        a.add_sample([block - 0.5])
        a.add_sample([block + 0.5])
        out.append(float(a.output()[0]))
    return out


def test_one_running_and_window_2_over_four_blocks():
    assert _run("one") == [1.0, 2.0, 4.0, 8.0]
    assert _run("running") == [1.0, 1.5, 7.0 / 3.0, 3.75]
    assert _run("window", 2) == [1.0, 1.5, 3.0, 6.0]
    assert _run("window", 9) == _run("running")


def test_two_values_are_averaged_apart():
    a = gm.TimeAverager(2, 1, "running")
    a.add_sample([1.0, 10.0])
    assert a.output().tolist() == [1.0, 10.0]
    a.add_sample([3.0, 30.0])
    assert a.output().tolist() == [2.0, 20.0]


def test_the_file_text():
    assert gm.header("t", ["c_r", "c_v[2]"]) == "# Time-averaged data for fix t\n# TimeStep c_r c_v[2]\n"
    assert gm.header("t", ["c_r"], "# my title", "# step value") == "# my title\n# step value\n"
    assert gm.line(30, [1.5, -2.0e-7]) == "30 1.5 -2e-07\n"
    assert gm.line(30, [1.0 / 3.0], " %.10g") == "30 0.3333333333\n"
    assert gm.line(30, [1.0 / 3.0, 2.0], "%.10g") == "300.33333333332\n"   # (the format is applied as given)


def test_a_thermo_cell_and_its_normalisation():
    assert gm.thermo_cell(1.0 / 3.0) == "  0.33333333 "
    assert gm.thermo_cell(-1.0e20) == "      -1e+20 "
    assert gm.thermo_value(10.0, True, True, 4) == 2.5
    assert gm.thermo_value(10.0, True, False, 4) == 10.0
    assert gm.thermo_value(10.0, False, True, 4) == 10.0
    assert gm.thermo_value(10.0, True, True, 0) == 10.0
