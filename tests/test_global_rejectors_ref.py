"""Pins tests/global_rejectors_ref.py, the numpy restatement the global correspondence rejectors are tested against, on cases
worked by hand (include/ope.h states the rules).  No GPU."""
import math

import numpy as np
import pytest

import global_rejectors_ref as R

MARGIN = 1e-9   # every var-trimmed input must decide its arg-min by at least this (global_rejectors_ref.var_trimmed)


def f32(*v):
    return np.array(v, np.float32)


# ---- median distance: position m / 2 of the ascending order (the upper middle for even m)
@pytest.mark.parametrize("d, median, keep", [
    ([4.0], 4.0, [1]),
    ([4.0, 1.0], 4.0, [1, 1]),
    ([4.0, 1.0, 2.0], 2.0, [0, 1, 1]),
    ([4.0, 1.0, 2.0, 3.0], 3.0, [0, 1, 1, 1]),
])
def test_median_position_is_m_over_two(d, median, keep):
    k, st = R.median_distance(f32(*d), 1.0)
    assert st["threshold"] == median and st["n_in"] == len(d)
    assert k.tolist() == [bool(x) for x in keep] and st["n_out"] == sum(keep)
    assert math.isnan(st["ratio"])


def test_median_factor_scales_the_threshold_in_fp64():
    d = f32(1.0, 2.0, 3.0, 4.0, 5.0)        # median 3, factor 0.8 -> 2.4
    k, st = R.median_distance(d, 0.8)
    assert st["threshold"] == 3.0 and k.tolist() == [True, True, False, False, False]


def test_median_factor_zero_keeps_only_zero_distances():
    k, st = R.median_distance(f32(0.0, 1.0, 0.0, 2.0), 0.0)
    assert k.tolist() == [True, False, True, False] and st["n_out"] == 2
    k, _ = R.median_distance(f32(1.0, 2.0, 3.0), 0.0)
    assert not k.any()


def test_median_all_equal_keeps_all_at_factor_one_and_none_below():
    d = f32(*[0.25] * 7)
    k, st = R.median_distance(d, 1.0)
    assert k.all() and st["threshold"] == 0.25
    k, _ = R.median_distance(d, 0.999)
    assert not k.any()


def test_median_of_nothing_keeps_nothing():
    k, st = R.median_distance(f32(), 0.8)
    assert len(k) == 0 and st["n_in"] == 0 and st["n_out"] == 0 and math.isnan(st["threshold"])


# ---- one to one
def test_one_to_one_keeps_the_nearest_query_of_each_target_in_query_order():
    q = [0, 1, 2, 3, 4]
    t = [7, 7, 3, 7, 3]
    d = f32(0.5, 0.2, 0.9, 0.3, 0.1)
    k, st = R.one_to_one(q, t, d)
    assert k.tolist() == [False, True, False, False, True]
    assert st["n_in"] == 5 and st["n_out"] == 2 and math.isnan(st["threshold"]) and math.isnan(st["ratio"])


def test_one_to_one_tie_goes_to_the_smallest_query_index():
    # the same distance twice onto target 5: query 2 wins over query 9, wherever they stand in the list
    k, _ = R.one_to_one([9, 2, 4], [5, 5, 5], f32(0.25, 0.25, 0.5))
    assert k.tolist() == [False, True, False]
    k, _ = R.one_to_one([2, 9, 4], [5, 5, 5], f32(0.25, 0.25, 0.5))
    assert k.tolist() == [True, False, False]


def test_one_to_one_drops_pairs_without_a_match():
    k, st = R.one_to_one([0, 1, 2], [-1, 4, -1], f32(0.1, 0.2, 0.3))
    assert k.tolist() == [False, True, False] and st["n_in"] == 3 and st["n_out"] == 1


# ---- var trimmed
def test_var_trimmed_of_two_keeps_nothing():
    # lo = 0, hi = 1: best = 0, ratio = 0, idx = 0, trimmed = s[0]; the comparison is strict
    k, st = R.var_trimmed(f32(3.0, 1.0))
    assert st["best"] == 0 and st["idx"] == 0 and st["ratio"] == 0.0 and st["threshold"] == 1.0
    assert not k.any() and st["n_out"] == 0


def test_var_trimmed_of_three_by_hand():
    # defaults: lo = 0, hi = 2, L = 0.  FRMS_0 = (27)^2 * 1 * s0 = 729 s0, FRMS_1 = (27/8)^2 / 2 * s1 = 5.6953125 s1
    d = f32(1.0, 4.0, 100.0)
    k, st = R.var_trimmed(d)
    assert st["margin"] >= MARGIN
    assert st["best"] == 1                       # 22.78 < 729
    assert st["ratio"] == float(np.float32(1) / np.float32(3))
    assert st["idx"] == int(3.0 * st["ratio"]) == 1 and st["threshold"] == 4.0
    assert k.tolist() == [True, False, False]
    # with s1 large the first position wins: 729 * 1 < 5.6953125 * 200
    k, st = R.var_trimmed(f32(1.0, 200.0, 300.0))
    assert st["best"] == 0 and st["idx"] == 0 and not k.any()


@pytest.mark.parametrize("m, best, idx", [(20, 13, 12), (257, 179, 178)])
def test_var_trimmed_interior_minimum_and_the_fp32_ratio_round_trip(m, best, idx):
    d = R.mixture(m, 0)
    k, st = R.var_trimmed(d, 0.3, 0.95)
    assert st["margin"] >= MARGIN
    lo, hi = int(0.3 * m), int(0.95 * m)
    assert lo < st["best"] < hi - 1              # interior
    assert (st["best"], st["idx"]) == (best, idx)   # int(double(m) * double(float(best) / float(m))) falls one short
    s = np.sort(d.astype(np.float64))
    assert st["threshold"] == s[idx] and st["n_out"] == int((d.astype(np.float64) < s[idx]).sum()) == idx
    assert k.sum() == st["n_out"] and (d[k] < 1e-5).all()   # every outlier falls


def test_var_trimmed_frms_is_pcl_expression_with_the_head_sum_only():
    # m = 10, min 0.3, max 0.95: lo = 3, hi = 9, L = s0 + s1 + s2
    d = f32(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
    _, st = R.var_trimmed(d, 0.3, 0.95)
    L = 6.0
    frms = [(1.0 / ((j + 1) / 10.0) ** 3) ** 2 / (j + 1) * (float(j + 1) + L) for j in range(3, 9)]
    assert st["best"] == 3 + int(np.argmin(frms)) == 8
    assert st["margin"] >= MARGIN


@pytest.mark.parametrize("d, lo_r, hi_r", [([], 0.05, 0.95), ([2.0], 0.05, 0.95), ([1.0, 2.0, 3.0], 0.5, 0.5), ([1.0, 2.0, 3.0, 4.0], 0.3, 0.4)])
def test_var_trimmed_with_an_empty_range_keeps_everything(d, lo_r, hi_r):
    k, st = R.var_trimmed(f32(*d), lo_r, hi_r)
    assert k.all() and st["n_out"] == len(d) and st["ratio"] == 1.0 and math.isnan(st["threshold"])


def test_mixtures_decide_their_minimum_by_far_more_than_the_margin():
    for m in (64, 255, 256, 257, 1000, 70001):
        assert R.var_trimmed(R.mixture(m, 0), 0.3, 0.95)[1]["margin"] >= 6e-5


# ---- lists
def test_a_list_applies_each_rejector_to_the_survivors_of_the_one_before():
    q = np.arange(6)
    t = np.array([0, 0, 1, 1, 2, 2])
    d = f32(0.1, 0.2, 0.9, 0.8, 0.3, 0.4)
    mask, st = R.apply_list([dict(kind=R.ONE_TO_ONE), dict(kind=R.MEDIAN_DISTANCE, factor=0.8)], q, t, d)
    # one to one leaves {0.1, 0.8, 0.3}; their median is 0.3, times 0.8: only 0.1 stays
    assert st[0]["n_out"] == 3 and st[1]["n_in"] == 3 and st[1]["threshold"] == float(np.float32(0.3))
    assert mask.tolist() == [True, False, False, False, False, False]
    # the other order: the median of all six is 0.4 (position 3), times 0.8 keeps {0.1, 0.2, 0.3}; one to one then drops 0.2
    mask, st = R.apply_list([dict(kind=R.MEDIAN_DISTANCE, factor=0.8), dict(kind=R.ONE_TO_ONE)], q, t, d)
    assert mask.tolist() == [True, False, False, False, True, False] and st[1]["n_in"] == 3
