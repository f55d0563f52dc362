"""tests/corr_sac_ref.py pinned on its own (no GPU, no library): matches against cKDTree, the draws against plane_ref's, the fit
against an independent Kabsch, the threshold against numpy's eigenvalues, the loop's k by hand, the cases without a model."""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import corr_sac_ref as ref
import plane_ref

F = np.float32


def rigid(deg=(25.0, -40.0, 60.0), t=(0.05, -0.02, 0.11)):
    a, b, c = np.radians(deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def kabsch(s, t):
    """Independent fp64 rigid fit: centred cross-covariance, numpy SVD, reflection guard."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    cs, ct = s.mean(0), t.mean(0)
    H = (s - cs).T @ (t - ct)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ct - R @ cs
    return T


def test_matches_equal_a_kd_tree_on_tie_free_rows():
    rng = np.random.default_rng(3)
    fs = rng.uniform(0, 100, (150, 33)).astype(F)
    ft = rng.uniform(0, 100, (211, 33)).astype(F)
    ft[17] = fs[5]                                   # an exact match: distance 0
    si, ti, d, dropped = ref.feature_matches(fs, ft)
    dist, idx = cKDTree(ft.astype(np.float64)).query(fs.astype(np.float64))
    assert dropped == 0
    np.testing.assert_array_equal(si, np.arange(150))
    np.testing.assert_array_equal(ti, idx)
    assert ti[5] == 17 and d[5] == 0.0
    np.testing.assert_allclose(d, dist * dist, rtol=33 * 2.0 ** -23)   # a float32 sum of 33 non-negative terms


def test_matches_ties_take_the_lowest_index_and_nan_rows_drop():
    rng = np.random.default_rng(4)
    ft = rng.uniform(0, 100, (20, 33)).astype(F)
    ft[11] = ft[3]                                   # two equal target rows
    fs = np.stack([ft[11], ft[7], np.full(33, np.nan, F)])
    si, ti, d, dropped = ref.feature_matches(fs, ft)
    assert dropped == 1
    np.testing.assert_array_equal(si, [0, 1])
    np.testing.assert_array_equal(ti, [3, 7])
    assert ref.feature_matches(fs, np.zeros((0, 33), F))[3] == 3


@pytest.mark.parametrize("n", [3, 4, 57])
def test_draws_equal_plane_refs_for_the_same_seed_and_size(n):
    pts = np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(F)   # no three of them on a line: plane_ref redraws nothing
    want = plane_ref.draw_samples(pts, 40, 12345)
    got = ref.draw_samples(pts, 40, 12345, -1.0)                       # every edge is > -1: nothing is redrawn here either
    assert len(want) == 40
    np.testing.assert_array_equal(got, want)
    if n == 3:
        assert all(sorted(s) == [0, 1, 2] for s in got.tolist())


def test_draws_redraw_short_triangles():
    pts = np.random.default_rng(9).uniform(-1, 1, (30, 3)).astype(F)
    thr = 0.5
    got = ref.draw_samples(pts, 25, 12345, thr)
    free = ref.draw_samples(pts, 25, 12345, -1.0)
    assert len(got) == 25 and not np.array_equal(got, free)
    for a, b, c in got:
        assert min(float(ref.d2(pts[a], pts[b])), float(ref.d2(pts[a], pts[c])), float(ref.d2(pts[b], pts[c]))) > thr


def test_threshold_against_numpy_eigenvalues():
    pts = (np.random.default_rng(2).normal(size=(400, 3)) * [0.3, 0.1, 0.02] + [0.5, -0.2, 1.0]).astype(F)
    ev = np.linalg.eigvalsh(np.cov(pts.astype(np.float64).T, bias=True))
    want = (np.sqrt(ev).sum() / 3.0) ** 2
    assert ref.sample_dist_thresh(pts) == pytest.approx(want, rel=2e-3)    # float32 running sums of 400 terms, offset cloud
    assert ref.sample_dist_thresh(np.zeros((50, 3), F)) == 0.0             # coincident points at the origin: exactly 0
    t = ref.sample_dist_thresh(np.tile(pts[:1], (50, 1)))                  # elsewhere the running sums leave a residue of either sign:
    assert math.isnan(t) or 0.0 <= t < 1e-6                                # a tiny threshold, or NaN (the root of a negative eigenvalue)


def test_fit_against_an_independent_kabsch():
    rng = np.random.default_rng(5)
    T = rigid()
    worst = 0.0
    for _ in range(50):
        s = rng.uniform(-0.2, 0.2, (3, 3)).astype(F)
        t = (s.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
        if ref.prerejective_ref.singular_ratio(s) < 0.1:
            continue
        worst = max(worst, float(np.abs(ref.fit(s, t).astype(np.float64) - kabsch(s, t)).max()))
    assert worst <= 2e-6, worst                                            # float32 inputs and outputs of order 1


def test_within_is_strict_and_widened():
    T = np.eye(4, dtype=F)
    s = np.zeros((3, 3), F)
    t = np.array([[0.5, 0, 0], [0.4999999, 0, 0], [np.nan, 0, 0]], F)      # |d|^2 == 0.25 == thr^2 exactly for the first pair
    assert ref.within(T, s, t, 0.5).tolist() == [False, True, False]


def test_the_loops_k_by_hand():
    # n = 10: counts 3, 5, 10 -> k = log(0.01) / log(1 - w^3) = 168.2, 34.49, log(0.01) / log(eps) = 0.128: stops after the third
    k1 = math.log(0.01) / math.log(1 - 0.3 ** 3)
    k2 = math.log(0.01) / math.log(1 - 0.5 ** 3)
    assert 168 < k1 < 169 and 34 < k2 < 35
    assert plane_ref.replay_loop([3, 5, 10, 10], 10, 1000, 0.99) == (2, 3)
    assert plane_ref.replay_loop([3, 2, 3, 1], 10, 1000, 0.99) == (0, 4)       # the counts run out (an empty selection): first of equals
    assert plane_ref.replay_loop([3] * 50, 1000, 5, 0.99) == (0, 6)            # iterations_ > max_iterations ends it
    assert plane_ref.replay_loop([0], 10, 1000, 0.99) == (0, 1)                # a hypothesis without inliers is a model


def test_reject_on_exact_matches_stops_at_once_and_recovers_the_pose():
    rng = np.random.default_rng(6)
    T = rigid()
    s = rng.uniform(-0.2, 0.2, (40, 3)).astype(F)
    t = (s.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    perm = rng.permutation(40)
    out = ref.reject(s, t[perm], np.arange(40), np.argsort(perm), inlier_threshold=0.01, max_iterations=100)
    assert out["found"] and out["best"] == 0 and out["iterations"] == 1 and out["counts"][0] == 40
    np.testing.assert_array_equal(out["inlier_pos"], np.arange(40))
    assert len(out["samples"]) == 101
    np.testing.assert_allclose(out["T_best"], T, atol=5e-6)


def test_reject_drops_wrong_matches():
    rng = np.random.default_rng(8)
    T = rigid()
    s = rng.uniform(-0.2, 0.2, (60, 3)).astype(F)
    t = (s.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    ti = np.arange(60)
    ti[:20] = (ti[:20] + 30) % 60                                          # a third of the matches are wrong
    out = ref.coarse_pose(s, np.zeros((0, 33), F), t, np.zeros((0, 33), F)) # no features: no matches, no model
    assert not out["found"] and len(out["inlier_pos"]) == 0 and np.array_equal(out["T_svd"], np.eye(4))
    out = ref.reject(s, t, np.arange(60), ti, inlier_threshold=0.005, max_iterations=500)
    assert out["found"]
    np.testing.assert_array_equal(out["inlier_pos"], np.arange(20, 60))
    assert 1 < out["iterations"] < 500
    pose = ref.svd_pose(s[out["inlier_pos"]], t[ti[out["inlier_pos"]]])
    np.testing.assert_allclose(pose, T, atol=1e-6)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_fewer_than_three_matches_is_no_model(n):
    s = np.random.default_rng(1).uniform(-1, 1, (5, 3)).astype(F)
    out = ref.reject(s, s, np.arange(n), np.arange(n))
    assert not out["found"] and out["best"] == -1 and out["iterations"] == 0 and len(out["samples"]) == 0
    np.testing.assert_array_equal(out["inlier_pos"], np.arange(n))         # remaining = original
    np.testing.assert_array_equal(out["T_best"], np.eye(4, dtype=F))


def test_coincident_source_points_run_the_draws_dry():
    s = np.tile(np.array([[0.1, 0.2, 0.3]], F), (6, 1))
    t = np.random.default_rng(1).uniform(-1, 1, (6, 3)).astype(F)
    out = ref.reject(s, t, np.arange(6), np.arange(6), max_iterations=10)
    assert not 0.0 > out["thresh"] and len(out["samples"]) == 0            # (0, or NaN: no edge of length 0 is above either)
    assert not out["found"] and out["iterations"] == 0
    np.testing.assert_array_equal(out["inlier_pos"], np.arange(6))
