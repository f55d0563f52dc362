"""tests/sacia_ref.py pinned on its own, without the device: answers worked out by hand for every rule, then agreement with the C
oracle on ordinary inputs, so that the two references check each other before either judges a kernel.  Last, what
test_gpu_sacia.py takes for granted about its inputs (sacia_cases.py) is checked here, on the CPU."""
import numpy as np
import pytest

import oracle
import prerejective_ref
import sacia_cases as cases
import sacia_ref as ref

F32 = np.float32


class Scripted:
    """Stands in for the LCG: next() hands out the given numbers and fails when they run out."""

    def __init__(self, values):
        self.values, self.used = list(values), 0

    def next(self):
        v = self.values[self.used]
        self.used += 1
        return v


def scripted(monkeypatch, values):
    s = Scripted(values)
    monkeypatch.setattr(ref, "Lcg", lambda seed: s)
    return s


def idx(i, n=3):
    """A number in [0, 1) that int(n * .) turns into i."""
    return (i + 0.5) / n


# ------------------------------------------------------------------ draws
THREE = np.array([[0, 0, 0], [0.004, 0, 0], [1, 0, 0]], F32)     # points 0 and 1 are 4 mm apart: 0.01 -> 0.005 -> 0.0025 admits them


def test_draws_halve_after_3ns_rejections_restart_by_value_and_take_every_point_when_ns_is_S(monkeypatch):
    # ns = S = 3, min distance 0.01, 3 * ns = 9 rejections in a row halve it.
    h0 = ([idx(0)]                 # 0 accepted
          + [idx(0)]               # 0 again: already drawn, rejection 1
          + [idx(1)] * 8           # 1 is 0.004 from 0, < 0.01: rejections 2..9, the 9th halves to 0.005
          + [idx(1)] * 9           # 0.004 < 0.005: 9 more, halved to 0.0025
          + [idx(1)]               # 0.004 >= 0.0025: accepted
          + [idx(2)]               # 1 m away: accepted
          + [0.3, 0.8, 0.0])       # picks int(4 * .) = 1, 3, 0
    h1 = ([idx(1)]                 # accepted
          + [idx(0)]               # the distance is 0.01 again, not the 0.0025 hypothesis 0 ended with: rejection 1
          + [idx(2)]               # accepted; the count of rejections starts again
          + [idx(0)] * 18          # two halvings
          + [idx(0)]               # accepted
          + [0.99, 0.5, 0.25])     # picks 3, 2, 1
    s = scripted(monkeypatch, h0 + h1)
    samp, pick = ref.draws(THREE, 3, 4, 2, 0.01, seed=0)
    assert samp.tolist() == [[0, 1, 2], [1, 2, 0]]
    assert pick.tolist() == [[1, 3, 0], [3, 2, 1]]
    assert s.used == len(h0) + len(h1)          # one rejection fewer or more before a halving would leave numbers over or run out


def test_draws_distance_is_float32(monkeypatch):
    # |p| is 0.009999999737 in float64, below float32(0.01) = 0.009999999776, but sqrt((x x + y y) + z z) in float32 is that
    # float32(0.01) exactly: not closer than the minimum distance, so p is accepted at once (the numbers would run out otherwise)
    p = np.array([float.fromhex("0x1.a3fde8p-10"), float.fromhex("-0x1.0c15ap-7"), float.fromhex("0x1.69eeacp-8")], F32)
    assert np.linalg.norm(p.astype(np.float64)) < float(F32(0.01))
    s = scripted(monkeypatch, [idx(0, 2), idx(1, 2), 0.0, 0.0])
    samp, _ = ref.draws(np.stack([np.zeros(3, F32), p]), 2, 1, 1, 0.01, seed=0)
    assert samp.tolist() == [[0, 1]] and s.used == 4


def test_draws_accept_a_non_finite_point_and_what_follows_it(monkeypatch):
    # a NaN distance is not "closer": the NaN point is accepted, and so is the next point, compared with it
    xyz = np.array([[np.nan, 0, 0], [0, 0, 0], [1, 0, 0]], F32)
    scripted(monkeypatch, [idx(0), idx(1), idx(2), 0, 0, 0])
    samp, _ = ref.draws(xyz, 3, 1, 1, 0.01, seed=0)
    assert samp.tolist() == [[0, 1, 2]]


def test_draws_on_the_real_stream():
    # with no minimum distance only the already-drawn rule is left: the stream of prerejective_ref.draws
    xyz = np.random.default_rng(1).uniform(-1, 1, (7, 3)).astype(F32)
    samp, pick = ref.draws(xyz, 3, 5, 200, 0.0, seed=3)
    s0, p0 = prerejective_ref.draws(7, 3, 5, 200, seed=3)
    np.testing.assert_array_equal(samp, s0)
    np.testing.assert_array_equal(pick, p0)
    # the first number of seed 1, by hand: x1 = a + c (mod 2^64), (x1 >> 11) / 2^53 = 0.4232..., int(7 * .) = 2
    x1 = (6364136223846793005 + 1442695040888963407) % 2 ** 64
    assert ref.draws(xyz, 1, 1, 1, 0.0, seed=1)[0][0, 0] == int(7 * ((x1 >> 11) / 2.0 ** 53))


# ------------------------------------------------------------------ feature_knn, correspondences
def test_feature_knn_ties_nan_rows_and_short_targets():
    zeros = np.zeros((6, 33), F32)
    assert ref.feature_knn(zeros, np.zeros(33, F32), 4).tolist() == [0, 1, 2, 3]        # all distances equal: the lower index
    with_nan = zeros.copy()
    with_nan[1, 7] = np.nan
    assert ref.feature_knn(with_nan, np.zeros(33, F32), 4).tolist() == [0, 2, 3, 4]     # a NaN row never matches
    assert ref.feature_knn(zeros[:3], np.zeros(33, F32), 5).tolist() == [0, 1, 2, -1, -1]   # k > nt
    q = np.zeros(33, F32)
    q[0] = np.nan
    assert ref.feature_knn(zeros, q, 3).tolist() == [-1, -1, -1]                        # a NaN query matches nothing
    near = zeros.copy()
    near[:, 0] = [5, 3, 1, 3, 0, 9]                                                     # distances 25 9 1 9 0 81
    assert ref.feature_knn(near, np.zeros((2, 33), F32), 4).tolist() == [[4, 2, 1, 3]] * 2


def test_feature_knn_sums_in_float32_in_bin_order():
    a = np.zeros((3, 33), F32)
    a[0, 0], a[0, 1], a[0, 2] = 4096, 1, 1          # (2^24 + 1) + 1: each 1 is lost in float32, 2^24
    a[1, 0] = 4096                                  # 2^24
    a[2, 0], a[2, 1], a[2, 2] = 1, 1, 4096          # (1 + 1) + 2^24 = 2^24 + 2, exact in float32
    # float64 would order 1, 0 = 2; float32 in another order of the bins would not separate 2 from 0
    assert ref.feature_knn(a, np.zeros(33, F32), 3).tolist() == [0, 1, 2]
    assert ref.feature_knn(a[::-1], np.zeros(33, F32), 3).tolist() == [1, 2, 0]


def test_correspondences_fall_back_to_the_first_place():
    nn = np.array([[4, 2, -1], [-1, -1, -1], [7, 8, 9]], np.int32)
    samp = np.array([[0, 0, 2], [1, 2, 0]])
    pick = np.array([[1, 2, 2], [2, 0, 0]])
    assert ref.correspondences(samp, pick, nn).tolist() == [[2, 4, 9], [-1, 7, 4]]


# ------------------------------------------------------------------ fit
def test_fit_recovers_a_pose_and_is_a_rotation_below_full_rank():
    T = cases.pose()
    rng = np.random.default_rng(2)
    for pts in (rng.uniform(-1, 1, (5, 3)), rng.uniform(-1, 1, (3, 3))):                # full rank, then coplanar (rank 2)
        out = ref.fit(pts, pts @ T[:3, :3].T + T[:3, 3])
        np.testing.assert_allclose(out, T, atol=2e-7)
    line = np.outer(np.arange(4.0), [1.0, 2.0, -1.0])                                   # collinear: rank 1
    out = ref.fit(line, line @ T[:3, :3].T + T[:3, 3]).astype(np.float64)
    assert abs(np.linalg.det(out[:3, :3]) - 1) < 1e-6
    np.testing.assert_allclose(line @ out[:3, :3].T + out[:3, 3], line @ T[:3, :3].T + T[:3, 3], atol=1e-6)
    mirror = rng.uniform(-1, 1, (5, 3))                                                 # a mirrored copy: still det +1
    out = ref.fit(mirror, mirror * [1, 1, -1]).astype(np.float64)
    assert abs(np.linalg.det(out[:3, :3]) - 1) < 1e-6
    assert np.isnan(ref.fit(np.array([[np.nan, 0, 0], [0, 1, 0], [1, 0, 0]]), np.eye(3))).any()


# ------------------------------------------------------------------ error, scan
def test_error_divides_the_squared_distance_by_the_unsquared_threshold():
    src = np.array([[0.25, 0, 0]], F32)
    tgt = np.array([[0.25, 0.1, 0], [9, 9, 9]], F32)            # d = 0.1: d^2 = 0.01 <= 0.05 < d
    e, b = ref.error(src, tgt, np.eye(4, dtype=F32), 0.05)
    assert e == pytest.approx(0.2, abs=1e-6) and 0 < b < 1e-5    # not 1 (d against thr) and not 1 either (d^2 against thr^2)
    e, _ = ref.error(src, tgt + F32(0.25), np.eye(4, dtype=F32), 0.05)
    assert e == 1.0
    T = np.eye(4, dtype=F32)
    T[1, 3] = 0.1                                               # the transform is applied: the point lands on the target
    assert ref.error(src, tgt, T, 0.05)[0] == pytest.approx(0.0, abs=1e-12)


def test_error_counts_non_finite_source_points_and_never_matches_a_non_finite_target():
    src = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0.1]], F32)
    tgt = np.array([[0, 0, 0], [0, 0, np.nan], [np.inf, 0, 0.1]], F32)
    term, bound = ref.terms(src, tgt, np.eye(4, dtype=F32), 0.05)
    np.testing.assert_allclose(term, [0, 1, 1, 0.2], atol=1e-6)
    assert bound[1] == bound[2] == 0
    assert ref.error(src, tgt[1:], np.eye(4, dtype=F32), 0.05) == (4.0, 0.0)            # no finite target point at all


def test_scan_is_strict_in_float32_and_the_first_of_equals_wins():
    assert ref.scan([5.0, 3.0, 3.0, 4.0, 3.0]) == 1
    assert ref.scan([2.0, 2.0]) == 0
    assert ref.scan([300.0, 300.0 - 1e-6]) == 0          # equal as float32 (an ulp of 300 is 3e-5): no change
    assert ref.scan([300.0, 300.0 - 1e-4]) == 1
    assert ref.scan([7.0]) == 0


# ------------------------------------------------------------------ against the oracle
def test_feature_knn_agrees_with_the_oracle():
    rng = np.random.default_rng(9)
    tf = rng.uniform(0, 100, (200, 33)).astype(F32)
    tf[50:60] = tf[10:20]                                        # ties
    tf[100] = np.nan
    q = np.concatenate([tf[5:15] + F32(0.5), rng.uniform(0, 100, (10, 33)).astype(F32)])
    for k in (1, 5, 8):
        np.testing.assert_array_equal(ref.feature_knn(tf, q, k), oracle.feature_knn(tf, q, k)[0])
    np.testing.assert_array_equal(ref.feature_knn(tf[:3], q, 5), oracle.feature_knn(tf[:3], q, 5)[0])


@pytest.mark.parametrize("S,K,seed", cases.PER_HYPOTHESIS + cases.PREFIXES)
def test_runs_agree_with_the_oracle(S, K, seed):
    src, sf, tgt, tf = cases.partial_copy()
    out = cases.reference_run(S, K, seed)
    n = len(src)
    tree = oracle.KdTree(tgt)
    for h in range(cases.H):
        # the oracle sums its terms in float32, one after the other: n - 1 roundings of a partial sum that is at most the error
        e = oracle.sacia_error(src, tree, out["T"][h], cases.THR)
        assert abs(e - out["error"][h]) <= out["bound"][h] + (n - 1) * ref.U32 * out["error"][h] + 1e-12, (h, e, out["error"][h])
        if not cases.exempt(src, tgt, out["samples"][h:h + 1], out["targets"][h:h + 1])[0]:
            # the oracle's fit accumulates in float32 (PCL's): 3e-6 measured, against translations of 0.3
            assert np.abs(oracle.umeyama(src[out["samples"][h]], tgt[out["targets"][h]]) - out["T"][h]).max() < 1e-5, h
    if not cases.close_calls(out["error"], out["bound"]):
        T, e, best = oracle.sacia(src, sf, tgt, tf, n_iter=cases.H, nr_samples=S, k_corr=K, max_corr_dist=cases.THR, seed=seed)
        assert best == out["best_iteration"]
        assert np.abs(T - out["T_best"]).max() < 1e-5
        assert abs(e - out["best_error"]) <= out["bound"][best] + n * ref.U32 * e


def test_void_hypotheses_agree_with_the_oracle():
    src, sf, tgt, tf, _ = cases.nan_source()
    out = cases.nan_run()
    T, e, best = oracle.sacia(src, sf, tgt, tf, n_iter=cases.H, nr_samples=cases.NAN_S, k_corr=cases.NAN_K, max_corr_dist=cases.THR,
                              seed=cases.NAN_SEED)
    assert best == out["best_iteration"] and np.abs(T - out["T_best"]).max() < 1e-5
    assert abs(e - out["best_error"]) <= out["bound"][best] + len(src) * ref.U32 * e
    # all hypotheses void: hypothesis 0 stays, the identity, |source|
    sf_all = np.full_like(sf, np.nan)
    o = ref.run(src, sf_all, tgt, tf, max_iterations=5, nr_samples=3, k_correspondences=2, seed=4)
    T, e, best = oracle.sacia(src, sf_all, tgt, tf, n_iter=5, nr_samples=3, k_corr=2, seed=4)
    assert o["void"].all() and o["best_iteration"] == best == 0 and o["best_error"] == e == len(src)
    assert np.array_equal(o["T_best"], np.eye(4)) and np.array_equal(T, np.eye(4))


# ------------------------------------------------------------------ what the GPU tests take for granted
def test_few_fits_are_exempt_and_no_prefix_is_a_close_call():
    src, _, tgt, _ = cases.partial_copy()
    n_exempt = 0
    for S, K, seed in cases.PER_HYPOTHESIS:
        out = cases.reference_run(S, K, seed)
        n_exempt += int(cases.exempt(src, tgt, out["samples"], out["targets"]).sum())
    assert n_exempt <= 0.02 * cases.H * len(cases.PER_HYPOTHESIS), n_exempt
    for S, K, seed in cases.PREFIXES:
        out = cases.reference_run(S, K, seed)
        assert cases.close_calls(out["error"], out["bound"]) == []
        winners = {ref.scan(out["error"][:h]) for h in range(1, cases.H + 1)}
        assert len(winners) >= 4, winners                                         # the lead changes hands: the prefixes differ
        assert not cases.exempt(src, tgt, out["samples"], out["targets"])[sorted(winners)].any()


def test_narrow_clouds_halve_and_have_a_clear_winner():
    runs = cases.narrow_runs()
    for name, (src, sf, tgt, tf, S, K, h, seed) in cases.narrow_cases().items():
        out = runs[name]
        assert cases.close_calls(out["error"], out["bound"]) == [], name
        b = out["best_iteration"]
        assert not cases.exempt(src, tgt, out["samples"][b:b + 1], out["targets"][b:b + 1])[0], name
    src = cases.narrow_cases()["ball"][0]
    s = runs["ball"]["samples"]
    d = np.linalg.norm(src[s][:, :, None, :].astype(np.float64) - src[s][:, None, :, :], axis=-1)
    # every pair of samples is closer than half the distance, so every hypothesis halved it at least twice, each time from 0.01: a
    # run that kept the halved distance would spend 3 * ns fewer numbers of the stream per halving and draw other samples after it
    assert d.max() < 0.005
    five = cases.narrow_cases()["ns_equals_S"]
    assert len(five[0]) == five[4] and all(sorted(row) == list(range(5)) for row in runs["ns_equals_S"]["samples"].tolist())
    dup, _, dup_tgt, dup_f = cases.narrow_cases()["duplicates"][:4]
    assert len(np.unique(dup, axis=0)) == 200 and len(dup) == 300
    # the target rows of a duplicated point tie in descriptor distance but are different points: the tie rule decides a fit
    assert len(np.unique(dup_f, axis=0)) == 200 and len(np.unique(dup_tgt, axis=0)) == 300


def test_the_nan_case_draws_nan_rows():
    src, sf, tgt, tf, bad = cases.nan_source()
    out = cases.nan_run()
    hit = np.isin(out["samples"], bad).any(1)
    assert hit[0] and 5 <= hit.sum() < cases.H                    # hypothesis 0 among them: the scan starts from a void one
    np.testing.assert_array_equal(out["void"], hit)
    assert (out["error"][hit] == len(src)).all() and (out["targets"][np.isin(out["samples"], bad)] == -1).all()
    assert not out["void"][out["best_iteration"]]
    assert cases.close_calls(out["error"], out["bound"]) == []
