"""ope_sacia and the batch's SAC-IA against tests/sacia_ref.py (numpy, float64), hypothesis by hypothesis.

The call returns the winner only, so a hypothesis is looked at through max_iterations = 1 with forced samples, and the draws
through prefixes: the stream is sequential, so a run of h hypotheses must return the reference's winner among the first h.  The
fit is compared with the reference's fit; the score with the reference's score OF THE TRANSFORM THE DEVICE RETURNED, within the
bound sacia_ref.error derives for a float32 evaluation.  The inputs are sacia_cases.py's; what these tests take for granted about
them (few ill-conditioned fits, no close call between hypotheses, draws that hit a NaN row) is asserted in test_sacia_ref.py,
without a GPU, and again here where a test leans on it.
"""
import os

import numpy as np
import pytest

import sacia_cases as cases
import sacia_ref as ref
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = float(np.finfo(F32).eps)
THR = cases.THR


@pytest.fixture(scope="module")
def ctx():
    ope = load_pkg()
    c = ope.Context(0)
    yield c
    c.close()


class Pair:
    """A source and a target on the device."""

    def __init__(self, ctx, src, tgt, sf=None, tf=None):
        self.ctx, self.src, self.tgt = ctx, np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.sf = np.zeros((len(src), 33), F32) if sf is None else sf
        self.tf = np.zeros((len(tgt), 33), F32) if tf is None else tf
        self.cs, self.ct = ctx.upload(self.src), ctx.upload(self.tgt)
        self.ix = ctx.build_index(self.ct)

    def forced(self, samp, corr, thr=THR):
        """The hypotheses (samp[h], corr[h]) and no others: (T, error, iteration) of the winner."""
        samp, corr = np.atleast_2d(samp), np.atleast_2d(corr)
        p = load_pkg().default_sacia_params(max_iterations=len(samp), nr_samples=samp.shape[1], k_correspondences=1, max_corr_dist=thr)
        return self.ctx.sacia(self.cs, self.sf, self.ct, self.ix, self.tf, p, forced_samples=np.r_[samp.ravel(), corr.ravel()])

    def seeded(self, h, S, K, seed, thr=THR, msd=0.01):
        p = load_pkg().default_sacia_params(max_iterations=h, nr_samples=S, k_correspondences=K, max_corr_dist=thr,
                                            min_sample_dist=msd, seed=seed)
        return self.ctx.sacia(self.cs, self.sf, self.ct, self.ix, self.tf, p)


def transform_tolerance(T_ref):
    """Device and reference both fit in float64 and round to float32, so an element differs by one float32 rounding of a value that
    is at most max(1, |t|): half an epsilon of it.  Measured on the MI355X, the largest element of device minus reference over every
    well-conditioned hypothesis of this file (158 forced ones, every prefix winner, the batch's four): 0.0, the host fit and numpy's
    SVD round to the same float32 (|t| up to 0.6).  Allowed: 4 epsilon of max(1, |t|) = 4.8e-7, eight times what one rounding
    explains, for fits whose conditioning (down to 1e-3) multiplies the float64 difference of the two decompositions."""
    return 4 * EPS * max(1.0, float(np.abs(np.asarray(T_ref, np.float64)[:3, 3]).max()))


def assert_transform(T, T_ref, what):
    d = float(np.abs(T.astype(np.float64) - np.asarray(T_ref, np.float64)).max())
    print(f"[sacia] {what}: |T - T_ref|_max = {d:.3e} (allowed {transform_tolerance(T_ref):.3e})")
    assert d <= transform_tolerance(T_ref), (what, d)
    return d


def assert_error(pair, T, err, what, extra=0.0):
    """The device's error against the reference's error of the same float32 transform, within the reference's bound (derived in
    sacia_ref.error, not measured; on the MI355X the difference came to at most 4.3 % of it, 1.2e-4 of 0.134 at 262 144 points)."""
    e, b = ref.error(pair.src, pair.tgt, T, THR)
    print(f"[sacia] {what}: error {err!r}, reference {e!r}, |difference| {abs(err - e):.3e}, bound {b + extra:.3e}")
    assert abs(err - e) <= b + extra, (what, err, e, b + extra)
    return e


@pytest.fixture(scope="module")
def copy_pair(ctx):
    src, sf, tgt, tf = cases.partial_copy()
    return Pair(ctx, src, tgt, sf, tf)


# ------------------------------------------------------------------ every hypothesis, not the winner
@pytest.mark.parametrize("S,K,seed", cases.PER_HYPOTHESIS)
def test_every_hypothesis_fit_and_score(copy_pair, S, K, seed):
    out = cases.reference_run(S, K, seed)
    ex = cases.exempt(copy_pair.src, copy_pair.tgt, out["samples"], out["targets"])
    assert ex.sum() <= 0.02 * cases.H * len(cases.PER_HYPOTHESIS)      # over all four cases: test_sacia_ref.py
    worst = 0.0
    for h in range(cases.H):
        T, err, it = copy_pair.forced(out["samples"][h], out["targets"][h])
        assert it == 0
        if not ex[h]:
            d = float(np.abs(T.astype(np.float64) - out["T"][h]).max())
            worst = max(worst, d)
            assert d <= transform_tolerance(out["T"][h]), (h, d)         # measured 0, allowed 4 eps max(1, |t|): see there
        e, b = ref.error(copy_pair.src, copy_pair.tgt, T, THR)
        assert abs(err - e) <= b, (h, err, e, b)                         # the derived bound: see assert_error
    print(f"[sacia] S={S} K={K}: largest |T - T_ref| over {int((~ex).sum())} hypotheses {worst:.3e}")


# ------------------------------------------------------------------ the draws, through prefixes
def assert_prefixes(pair, out, S, K, seed, H, what):
    for h in range(1, H + 1):
        T, err, it = pair.seeded(h, S, K, seed)
        w = ref.scan(out["error"][:h])
        assert it == w, (what, h, it, w)
        assert_transform(T, out["T"][w], f"{what} prefix {h}")
        assert_error(pair, T, err, f"{what} prefix {h}")


@pytest.mark.parametrize("S,K,seed", cases.PREFIXES)
def test_every_prefix_of_a_seeded_run_has_the_reference_winner(copy_pair, S, K, seed):
    out = cases.reference_run(S, K, seed)
    assert cases.close_calls(out["error"], out["bound"]) == []
    assert_prefixes(copy_pair, out, S, K, seed, cases.H, f"S={S} K={K}")


# ------------------------------------------------------------------ narrow clouds
@pytest.mark.parametrize("name", ["ball", "duplicates", "ns_equals_S"])
def test_narrow_clouds(ctx, name):
    """A 5 mm ball under min_sample_dist 0.01 (every hypothesis halves the distance, and starts from 0.01 again), duplicate points
    (rejected by distance 0, and equal descriptors: ties in findSimilarFeatures), and ns == S (only the already-drawn rule ends)."""
    src, sf, tgt, tf, S, K, H, seed = cases.narrow_cases()[name]
    out = cases.narrow_runs()[name]
    assert cases.close_calls(out["error"], out["bound"]) == []
    assert_prefixes(Pair(ctx, src, tgt, sf, tf), out, S, K, seed, H, name)


# ------------------------------------------------------------------ the threshold quirk
def test_squared_distance_against_the_unsquared_threshold(ctx):
    """Every source point 0.1 from its nearest target point, thr = 0.05: d^2 = 0.01 <= thr < d, every term 0.01 / 0.05 = 0.2.  A
    squared threshold (0.0025) or a rooted distance (0.1) would make every term 1.

    The target is the source shifted by 0.1 along x: a grid of 0.3, so that a point's own copy is its nearest.  The identity comes
    from four more points, far out on the x and y axes, each paired with its own copy; for these the shift is not along x but
    outward, 0.1 each, so their shifts cancel (no translation, no torque) and the fit is the identity while they too sit 0.1 from
    their nearest."""
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.3 - 1.05
    anchors = np.array([[5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0]], np.float64)
    src = np.concatenate([g, anchors]).astype(F32)
    tgt = np.concatenate([g + [0.1, 0, 0], anchors * (5.1 / 5.0)]).astype(F32)
    pair = Pair(ctx, src, tgt)
    a = np.arange(len(g), len(g) + 4)
    T, err, it = pair.forced(a, a)
    assert_transform(T, np.eye(4), "threshold quirk")
    term, _ = ref.terms(src, tgt, T, THR)
    assert np.abs(term - 0.2).max() < 1e-5, np.abs(term - 0.2).max()      # float32 rounding of the shifted coordinates: 4e-7 of 0.2
    e = assert_error(pair, T, err, "threshold quirk")
    assert abs(e - 0.2 * len(src)) < 1e-5 * len(src) and abs(err - 0.2 * len(src)) < 1e-5 * len(src)


# ------------------------------------------------------------------ past the launch cap
@pytest.fixture(scope="module")
def big_source():
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-0.15, 0.15, (64, 3)).astype(F32)
    near = rng.uniform(-0.3, 0.3, (262144, 3)).astype(F32)             # d^2 to the nearest of 64 on either side of thr
    near[:6] = tgt[:6]                                                 # the samples: copies of target points
    far = (rng.uniform(-0.3, 0.3, (257, 3)) + [40.0, -30.0, 20.0]).astype(F32)
    return tgt, near, far


@pytest.mark.parametrize("n", [262144, 262145, 262144 + 257])
def test_past_the_launch_cap(ctx, big_source, n):
    """The launch is at most 1024 blocks of 256 lanes: 262 144 lanes.  At n = 262 144 every lane takes one point and adds nothing in
    float32; at 262 145 one lane, and at 262 144 + 257 each of 257 lanes, takes two points and adds two terms in float32 (one
    rounding of a sum of at most 2, which accumulation_bound adds to the bound).  The last 257 points of the source lie 54 m from
    the target and score 1 each.  A kernel that dropped its grid stride would lose every lane's second point, each of them a
    term: n - 262 144 too little."""
    tgt, near, far = big_source
    src = np.concatenate([near[:n - len(far)], far])                    # the last 257 far from the target, for every n
    pair = Pair(ctx, src, tgt)
    lanes = 1024 * 256
    per_lane = np.bincount(np.arange(n) % lanes, minlength=lanes)       # n_valid = n: lane l takes points l, l + lanes, ...
    assert per_lane.max() == (1 if n == lanes else 2) and (per_lane == 2).sum() == n - lanes
    acc = ref.accumulation_bound(per_lane)
    assert acc == (n - lanes) * 2 * ref.U32
    samp = np.array([[0, 1, 2], [3, 4, 5]])
    corr = np.array([[0, 1, 2], [5, 3, 4]])                             # the identity, and a wrong pairing
    errs, refs = [], []
    for h in range(2):                                                  # each alone: its own score
        T, err, it = pair.forced(samp[h], corr[h])
        assert_transform(T, ref.fit(src[samp[h]], tgt[corr[h]]), f"n={n} hypothesis {h}")
        e = assert_error(pair, T, err, f"n={n} hypothesis {h}", extra=acc)
        term, _ = ref.terms(src[-len(far):], tgt, T, THR)
        assert (term == 1).all() and len(far) + 1000 < e < n - 1000     # the far points on top of a sum of fractions
        errs.append(err)
        refs.append(e)
    assert abs(refs[0] - refs[1]) > 1.0                                 # no close call (an ulp of the float32 the scan compares: 0.016)
    w = int(refs[1] < refs[0])
    for order in ([0, 1], [1, 0]):                                      # H = 2 (grid.y = 2), either order
        T, err, it = pair.forced(samp[order], corr[order])
        assert it == order.index(w) and err == errs[w], (order, it, err, errs)
        assert_transform(T, ref.fit(src[samp[w]], tgt[corr[w]]), f"n={n} H=2")


# ------------------------------------------------------------------ first of equals
def test_first_of_equal_hypotheses_wins(copy_pair):
    out = cases.reference_run(5, 5, 33)
    best = out["best_iteration"]
    order = [h for h in range(12) if h != best][:10]
    order[3] = order[7] = best                                          # the same sample set twice: equal errors, bit for bit
    samp, corr = out["samples"][order], out["targets"][order]
    assert ref.scan(out["error"][order]) == 3
    T, err, it = copy_pair.forced(samp, corr)
    assert it == 3                                                      # "<" keeps the first; "<=" would return 7
    assert_transform(T, out["T"][best], "first of equals")
    assert_error(copy_pair, T, err, "first of equals")


# ------------------------------------------------------------------ non-finite points
def test_non_finite_source_points_score_one_each(ctx, copy_pair):
    out = cases.reference_run(5, 5, 33)
    h = out["best_iteration"]
    samp, corr = out["samples"][h], out["targets"][h]
    src = copy_pair.src.copy()
    free = np.setdiff1d(np.arange(len(src)), samp)
    bad = free[[3, 77, 200, 310, 555, 580, 594]]
    src[bad[:3]] = np.nan
    src[bad[3:5], 0] = np.inf
    src[bad[5:], 2] = -np.inf
    pair = Pair(ctx, src, copy_pair.tgt)
    T, err, it = pair.forced(samp, corr)
    assert_transform(T, out["T"][h], "non-finite source")
    e = assert_error(pair, T, err, "non-finite source")
    # the same hypothesis without those points scores their count less
    keep = np.setdiff1d(np.arange(len(src)), bad)
    e_without, b = ref.error(src[keep], copy_pair.tgt, T, THR)
    assert abs(err - (e_without + len(bad))) <= b


def test_non_finite_target_points_are_never_matched(ctx, copy_pair):
    out = cases.reference_run(5, 5, 33)
    h = out["best_iteration"]
    junk = np.array([[np.nan, 0, 0], [0, np.inf, 0], [np.nan] * 3, [0, 0, -np.inf]], F32)
    tgt = np.concatenate([copy_pair.tgt[:100], junk, copy_pair.tgt[100:]])
    corr = np.where(out["targets"][h] >= 100, out["targets"][h] + len(junk), out["targets"][h])
    pair = Pair(ctx, copy_pair.src, tgt)
    T, err, it = pair.forced(out["samples"][h], corr)
    assert_transform(T, out["T"][h], "non-finite target")
    e = assert_error(pair, T, err, "non-finite target")
    e_clean, b = ref.error(copy_pair.src, copy_pair.tgt, T, THR)
    assert abs(err - e_clean) <= b and e == e_clean                      # as if they were not there


# ------------------------------------------------------------------ too few target descriptors
@pytest.mark.parametrize("name", ["nt_3_K_5", "nan_rows_K_8"])
def test_a_pick_on_an_empty_place_takes_the_first(ctx, name):
    """Fewer target descriptors (that are not NaN) than K: the k-NN row has empty places, a pick on one takes row[0].  Hypothesis 0
    of eight seeds whose picks do land on an empty place: the transform shows which correspondences were taken."""
    case = cases.few_target_cases()[name]
    src, sf, tgt, tf, S, K = case
    seeds = cases.fallback_seeds(case)
    assert len(seeds) == 8
    pair = Pair(ctx, src, tgt, sf, tf)
    for seed, samp, corr in seeds:
        T, err, it = pair.seeded(1, S, K, seed)
        assert it == 0
        assert_transform(T, ref.fit(src[samp], tgt[corr]), f"{name} seed {seed}")
        assert_error(pair, T, err, f"{name} seed {seed}")


# ------------------------------------------------------------------ NaN descriptor rows in the source
def test_a_sample_with_a_nan_descriptor_makes_a_void_hypothesis_not_an_error(ctx):
    """ope_fpfh writes NaN rows for non-finite points, and the draws run over all points: a hypothesis that draws one has no
    correspondence for it.  It is void: it scores |source|, its transform is the identity, and the run goes on.  (Before this test
    ope_sacia returned OPE_EINVAL "sample index out of range" for such an input.)"""
    src, sf, tgt, tf, bad = cases.nan_source()
    out = cases.nan_run()
    assert out["void"][0] and 5 <= out["void"].sum() < cases.H and not out["void"][out["best_iteration"]]
    assert cases.close_calls(out["error"], out["bound"]) == []
    pair = Pair(ctx, src, tgt, sf, tf)
    for h in range(1, cases.H + 1):
        T, err, it = pair.seeded(h, cases.NAN_S, cases.NAN_K, cases.NAN_SEED)
        w = ref.scan(out["error"][:h])
        assert it == w, (h, it, w)
        assert np.isfinite(T).all()
        if out["void"][w]:
            assert np.array_equal(T, np.eye(4, dtype=F32)) and err == len(src), (h, err)
        else:
            assert_transform(T, out["T"][w], f"nan rows prefix {h}")
            assert_error(pair, T, err, f"nan rows prefix {h}")
    # nothing but void hypotheses: hypothesis 0 stays
    T, err, it = Pair(ctx, src, tgt, np.full_like(sf, np.nan), tf).seeded(5, 3, 2, 4)
    assert it == 0 and err == len(src) and np.array_equal(T, np.eye(4, dtype=F32))
    # a non-finite sample with a descriptor that does match: the fit is not finite, void all the same
    k = int(bad[0])
    finite = np.flatnonzero(np.isfinite(src).all(1))[:2]
    T, err, it = pair.forced([[k, finite[0], finite[1]]], [[0, 1, 2]])
    assert it == 0 and err == len(src) and np.array_equal(T, np.eye(4, dtype=F32))


# ------------------------------------------------------------------ the batch
def test_the_batch_matches_the_reference_on_its_own_features(ctx):
    """ope_coarse_pose_batch on the four-cluster fixture of test_gpu_coarse_batch.py, cut down to every third point and 40
    hypotheses: each cluster's key points and descriptors as the batch computed them, through sacia_ref.run with the cluster's
    seed.  coarse_sacia_error_kernel (brute force from LDS, double sums) against the numpy score."""
    from test_gpu_coarse_batch import raw_candidates, with_nans
    ope = load_pkg()
    pcd = __import__("importlib").import_module("object-pose-estimation_amd.pcd")
    model = np.ascontiguousarray(pcd.read_pcd(os.path.join(ROOT, "tests", "golden", "drill_model_decimated.pcd"))[0], F32)
    clouds = raw_candidates(3, scene_at=1) + [with_nans(raw_candidates(4, scene_at=0, seed=3)[3], 11)]
    clouds = [np.ascontiguousarray(c[::3]) for c in clouds]
    H = 40
    seeds = [1, 2, 3, 4]
    p = ope.default_coarse_params(sacia=ope.default_sacia_params(max_iterations=H))
    res = ctx.coarse_pose_batch(ctx.upload(model), [ctx.upload(c) for c in clouds], p, seeds=seeds)
    midx, _, mf = ctx.coarse_batch_features(-1)
    mk = model[midx]
    for i, (cloud, r) in enumerate(zip(clouds, res)):
        tidx, _, tf = ctx.coarse_batch_features(i)
        tk = cloud[tidx]
        assert r.status == 0 and r.n_src_keys == len(mk) and r.n_tgt_keys == len(tk)
        out = ref.run(mk, mf, tk, tf, max_iterations=H, nr_samples=5, k_correspondences=5, max_corr_dist=0.05, min_sample_dist=0.01,
                      seed=seeds[i])
        close = cases.close_calls(out["error"], out["bound"])
        print(f"[sacia batch] cluster {i}: {len(mk)} x {len(tk)} key points, winner {r.best_iteration} (reference "
              f"{out['best_iteration']}), close calls {[c for c in close if c[0] == H]}")
        assert [c for c in close if c[0] == H] == [], (i, close)
        b = out["best_iteration"]
        assert not cases.exempt(mk, tk, out["samples"][b:b + 1], out["targets"][b:b + 1])[0]
        assert r.best_iteration == b, (i, r.best_iteration, b)
        assert_transform(r.T, out["T_best"], f"batch cluster {i}")
        e, bound = ref.error(mk, tk, r.T, 0.05)
        print(f"[sacia batch] cluster {i}: error {r.best_error!r}, reference {e!r}, bound {bound:.3e}")
        assert abs(r.best_error - e) <= bound, (i, r.best_error, e, bound)
