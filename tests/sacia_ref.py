"""pcl::SampleConsensusInitialAlignment restated in numpy, float64 wherever the rule does not say float32.

Written from PCL's rules, not from the kernels or the C oracle, so that a choice the three of them share can still be wrong here:
selectSamples, findSimilarFeatures, TransformationEstimationSVD (Umeyama without scale, by numpy.linalg.svd), computeErrorMetric
with TruncatedError, and the "lowest error so far" scan.  Nothing here calls the library.  test_sacia_ref.py pins this file on its
own (answers worked out by hand) and against the oracle.

Layout: a transform is (4, 4) in math layout (T[r, c]); forced samples are (2, H, S): source indices, then target indices.
"""
import numpy as np

from prerejective_ref import Lcg

F32 = np.float32
U32 = 2.0 ** -24          # unit round-off of float32 (half an ulp of 1)


# ------------------------------------------------------------------ selectSamples and the picks
def _dist32(a, b):
    """Euclidean distance of two float32 points, every operation in float32: sqrt((dx dx + dy dy) + dz dz)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(a, F32) - np.asarray(b, F32)
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def draws(xyz, S, K, H, min_sample_dist, seed):
    """(samp, pick), both (H, S) int32.  Per hypothesis: indices int(ns * next()) until S are accepted; an index is rejected if it
    was already drawn for this hypothesis or lies closer than the current minimum distance to an accepted one (a NaN distance is
    not closer).  3 * ns rejections in a row halve the distance; the distance is an argument passed by value, so the next
    hypothesis starts from min_sample_dist again.  Then S picks int(K * next()).  One stream for the whole run."""
    xyz = np.asarray(xyz, F32)
    ns = len(xyz)
    rng = Lcg(seed)
    samp = np.zeros((H, S), np.int32)
    pick = np.zeros((H, S), np.int32)
    for h in range(H):
        msd = F32(min_sample_dist)
        got, rejected = [], 0
        while len(got) < S:
            i = int(ns * rng.next())
            if i in got or any(_dist32(xyz[i], xyz[j]) < msd for j in got):
                rejected += 1
                if rejected >= 3 * ns:
                    msd = msd * F32(0.5)
                    rejected = 0
            else:
                got.append(i)
                rejected = 0
        samp[h] = got
        pick[h] = [int(K * rng.next()) for _ in range(S)]
    return samp, pick


# ------------------------------------------------------------------ findSimilarFeatures
def feature_knn(tgt_feat, q, k):
    """The k nearest target descriptors of q ((33,) -> (k,), or (m, 33) -> (m, k)), int32: squared L2 summed in float32 bin after
    bin; a NaN distance never matches; equal distances go to the lower index; places nothing fills hold -1."""
    tf = np.asarray(tgt_feat, F32).reshape(-1, 33)
    q = np.asarray(q, F32)
    if q.ndim == 1:
        return feature_knn(tf, q[None], k)[0]
    out = np.full((len(q), k), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, row in enumerate(q):
            d = np.zeros(len(tf), F32)
            for b in range(33):
                u = row[b] - tf[:, b]
                d = d + u * u
            ok = np.flatnonzero(~np.isnan(d))
            best = ok[np.lexsort((ok, d[ok]))][:k]          # by distance, then by index
            out[j, :len(best)] = best
    return out


def correspondences(samp, pick, nn):
    """nn: (n_src, K) rows of feature_knn by source index.  The target of a sample is row[pick], or row[0] where that place is
    empty (-1 when the whole row is)."""
    samp, pick = np.asarray(samp), np.asarray(pick)
    row = np.asarray(nn)[samp]                                   # (H, S, K)
    c = np.take_along_axis(row, pick[..., None].astype(np.int64), axis=-1)[..., 0]
    return np.where(c >= 0, c, row[..., 0]).astype(np.int32)


# ------------------------------------------------------------------ TransformationEstimationSVD
def fit(src_pts, tgt_pts):
    """Umeyama without scale in float64: R = U diag(1, 1, s) V^T of the cross-covariance, t = mean_t - R mean_s, cast to float32.
    s = sign(det U det V): with full rank that is the sign of the covariance's determinant (Umeyama's rule), and below it (coplanar or
    collinear samples) it is the rule the project adopted, a rotation all the same."""
    ps, pt = np.asarray(src_pts, np.float64), np.asarray(tgt_pts, np.float64)
    ms, mt = ps.mean(0), pt.mean(0)
    sigma = (pt - mt).T @ (ps - ms) / len(ps)
    T = np.eye(4)
    if not np.isfinite(sigma).all():
        T[:3] = np.nan
        return T.astype(F32)
    U, _, Vt = np.linalg.svd(sigma)
    s = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    R = U @ np.diag([1.0, 1.0, s]) @ Vt
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T.astype(F32)


def conditioning(pts):
    """sigma_2 / sigma_1 of the centred points: near 0 they lie on a line and the fit's rotation about it is arbitrary."""
    p = np.asarray(pts, np.float64)
    s = np.linalg.svd(p - p.mean(0), compute_uv=False)
    return float(s[1] / s[0]) if s[0] > 0 else 0.0


# ------------------------------------------------------------------ computeErrorMetric
def terms(src, tgt, T, thr, chunk=4096):
    """Per source point (term, bound), float64.  See error()."""
    s = np.asarray(src, F32).astype(np.float64)
    t = np.asarray(tgt, F32).astype(np.float64)
    t = t[np.isfinite(t).all(1)]
    T = np.asarray(T, F32).astype(np.float64)
    thr = float(F32(thr))
    term = np.ones(len(s))
    bound = np.zeros(len(s))
    ok = np.flatnonzero(np.isfinite(s).all(1))
    if len(t) == 0 or not np.isfinite(T).all():
        return term, bound
    for a in range(0, len(ok), chunk):
        i = ok[a:a + chunk]
        p = s[i]
        x = p @ T[:3, :3].T + T[:3, 3]
        d2 = ((x[:, None, :] - t[None, :, :]) ** 2).sum(2).min(1)
        d = np.sqrt(d2)
        mag = np.sqrt(((np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])) ** 2).sum(1))
        delta = 4.01 * U32 * mag
        delta = delta + 3.0 * U32 * (d + delta)
        term[i] = np.where(d2 <= thr, d2 / thr, 1.0)
        b = (2.0 * d * delta + delta * delta) / thr + U32
        bound[i] = np.where(d - delta > np.sqrt(thr), 0.0, b)
    return term, bound


def error(src, tgt, T, thr, chunk=4096):
    """(error, bound).  The transformed source is taken in float64 from the float32 T given; d2 is the squared distance to the
    nearest finite target point by brute force.  A point's term is d2 / thr if d2 <= thr, else 1: the SQUARED distance against the
    threshold as given, not squared (PCL's TruncatedError); thr is taken as the float32 the call receives.  A non-finite source
    point, or any point under a non-finite T or against no finite target point, has term 1.  The terms are summed in float64.

    bound: what a float32 evaluation of the same sum may differ by, sum of (2 d delta + delta^2) / thr + u over the finite points,
    u = 2^-24.  The term is continuous in d2 with slope at most 1 / thr, and the nearest distance moves by at most delta when the
    point does, so a distance error delta costs at most (2 d delta + delta^2) / thr.  delta counts the roundings:
      * a coordinate ((r0 x + r1 y) + r2 z) + t passes each product through 1 multiplication and at most 3 additions: 4 roundings,
        |error| <= 4.01 u m_r with m_r = |r0 x| + |r1 y| + |r2 z| + |t|; the point moves by at most 4.01 u |m|_2.
      * (dx dx + dy dy) + dz dz with d = x - p: the subtraction (counted twice, it is squared), the multiplication and at most 2
        additions, 5 roundings of non-negative terms: the squared distance is off by a factor within 1 +- 5.01 u, the distance by
        1 +- 3 u.
      so delta = 4.01 u |m|_2 + 3 u (d + 4.01 u |m|_2): a few ulps of the transformed point's magnitude.
      * the division by thr is one more rounding of a term that is at most 1: + u.
    A point with d - delta > sqrt(thr) scores exactly 1 either way: bound 0.  The sum itself is not covered: a caller whose device
    sums in float32 adds that (accumulation_bound)."""
    term, bound = terms(src, tgt, T, thr, chunk)
    return float(term.sum()), float(bound.sum())


def accumulation_bound(terms_per_lane):
    """A lane that adds k terms of at most 1 in float32 makes k - 1 roundings of a partial sum of at most k: (k - 1) k u."""
    k = np.asarray(terms_per_lane, np.float64)
    return float(((k - 1) * k).sum() * U32)


# ------------------------------------------------------------------ the scan
def scan(errors):
    """The winner: a hypothesis replaces the best so far only if its error, as float32, is strictly lower; hypothesis 0 starts."""
    best = 0
    for i in range(1, len(errors)):
        if F32(errors[i]) < F32(errors[best]):
            best = i
    return best


# ------------------------------------------------------------------ the whole call
def run(src, src_feat, tgt, tgt_feat, max_iterations=400, nr_samples=5, k_correspondences=5, max_corr_dist=0.05,
        min_sample_dist=0.01, seed=1, forced_samples=None):
    """Every hypothesis's samples, picks, correspondences, transform, error and bound, and the winner.

    A hypothesis is void if one of its samples has no matching descriptor (correspondence -1) or its fit is not finite (a non-finite
    point among its pairs): it scores |source| (every term 1) and its transform is the identity."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    H, S, K = max_iterations, nr_samples, k_correspondences
    if forced_samples is not None:
        fs = np.asarray(forced_samples, np.int32).reshape(2, H, S)
        samp, corr, pick = fs[0], fs[1], None
    else:
        samp, pick = draws(src, S, K, H, min_sample_dist, seed)
        sf = np.asarray(src_feat, F32).reshape(-1, 33)
        uniq = np.unique(samp)
        nn = np.full((len(src), K), -1, np.int32)
        nn[uniq] = feature_knn(tgt_feat, sf[uniq], K)
        corr = correspondences(samp, pick, nn)
    T = np.tile(np.eye(4, dtype=F32), (H, 1, 1))
    err = np.full(H, float(len(src)))
    bound = np.zeros(H)
    void = np.zeros(H, bool)
    for h in range(H):
        if (corr[h] < 0).any():
            void[h] = True
            continue
        Th = fit(src[samp[h]], tgt[corr[h]])
        if not np.isfinite(Th).all():
            void[h] = True
            continue
        T[h] = Th
        err[h], bound[h] = error(src, tgt, Th, max_corr_dist)
    best = scan(err)
    return dict(samples=samp, picks=pick, targets=corr, T=T, error=err, bound=bound, void=void, best_iteration=best,
                T_best=T[best].copy(), best_error=float(err[best]))
