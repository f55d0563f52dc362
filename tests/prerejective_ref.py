"""ope_prerejective restated in numpy: pcl::SampleConsensusPrerejective as include/ope.h specifies it, float32 where the device is
float32 and in the device's operation order, float64 where it is float64.  The error's sum is math.fsum (correctly rounded): the
device's sum has an order of its own, and a test allows it the rounding of a sum of non-negative terms.

Nothing here calls the library.  test_prerejective_ref.py pins this file on its own (known poses, cKDTree, a plain loop)."""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
F32 = np.float32


# ------------------------------------------------------------------ draws
class Lcg:
    """The stream of sacia_draws: x <- x * 6364136223846793005 + 1442695040888963407 (mod 2^64), next() = (x >> 11) / 2^53."""

    def __init__(self, seed):
        self.x = int(seed) & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return float(self.x >> 11) * (1.0 / 9007199254740992.0)


def draws(ns, S, K, H, seed):
    """Per iteration S distinct source indices int(ns * next()) (an index equal to an earlier one of the iteration is drawn again),
    then S picks int(K * next())."""
    rng = Lcg(seed)
    samp = np.zeros((H, S), np.int32)
    pick = np.zeros((H, S), np.int32)
    for it in range(H):
        got = []
        while len(got) < S:
            si = int(ns * rng.next())
            if si not in got:
                got.append(si)
        samp[it] = got
        pick[it] = [int(K * rng.next()) for _ in range(S)]
    return samp, pick


# ------------------------------------------------------------------ correspondences
def feature_knn(tgt_feat, q_feat, K):
    """The K nearest target descriptors of every query row: squared L2 summed in float32, component after component; ties by
    index; NaN distances never match (-1 pads a short row)."""
    tf = np.asarray(tgt_feat, F32)
    out = np.full((len(q_feat), K), -1, np.int32)
    for j, q in enumerate(np.asarray(q_feat, F32)):
        d = np.zeros(len(tf), F32)
        for c in range(33):
            u = q[c] - tf[:, c]
            d = d + u * u
        ok = np.flatnonzero(d == d)
        order = ok[np.argsort(d[ok], kind="stable")][:K]
        out[j, :len(order)] = order
    return out


def correspondences(samp, pick, src_feat, tgt_feat, K):
    uniq = np.unique(samp)
    nn = feature_knn(tgt_feat, np.asarray(src_feat, F32)[uniq], K)
    row = nn[np.searchsorted(uniq, samp)]                       # (H, S, K)
    c = np.take_along_axis(row, pick[..., None].astype(np.int64), axis=2)[..., 0]
    return np.where(c >= 0, c, row[..., 0]).astype(np.int32)


# ------------------------------------------------------------------ prerejection
def edge_ratios(src, tgt, samp, corr):
    """(H, S) float32: per edge i -> (i + 1) mod S the smaller of the two squared lengths over the larger."""
    ps, pt = np.asarray(src, F32)[samp], np.asarray(tgt, F32)[corr]            # (H, S, 3)

    def d2(p):
        d = p - np.roll(p, -1, axis=1)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    ds, dt = d2(ps), d2(pt)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ds < dt, ds / dt, dt / ds).astype(F32)


def polygon(src, tgt, samp, corr, similarity):
    thr2 = F32(similarity) * F32(similarity)
    return (edge_ratios(src, tgt, samp, corr) >= thr2).all(1)    # a NaN ratio compares false


# ------------------------------------------------------------------ the fit
def _jacobi3(S):
    S = [float(v) for v in S]
    V = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    for _ in range(60):
        off = abs(S[1]) + abs(S[2]) + abs(S[5])
        diag = abs(S[0]) + abs(S[4]) + abs(S[8])
        if off <= 1e-300 or off <= 1e-16 * diag:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = S[3 * p + q]
                if apq == 0.0:
                    continue
                theta = (S[3 * q + q] - S[3 * p + p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    a, b = S[3 * k + p], S[3 * k + q]
                    S[3 * k + p], S[3 * k + q] = c * a - s * b, s * a + c * b
                for k in range(3):
                    a, b = S[3 * p + k], S[3 * q + k]
                    S[3 * p + k], S[3 * q + k] = c * a - s * b, s * a + c * b
                for k in range(3):
                    a, b = V[3 * k + p], V[3 * k + q]
                    V[3 * k + p], V[3 * k + q] = c * a - s * b, s * a + c * b
    return S, V


def _det3(M):
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6])


def umeyama(ps, pt):
    """Eigen::umeyama(src, dst, false) as the library's host fit runs it (fp64; SVD through the eigenvectors of sigma^T sigma, Gram-
    Schmidt with completion, Eigen's rank rule), cast to float32 at the end.  (4, 4) math layout."""
    ps, pt = np.asarray(ps, np.float64), np.asarray(pt, np.float64)
    n = len(ps)
    sm, dm = ps.sum(0) / n, pt.sum(0) / n
    sigma = [0.0] * 9
    for i in range(n):
        for r in range(3):
            for c in range(3):
                sigma[3 * r + c] += (pt[i, r] - dm[r]) * (ps[i, c] - sm[c])
    sigma = [v / n for v in sigma]
    AtA = [sigma[i] * sigma[j] + sigma[3 + i] * sigma[3 + j] + sigma[6 + i] * sigma[6 + j] for i in range(3) for j in range(3)]
    D, Vt = _jacobi3(AtA)
    ev = [D[0], D[4], D[8]]
    order = sorted(range(3), key=lambda a: -ev[a])          # stable, descending
    V = [0.0] * 9
    for c in range(3):
        for r in range(3):
            V[3 * r + c] = Vt[3 * r + order[c]]
    Uc, sv = [], []
    for c in range(3):
        u = [sigma[3 * r] * V[c] + sigma[3 * r + 1] * V[3 + c] + sigma[3 * r + 2] * V[6 + c] for r in range(3)]
        Uc.append(u)
        sv.append(math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))
    tiny = 1e-14 * (sv[0] if sv[0] > 0 else 1.0)
    for c in range(3):
        u = Uc[c]
        for p in range(c):
            d = u[0] * Uc[p][0] + u[1] * Uc[p][1] + u[2] * Uc[p][2]
            for r in range(3):
                u[r] -= d * Uc[p][r]
        nrm = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        if sv[c] <= tiny or nrm <= 1e-8 * sv[c] + 1e-300:
            if c == 0:
                u[:] = [1.0, 0.0, 0.0]
            elif c == 1:
                a = Uc[0]
                m = (0 if abs(a[0]) < abs(a[2]) else 2) if abs(a[0]) < abs(a[1]) else (1 if abs(a[1]) < abs(a[2]) else 2)
                d = a[m]
                u[:] = [(1.0 if r == m else 0.0) - d * a[r] for r in range(3)]
            else:
                a, b = Uc[0], Uc[1]
                u[:] = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            nrm = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        for r in range(3):
            u[r] /= nrm
    U = [Uc[c][r] for r in range(3) for c in range(3)]
    Sg = [1.0, 1.0, -1.0 if _det3(sigma) < 0 else 1.0]
    rank = sum(1 for i in range(3) if not (abs(sv[i]) <= abs(sv[0]) * 1e-5))
    if rank == 2:
        Sg = [1.0, 1.0, 1.0 if _det3(U) * _det3(V) > 0 else -1.0]
    T = np.eye(4, dtype=np.float64)
    for i in range(3):
        for j in range(3):
            T[i, j] = sum(U[3 * i + k] * Sg[k] * V[3 * j + k] for k in range(3))
    for i in range(3):
        T[i, 3] = dm[i] - (T[i, 0] * sm[0] + T[i, 1] * sm[1] + T[i, 2] * sm[2])
    return T.astype(F32)


def singular_ratio(ps):
    """sigma_2 / sigma_1 of the centred source polygon: how far it is from a line (the fit's conditioning)."""
    p = np.asarray(ps, np.float64)
    s = np.linalg.svd(p - p.mean(0), compute_uv=False)
    return float(s[1] / s[0]) if s[0] > 0 else 0.0


# ------------------------------------------------------------------ the score
def transform(T, pts):
    """xform_row: ((r0 x + r1 y) + r2 z) + r3 per row, float32."""
    T, p = np.asarray(T, F32), np.asarray(pts, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def nearest_d2(q, tgt):
    """float32 squared distance of every query to its nearest finite target point: (dx dx + dy dy) + dz dz with d = q - p, the
    minimum over all points (what an exact search returns)."""
    t = np.asarray(tgt, F32)
    t = t[np.isfinite(t).all(1)]
    out = np.empty(len(q), F32)
    for a in range(0, len(q), 512):
        d = q[a:a + 512, None, :] - t[None, :, :]
        out[a:a + 512] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1)
    return out


def score(T, src, tgt, max_corr_dist):
    """getFitness: (inlier mask over the source, inliers, error)."""
    s = np.asarray(src, F32)
    finite = np.isfinite(s).all(1)
    mask = np.zeros(len(s), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = nearest_d2(transform(T, s[finite]), tgt).astype(np.float64)
    thr = float(max_corr_dist) * float(max_corr_dist)
    inl = d2 < thr                      # NaN (a transform that is not finite) compares false
    mask[np.flatnonzero(finite)[inl]] = True
    n = int(inl.sum())
    return mask, n, (math.fsum(d2[inl]) / n if n else FLT_MAX)


# ------------------------------------------------------------------ accept
def accept(survived, inliers, error, n_src, inlier_fraction):
    """The accept loop in iteration order: the winner's iteration, -1 for none."""
    lowest, best = FLT_MAX, -1
    for it in np.flatnonzero(survived):
        if F32(inliers[it]) / F32(n_src) >= F32(inlier_fraction) and error[it] < lowest:
            lowest, best = float(error[it]), int(it)
    return best


def align(src, src_feat, tgt, tgt_feat, max_iterations=50000, nr_samples=3, k_correspondences=5, similarity_threshold=0.8,
          max_corr_dist=0.15, inlier_fraction=0.25, seed=1, forced_samples=None):
    """The whole call.  forced_samples: (2, H, S) source then target indices."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    H, S, K = max_iterations, nr_samples, k_correspondences
    if forced_samples is not None:
        fs = np.asarray(forced_samples, np.int32).reshape(2, H, S)
        samp, corr, pick = fs[0], fs[1], None
    else:
        samp, pick = draws(len(src), S, K, H, seed)
        corr = correspondences(samp, pick, src_feat, tgt_feat, K)
    survived = polygon(src, tgt, samp, corr, similarity_threshold)
    T = np.tile(np.eye(4, dtype=F32), (H, 1, 1))
    inliers = np.zeros(H, np.int32)
    error = np.full(H, FLT_MAX, np.float64)
    for it in np.flatnonzero(survived):
        T[it] = umeyama(src[samp[it]], tgt[corr[it]])
        _, inliers[it], error[it] = score(T[it], src, tgt, max_corr_dist)
    best = accept(survived, inliers, error, len(src), inlier_fraction)
    out = dict(samples=samp, picks=pick, targets=corr, survived=survived, T=T, inliers=inliers, error=error, best_iteration=best,
               converged=best >= 0, T_best=T[best].copy() if best >= 0 else np.eye(4, dtype=F32))
    if best >= 0:
        out["inlier_idx"] = np.flatnonzero(score(T[best], src, tgt, max_corr_dist)[0]).astype(np.int32)
    return out
