"""The correspondence pipeline of the reference's estimateCoarsePose (BuildModel/src/poseestimator.cpp:43-60, :111-113) restated in
numpy (not a test module): pcl::registration::CorrespondenceEstimation over FPFH rows, CorrespondenceRejectorSampleConsensus
(RandomSampleConsensus over SampleConsensusModelRegistration) and TransformationEstimationSVD over the matches that remain.
float32 wherever PCL has `float`, float64 where it has `double`; every float32 operation is a single correctly rounded numpy
operation, so the order written here IS the specification ope_feature_correspondences and ope_corr_sac follow.  PCL itself is not
available: parity with it stays unpinned; the PCL function each part follows is named beside it.

Orders this file fixes (PCL leaves them to Eigen):
  * a descriptor distance: the 33 squared differences added component after component, float32;
  * a squared norm of a 3-vector: (x*x + y*y) + z*z, float32;
  * a moved point: ((r0 x + r1 y) + r2 z) + r3 per row (the library's xform_row);
  * eigen_values.array().sqrt().sum(): (sqrt l0 + sqrt l1) + sqrt l2, float32, l0 <= l1 <= l2.
The engine, the draw, the nine running sums and RandomSampleConsensus::computeModel are those of tests/plane_ref.py; the fit is
that of tests/prerejective_ref.py.  Nothing here calls the library.  test_corr_sac_ref.py pins this file on its own."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import plane_ref
import prerejective_ref
from plane_ref import MAX_SAMPLE_CHECKS, Mt19937, mean_and_covariance, replay_loop

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MIN = float(np.finfo(np.float32).tiny)
DEFAULTS = dict(inlier_threshold=0.05, max_iterations=1000, probability=0.99, seed=12345)


# ---------------------------------------------------------------- CorrespondenceEstimation::determineCorrespondences
def feature_matches(src_feat, tgt_feat):
    """Source row i in ORIGINAL order -> the target row with the smallest squared L2 distance over the 33 floats (a sequential
    float32 sum), the lowest index on a tie.  A row without a finite distance gives no match.  (src_idx, tgt_idx, dist, dropped)."""
    sf = np.ascontiguousarray(src_feat, F).reshape(-1, 33)
    tf = np.ascontiguousarray(tgt_feat, F).reshape(-1, 33)
    si, ti, dd = [], [], []
    if len(tf):
        for i, q in enumerate(sf):
            with np.errstate(all="ignore"):
                d = np.zeros(len(tf), F)
                for c in range(33):
                    u = q[c] - tf[:, c]
                    d = d + u * u
            d = np.where(np.isfinite(d), d, F(np.inf))
            j = int(np.argmin(d))                       # the first of equal minima
            if np.isfinite(d[j]):
                si.append(i); ti.append(j); dd.append(d[j])
    return np.asarray(si, np.int32), np.asarray(ti, np.int32), np.asarray(dd, F), len(sf) - len(si)


# ---------------------------------------------------------------- pcl::eigen33 (mat, evals), through the oracle's restatement
_lib = None


def _roots_lib():
    """oracle/features.c's compute_roots (what eigen33 of the normals' reference runs) behind one exported wrapper."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="corr_sac_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        shim = os.path.join(d, "shim.c")
        with open(shim, "w") as f:
            f.write('#include "features.c"\nvoid corr_sac_ref_roots(const float *m, float *r) { compute_roots(m, r); }\n')
        orc = os.path.join(ROOT, "oracle")
        so = os.path.join(d, "libcorr_sac_ref.so")
        others = [os.path.join(orc, s) for s in ("kdtree.c", "icp.c", "filters.c", "pose.c", "lm.c")]
        subprocess.check_call(["gcc", "-O3", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I", orc, "-shared", "-o", so,
                               shim, *others, "-lm", "-lpthread"])
        _lib = ctypes.CDLL(so)
        _lib.corr_sac_ref_roots.restype = None
    return _lib


def eigenvalues33(cov) -> np.ndarray:
    """pcl::eigen33 (mat, evals): the roots of mat / max|mat| (1 when that is <= FLT_MIN), times it; ascending, float32."""
    m = np.ascontiguousarray(cov, F).reshape(9)
    scale = F(np.max(np.abs(m)))
    if scale <= F(FLT_MIN):
        scale = F(1.0)
    with np.errstate(all="ignore"):
        sm = (m / scale).astype(F)
    r = np.zeros(3, F)
    fp = ctypes.POINTER(ctypes.c_float)
    _roots_lib().corr_sac_ref_roots(sm.ctypes.data_as(fp), r.ctypes.data_as(fp))
    with np.errstate(all="ignore"):
        return (r * scale).astype(F)


# ---------------------------------------------------------------- SampleConsensusModelRegistration
def sample_dist_thresh(src_pts) -> float:
    """computeSampleDistanceThreshold: the float mean and covariance of the matched source points (computeMeanAndCovarianceMatrix,
    nine running sums in match order), its eigenvalues, t = ((sqrt l0 + sqrt l1) + sqrt l2) / 3.0, squared, a double."""
    cov, _ = mean_and_covariance(np.asarray(src_pts, F).reshape(-1, 3))
    with np.errstate(all="ignore"):
        r = np.sqrt(eigenvalues33(cov))
        t = float((r[0] + r[1]) + r[2]) / 3.0
    return t * t


def d2(a, b):
    """(dx*dx + dy*dy) + dz*dz of a - b, float32."""
    d = np.asarray(a, F) - np.asarray(b, F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def is_sample_good(p0, p1, p2, thresh: float) -> bool:
    """isSampleGood: the three squared edge lengths of the source triangle (float32) each > sample_dist_thresh (a double)."""
    return bool(float(d2(p1, p0)) > thresh and float(d2(p2, p0)) > thresh and float(d2(p2, p1)) > thresh)


def draw_samples(src_pts, n_hyp: int, seed: int, thresh: float) -> np.ndarray:
    """getSamples / drawIndexSample for the n_hyp consecutive iterations RANSAC can run: a persistent shuffled_indices_ over all
    matches, three swaps per draw with rnd() = engine() >> 1, up to 1000 redraws while isSampleGood fails.  The list ends where
    getSamples would hand back an empty selection.  (h, 3) match positions."""
    pts = np.asarray(src_pts, F).reshape(-1, 3)
    n = len(pts)
    out = []
    if n < 3:
        return np.zeros((0, 3), np.int32)
    rng = Mt19937(seed & 0xFFFFFFFF)
    shuf = list(range(n))
    for _ in range(n_hyp):
        good = False
        for _check in range(MAX_SAMPLE_CHECKS):
            for i in range(3):
                j = i + rng.rnd() % (n - i)
                shuf[i], shuf[j] = shuf[j], shuf[i]
            s = shuf[:3]
            if is_sample_good(pts[s[0]], pts[s[1]], pts[s[2]], thresh):
                good = True
                break
        if not good:
            break
        out.append(s)
    return np.asarray(out, np.int32).reshape(-1, 3)


def fit(src3, tgt3) -> np.ndarray:
    """computeModelCoefficients: Eigen::umeyama(src3, tgt3, false) in float64 over the three pairs, cast to float32; (4, 4)."""
    return prerejective_ref.umeyama(src3, tgt3)


def within(T, src_pts, tgt_pts, threshold: float) -> np.ndarray:
    """countWithinDistance / selectWithinDistance: |T s - t|^2 < threshold^2; the point moved in float32, the squared norm in
    float32, widened; threshold^2 a double; strict (a NaN compares false)."""
    with np.errstate(all="ignore"):
        moved = prerejective_ref.transform(T, np.asarray(src_pts, F).reshape(-1, 3))
        return d2(moved, np.asarray(tgt_pts, F).reshape(-1, 3)).astype(np.float64) < float(threshold) * float(threshold)


# ---------------------------------------------------------------- TransformationEstimationSVD over many pairs
def svd_pose(src_pts, tgt_pts) -> np.ndarray:
    """Umeyama without scaling over all pairs, float64 (numpy's SVD), as a float64 (4, 4): what the paired-points SVD is held to."""
    s, t = np.asarray(src_pts, np.float64).reshape(-1, 3), np.asarray(tgt_pts, np.float64).reshape(-1, 3)
    T = np.eye(4)
    if len(s) == 0:
        return T
    sm, tm = s.mean(0), t.mean(0)
    sigma = (t - tm).T @ (s - sm) / len(s)
    U, sv, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    T[:3, :3] = U @ np.diag(S) @ Vt
    T[:3, 3] = tm - T[:3, :3] @ sm
    return T


# ---------------------------------------------------------------- the rejector
def reject(src, tgt, src_idx, tgt_idx, samples=None, thresh=None, **kw):
    """CorrespondenceRejectorSampleConsensus::getRemainingCorrespondences as the device runs it: every hypothesis first, the loop
    replayed (plane_ref.replay_loop).  samples: (h, 3) forced match positions; thresh: the sample distance threshold to draw with
    (None: computed here).  Returns a dict: found, best, iterations, T_best, inlier_pos, samples, T, counts, thresh."""
    p = dict(DEFAULTS, **kw)
    src, tgt = np.asarray(src, F).reshape(-1, 3), np.asarray(tgt, F).reshape(-1, 3)
    si, ti = np.asarray(src_idx, np.int64).reshape(-1), np.asarray(tgt_idx, np.int64).reshape(-1)
    ps, pt = src[si], tgt[ti]
    n = len(si)
    if thresh is None:
        thresh = sample_dist_thresh(ps) if n else 0.0
    if n < 3:
        samples = np.zeros((0, 3), np.int32)
    elif samples is None:
        samples = draw_samples(ps, p["max_iterations"] + 1, p["seed"], thresh)
    samples = np.asarray(samples, np.int32).reshape(-1, 3)
    T = np.array([fit(ps[s], pt[s]) for s in samples], F).reshape(-1, 4, 4)
    counts = np.array([int(within(t, ps, pt, p["inlier_threshold"]).sum()) for t in T], np.int32)
    best, it = replay_loop(counts, max(n, 1), p["max_iterations"], p["probability"])
    out = dict(found=best >= 0, best=best, iterations=it, samples=samples, T=T, counts=counts, thresh=thresh,
               T_best=np.eye(4, dtype=F), inlier_pos=np.arange(n, dtype=np.int32))
    if best >= 0:
        out["T_best"] = T[best].copy()
        out["inlier_pos"] = np.flatnonzero(within(T[best], ps, pt, p["inlier_threshold"])).astype(np.int32)
    return out


def coarse_pose(src, src_feat, tgt, tgt_feat, **kw):
    """The three steps: matches, the rejector, the SVD over the remaining matches.  The rejector's dict plus matches, dropped and
    T_svd (float64)."""
    si, ti, dist, dropped = feature_matches(src_feat, tgt_feat)
    out = reject(src, tgt, si, ti, **kw)
    keep = out["inlier_pos"]
    out.update(matches=(si, ti, dist), dropped=dropped,
               T_svd=svd_pose(np.asarray(src, F)[si[keep]], np.asarray(tgt, F)[ti[keep]]))
    return out
