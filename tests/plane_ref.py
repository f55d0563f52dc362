"""Host reference of the table-top segmentation for the plane tests (not a test module): pcl::SACSegmentation (SACMODEL_PLANE,
SAC_RANSAC, optimised coefficients), pcl::ExtractPolygonalPrismData and the steps of
ObjectSegmentationPlane::getSegmentedObjectsOnPlane between them, function by function, in numpy.  float32 wherever PCL has
`float`, float64 where it has `double`; every float32 operation below is a single correctly rounded numpy operation (no fused
multiply-add), so the order written here IS the specification the device follows.  PCL itself is not available: parity with it
stays unpinned; the PCL function each part follows is named beside it.

Orders this file fixes (PCL leaves them to Eigen's vectorisation):
  * a 4-vector dot product n . p with p.w = 1 (plane distances):      ((a*x + b*y) + c*z) + d
  * a 3-vector dot product / squared norm (the fourth term is 0):      (x*x + y*y) + z*z
  * normalize():                                                       v / sqrt(squared norm), a division per component
  * the crossing test runs over every hull edge once (vertex m-1 -> 0 first), in double.
  * RandomSampleConsensus starts from n_best_inliers_count = -INT_MAX: a first hypothesis with 0 inliers is a model.
  * ExtractPolygonalPrismData re-anchors d on vertex 0 only when it flips the normal (as PCL's source does).
"""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2147483647
DBL_EPSILON = sys.float_info.epsilon
FLT_MAX = float(np.finfo(np.float32).max)
MAX_SAMPLE_CHECKS = 1000          # SampleConsensusModel::max_sample_checks_

DEFAULTS = dict(distance_threshold=0.01, max_iterations=50, probability=0.99, optimize_coefficients=1, seed=12345)


# ---------------------------------------------------------------- std::mt19937
class Mt19937:
    """std::mt19937 (32-bit engine).  rnd() below is boost's uniform_int<>(0, INT_MAX) over it: engine() >> 1."""

    def __init__(self, seed: int):
        s = [0] * 624
        s[0] = seed & 0xFFFFFFFF
        for k in range(1, 624):
            s[k] = (1812433253 * (s[k - 1] ^ (s[k - 1] >> 30)) + k) & 0xFFFFFFFF
        self.s, self.i = s, 624

    def __call__(self) -> int:
        s = self.s
        if self.i >= 624:
            for k in range(624):
                y = (s[k] & 0x80000000) | (s[(k + 1) % 624] & 0x7FFFFFFF)
                s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = s[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF

    def rnd(self) -> int:
        return self() >> 1


# ---------------------------------------------------------------- eigen33 (pcl/common/impl/eigen.hpp), through the oracle's restatement
_eig = None


def _eigen_lib():
    """oracle/features.c's eigen33 (what the normals' reference runs) behind one exported wrapper, compiled once per process."""
    global _eig
    if _eig is None:
        d = tempfile.mkdtemp(prefix="plane_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        shim = os.path.join(d, "shim.c")
        with open(shim, "w") as f:
            f.write('#include "features.c"\nvoid plane_ref_eigen33(const float *m, float *ev, float *v) { eigen33(m, ev, v); }\n')
        orc = os.path.join(ROOT, "oracle")
        so = os.path.join(d, "libplane_ref.so")
        others = [os.path.join(orc, s) for s in ("kdtree.c", "icp.c", "filters.c", "pose.c", "lm.c")]
        subprocess.check_call(["gcc", "-O3", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I", orc, "-shared", "-o", so,
                               shim, *others, "-lm", "-lpthread"])
        _eig = ctypes.CDLL(so)
        _eig.plane_ref_eigen33.restype = None
    return _eig


def eigen33_smallest(cov: np.ndarray):
    """pcl::eigen33 (mat, eigenvalue, eigenvector): the smallest eigenpair of a symmetric float 3x3."""
    m = np.ascontiguousarray(cov, F).reshape(9)
    ev = ctypes.c_float()
    v = np.zeros(3, F)
    fp = ctypes.POINTER(ctypes.c_float)
    _eigen_lib().plane_ref_eigen33(m.ctypes.data_as(fp), ctypes.byref(ev), v.ctypes.data_as(fp))
    return F(ev.value), v


# ---------------------------------------------------------------- small float32 pieces
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    """Eigen normalize(): v / norm()."""
    v = np.asarray(v, F)
    return v / np.sqrt(dot3(v, v))


def plane_distance(coeff, pts):
    """The signed distance n . p + d (pointToPlaneDistanceSigned; the dot product of countWithinDistance): float32."""
    c = np.asarray(coeff, F)
    p = np.asarray(pts, F)
    with np.errstate(all="ignore"):
        return ((c[0] * p[..., 0] + c[1] * p[..., 1]) + c[2] * p[..., 2]) + c[3]


# ---------------------------------------------------------------- SampleConsensusModelPlane
def is_sample_good(p0, p1, p2) -> bool:
    """SampleConsensusModelPlane::isSampleGood: r = (p1 - p0) / (p2 - p0); good iff r[0] != r[1] || r[2] != r[1]."""
    with np.errstate(all="ignore"):
        r = (np.asarray(p1, F) - np.asarray(p0, F)) / (np.asarray(p2, F) - np.asarray(p0, F))
    return bool(r[0] != r[1]) or bool(r[2] != r[1])


def draw_samples(pts: np.ndarray, n_hyp: int, seed: int):
    """SampleConsensusModel::getSamples / drawIndexSample for the n_hyp consecutive iterations RANSAC can run: a persistent
    shuffled_indices_ over ALL points, three swaps per draw, up to 1000 redraws while isSampleGood fails.  The list ends early
    where getSamples would hand back an empty selection."""
    n = len(pts)
    out = []
    if n < 3:
        return np.zeros((0, 3), np.int32)
    rng = Mt19937(seed)
    shuf = list(range(n))
    for _ in range(n_hyp):
        good = False
        for _check in range(MAX_SAMPLE_CHECKS):
            for i in range(3):
                j = i + rng.rnd() % (n - i)
                shuf[i], shuf[j] = shuf[j], shuf[i]
            s = shuf[:3]
            if is_sample_good(pts[s[0]], pts[s[1]], pts[s[2]]):
                good = True
                break
        if not good:
            break
        out.append(s)
    return np.asarray(out, np.int32).reshape(-1, 3)


def sample_plane(p0, p1, p2) -> np.ndarray:
    """SampleConsensusModelPlane::computeModelCoefficients: n = (p1 - p0) x (p2 - p0), normalize(), d = -(n . p0)."""
    p0, p1, p2 = (np.asarray(p, F) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
        n = normalize3(n)
        return np.array([n[0], n[1], n[2], -dot3(n, p0)], F)


def within(coeff, pts, threshold: float) -> np.ndarray:
    """countWithinDistance / selectWithinDistance: fabsf(distance) < threshold, the comparison in double (strict)."""
    with np.errstate(all="ignore"):
        return np.abs(plane_distance(coeff, pts)).astype(np.float64) < float(threshold)


def seq_sum(v) -> np.float32:
    """A sequential float32 sum, in order."""
    v = np.asarray(v, F)
    return np.cumsum(v, dtype=F)[-1] if len(v) else F(0)


def mean_and_covariance(pts: np.ndarray):
    """pcl::computeMeanAndCovarianceMatrix (single pass): nine float running sums in the points' order, divided by the count,
    covariance = sums - mean * mean^T.  Returns (cov 3x3, centroid)."""
    p = np.asarray(pts, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    accu = np.array([seq_sum(x * x), seq_sum(x * y), seq_sum(x * z), seq_sum(y * y), seq_sum(y * z), seq_sum(z * z), seq_sum(x), seq_sum(y),
                     seq_sum(z)], F)
    accu = accu / F(len(p))
    cov = np.zeros((3, 3), F)
    cov[0, 0] = accu[0] - accu[6] * accu[6]
    cov[0, 1] = accu[1] - accu[6] * accu[7]
    cov[0, 2] = accu[2] - accu[6] * accu[8]
    cov[1, 1] = accu[3] - accu[7] * accu[7]
    cov[1, 2] = accu[4] - accu[7] * accu[8]
    cov[2, 2] = accu[5] - accu[8] * accu[8]
    cov[1, 0], cov[2, 0], cov[2, 1] = cov[0, 1], cov[0, 2], cov[1, 2]
    return cov, accu[6:9].copy()


def optimize_coefficients(pts, inliers, coeff) -> np.ndarray:
    """SampleConsensusModelPlane::optimizeModelCoefficients: fewer than 4 inliers leave the coefficients; otherwise the smallest
    eigenvector of the inliers' covariance and d = -(n . centroid)."""
    if len(inliers) < 4:
        return np.asarray(coeff, F).copy()
    cov, cen = mean_and_covariance(np.asarray(pts, F)[inliers])
    _, n = eigen33_smallest(cov)
    return np.array([n[0], n[1], n[2], -dot3(n, cen)], F)


# ---------------------------------------------------------------- RandomSampleConsensus::computeModel
def _k_of(best: int, n: int, probability: float) -> float:
    w = best / n
    p = 1.0 - math.pow(w, 3.0)
    p = max(DBL_EPSILON, p)
    p = min(1.0 - DBL_EPSILON, p)
    return math.log(1.0 - probability) / math.log(p)


def replay_loop(counts, n: int, max_iterations: int, probability: float):
    """The loop over counts already known: (winner or -1, iterations)."""
    best, best_cnt, k, it = -1, -INT_MAX, 1.0, 0
    while it < k:
        if it >= len(counts):
            break
        if int(counts[it]) > best_cnt:
            best_cnt, best = int(counts[it]), it
            k = _k_of(best_cnt, n, probability)
        it += 1
        if it > max_iterations:
            break
    return best, it


def literal_loop(pts, threshold: float, max_iterations: int, probability: float, seed: int):
    """RandomSampleConsensus::computeModel one hypothesis at a time: draw, model, count, update k.  Returns (coefficients or
    None, iterations, the samples drawn)."""
    n = len(pts)
    if n < 3:
        return None, 0, []
    rng = Mt19937(seed)
    shuf = list(range(n))
    best_cnt, k, it, model, drawn = -INT_MAX, 1.0, 0, None, []
    while it < k:
        sel = None
        for _check in range(MAX_SAMPLE_CHECKS):
            for i in range(3):
                j = i + rng.rnd() % (n - i)
                shuf[i], shuf[j] = shuf[j], shuf[i]
            s = shuf[:3]
            if is_sample_good(pts[s[0]], pts[s[1]], pts[s[2]]):
                sel = s
                break
        if sel is None:
            break
        drawn.append(sel)
        c = sample_plane(pts[sel[0]], pts[sel[1]], pts[sel[2]])
        cnt = int(within(c, pts, threshold).sum())
        if cnt > best_cnt:
            best_cnt, model = cnt, c
            k = _k_of(best_cnt, n, probability)
        it += 1
        if it > max_iterations:
            break
    return model, it, drawn


def plane_segment(pts, samples=None, **kw):
    """pcl::SACSegmentation::segment as the device runs it: every hypothesis first, the loop replayed.  Returns a dict:
    found, coeff, inliers, iterations, best, samples, hyp_coeffs, counts."""
    p = dict(DEFAULTS, **kw)
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    if samples is None:
        samples = draw_samples(pts, p["max_iterations"] + 1, p["seed"])
    samples = np.asarray(samples, np.int32).reshape(-1, 3)
    hyp = np.array([sample_plane(pts[a], pts[b], pts[c]) for a, b, c in samples], F).reshape(-1, 4)
    counts = np.array([int(within(c, pts, p["distance_threshold"]).sum()) for c in hyp], np.int32)
    best, it = replay_loop(counts, n, p["max_iterations"], p["probability"])
    out = dict(found=best >= 0, coeff=None, inliers=np.zeros(0, np.int32), iterations=it, best=best, samples=samples, hyp_coeffs=hyp,
               counts=counts)
    if best < 0:
        return out
    coeff = hyp[best]
    if p["optimize_coefficients"]:
        inl = np.flatnonzero(within(coeff, pts, p["distance_threshold"]))
        coeff = optimize_coefficients(pts, inl, coeff)
    out["coeff"] = coeff
    out["inliers"] = np.flatnonzero(within(coeff, pts, p["distance_threshold"])).astype(np.int32)
    return out


# ---------------------------------------------------------------- projection, prism
def project_points(pts, coeff) -> np.ndarray:
    """SampleConsensusModelPlane::projectPoints (ProjectInliers): n' = normalize(a b c); p - n' * ((n' . p) + d)."""
    c = np.asarray(coeff, F)
    p = np.asarray(pts, F)
    with np.errstate(all="ignore"):
        u = normalize3(c[:3])
        dist = plane_distance(np.array([u[0], u[1], u[2], c[3]], F), p)
        return np.stack([p[:, 0] - u[0] * dist, p[:, 1] - u[1] * dist, p[:, 2] - u[2] * dist], axis=1).astype(F)


def hull_plane(hull) -> np.ndarray:
    """ExtractPolygonalPrismData::segment's plane of the hull: mean and covariance of the vertices, eigen33, d = -(n . centroid),
    flipped towards the viewpoint (0 0 0) as seen from vertex 0, and then d = -(n . vertex 0)."""
    h = np.asarray(hull, F).reshape(-1, 3)
    cov, cen = mean_and_covariance(h)
    _, n = eigen33_smallest(cov)
    c = np.array([n[0], n[1], n[2], -dot3(n, cen)], F)
    vp = np.zeros(3, F) - h[0]
    if dot3(vp, c[:3]) < 0:
        n = -c[:3]
        c = np.array([n[0], n[1], n[2], -dot3(n, h[0])], F)
    return c


def point_in_polygon(x, y, px, py) -> np.ndarray:
    """pcl::isXYPointIn2DXYPolygon, in double: the crossing test over every edge (x, y arrays of points; px, py the polygon)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    inside = np.zeros(x.shape, bool)
    m = len(px)
    xold, yold = float(px[m - 1]), float(py[m - 1])
    with np.errstate(all="ignore"):
        for v in range(m):
            xnew, ynew = float(px[v]), float(py[v])
            if xnew > xold:
                x1, x2, y1, y2 = xold, xnew, yold, ynew
            else:
                x1, x2, y1, y2 = xnew, xold, ynew, yold
            hit = ((xnew < x) == (x <= xold)) & ((y - y1) * (x2 - x1) < (y2 - y1) * (x - x1))
            inside ^= hit
            xold, yold = xnew, ynew
    return inside


def prism_extract(pts, hull, height_min: float = 0.0, height_max: float = FLT_MAX):
    """pcl::ExtractPolygonalPrismData::segment: (indices ascending, the hull's plane)."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    h = np.asarray(hull, F).reshape(-1, 3)
    c = hull_plane(h)
    with np.errstate(all="ignore"):
        dist = plane_distance(c, pts).astype(np.float64)
        in_height = ~((dist < height_min) | (dist > height_max))
        proj = project_points(pts, c)
    k0 = 0 if abs(float(c[0])) > abs(float(c[1])) else 1
    k0 = k0 if abs(float(c[k0])) > abs(float(c[2])) else 2
    k1, k2 = (k0 + 1) % 3, (k0 + 2) % 3
    inside = point_in_polygon(proj[:, k1], proj[:, k2], h[:, k1], h[:, k2])
    return np.flatnonzero(in_height & inside).astype(np.int32), c


# ---------------------------------------------------------------- getSegmentedObjectsOnPlane, steps 2-7
def corners_of(proj_inliers, coeff) -> np.ndarray:
    """objectsegmentationplane.cpp:172-188: getMinMax3D, (min - 0.1, max + 0.1) as doubles rounded to float, z from the plane."""
    p = np.asarray(proj_inliers, F)
    mn = [F(np.min(p[:, d])) for d in range(2)]
    mx = [F(np.max(p[:, d])) for d in range(2)]
    xs = [F(float(mn[0]) - 0.1), F(float(mn[0]) - 0.1), F(float(mx[0]) + 0.1), F(float(mx[0]) + 0.1)]
    ys = [F(float(mn[1]) - 0.1), F(float(mx[1]) + 0.1), F(float(mx[1]) + 0.1), F(float(mn[1]) - 0.1)]
    a, b, c, d = (F(v) for v in coeff)
    out = np.zeros((4, 3), F)
    with np.errstate(all="ignore"):
        for i in range(4):
            x, y = xs[i], ys[i]
            z = -((a * x) + (b * y) + d) / c
            out[i] = (x, y, z)
    return out


def tabletop_segment(pts, **kw):
    """Stage by stage: first fit, corners, prism, second fit on the prism's points (re-indexed ascending), plane / non-plane
    indices into the input.  status 0 OK, 1 no first plane, 2 no second plane."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    first = plane_segment(pts, **kw)
    out = dict(status=1, first=first)
    if not first["found"]:
        return out
    proj = project_points(pts[first["inliers"]], first["coeff"])
    corners = corners_of(proj, first["coeff"]) if len(proj) else None
    out.update(corners=corners)
    prism_idx, _ = prism_extract(pts, corners)
    second = plane_segment(pts[prism_idx], **kw)
    out.update(status=2, prism_idx=prism_idx, second=second)
    if not second["found"]:
        return out
    mask = np.zeros(len(prism_idx), bool)
    mask[second["inliers"]] = True
    out.update(status=0, plane_idx=prism_idx[mask], not_plane_idx=prism_idx[~mask])
    return out
