"""Plain numpy references for the stand-alone scoring entry points: Registration::getFitnessScore on given nearest squared
distances (ope_fitness, the fitness pass of ope_icp_run_batch) and the two CorrespondenceRejector predicates on given pairs
(ope_reject_pairs).  The searches themselves come from the CPU oracle (oracle.KdTree, oracle.transform_points); what is
restated here is the arithmetic after them, in the number formats include/ope.h and the kernels state."""
import math

import numpy as np

import oracle

F32, F64 = np.float32, np.float64
DBL_MAX = float(np.finfo(np.float64).max)


def nearest_d2(src, tgt, T):
    """fp32 squared distance of every FINITE row of src, moved by T (fp32, the oracle's operation order), to its nearest
    point of tgt: (d2 of the finite rows, mask of the finite rows)."""
    src = np.ascontiguousarray(src, F32).reshape(-1, 3)
    ok = np.isfinite(src).all(1)
    if not ok.any():
        return np.empty(0, F32), ok
    _, d2, found = oracle.KdTree(tgt).knn(oracle.transform_points(src[ok], np.asarray(T, F32)), 1)
    assert (found == 1).all()
    return d2[:, 0].copy(), ok


def fitness_from_d2(d2, max_range=DBL_MAX):
    """getFitnessScore(max_range) on the nearest squared distances d2 (fp32): the rows with (double)d2 <= max_range,
    INCLUSIVE (registration.hpp: `if (nn_dists[0] <= max_range)`), summed exactly (math.fsum).  Returns (sum, n)."""
    d = np.asarray(d2, F32).astype(F64)
    sel = d <= max_range
    return math.fsum(d[sel].tolist()), int(sel.sum())


def fitness_score(total, n):
    """the score of (sum, n): the mean, DBL_MAX when no point was in range"""
    return total / n if n > 0 else DBL_MAX


def sum_bound(n):
    """Two fp64 sums of the same n non-negative terms, taken in different orders, differ by at most 2 (n - 1) 2^-53 relative
    (each is within (n - 1) 2^-53 of the exact sum, to first order)."""
    return 2.0 * max(n - 1, 0) * 2.0 ** -53


def _pairs(a, b):
    a = np.ascontiguousarray(a, F32).reshape(-1, 3)
    b = np.ascontiguousarray(b, F32).reshape(-1, 3)
    assert a.shape == b.shape
    return a, b


def surface_normal_score(a, b):
    """the fp32 score ((ax*bx + ay*by) + az*bz), every product and every sum rounded to fp32, in that order"""
    a, b = _pairs(a, b)
    with np.errstate(all="ignore"):
        p0, p1, p2 = a[:, 0] * b[:, 0], a[:, 1] * b[:, 1], a[:, 2] * b[:, 2]
        s = (p0 + p1) + p2
    assert s.dtype == F32
    return s


def reject_surface_normal(a, b, thr):
    """OPE_REJ_SURFACE_NORMAL: keep iff (double)score > thr (a NaN score is not kept)"""
    return surface_normal_score(a, b).astype(F64) > float(thr)


def self_occluded_score(a, b):
    """the fp64 score ax*(-bx/|b|) + ay*(-by/|b|) + az*(-bz/|b|), |b| the fp64 square root of the fp32 sum of squares
    ((bx*bx + by*by) + bz*bz); |b| = 0 gives 0/0 = NaN"""
    a, b = _pairs(a, b)
    with np.errstate(all="ignore"):
        ss = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
        assert ss.dtype == F32
        sl = np.sqrt(ss.astype(F64))
        ad, bd = a.astype(F64), b.astype(F64)
        s = (ad[:, 0] * (-bd[:, 0] / sl) + ad[:, 1] * (-bd[:, 1] / sl)) + ad[:, 2] * (-bd[:, 2] / sl)
    return s


def reject_self_occluded(a, b, thr):
    """OPE_REJ_SELF_OCCLUDED: keep iff score > thr (a NaN score is not kept)"""
    with np.errstate(invalid="ignore"):
        return self_occluded_score(a, b) > float(thr)


def apply64(T, P):
    T = np.asarray(T, F64)
    return np.asarray(P, F64) @ T[:3, :3].T + T[:3, 3]


def rms(T, P, Q):
    """root mean square distance of T * P to Q, in fp64"""
    return float(np.sqrt(((apply64(T, P) - np.asarray(Q, F64)) ** 2).sum(1).mean()))


def svd_case(name, T):
    """Paired points (P, Q) for TransformationEstimationSVD, Q = T * P rounded to fp32: 1, 2 and 3 pairs, 64 collinear, 300
    coplanar, 5 000 generic pairs whose first (the pivot of the device's sums) lies 1 m off the 5 cm cluster, and a cloud
    paired with its mirror image."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("n1", "n2", "n3"):
        P = rng.uniform(-0.1, 0.1, (int(name[1]), 3))
    elif name == "collinear":
        P = np.array([0.02, -0.01, 0.03]) + rng.uniform(-0.1, 0.1, (64, 1)) * np.array([[0.6, -0.48, 0.64]])
    elif name == "coplanar":
        e1, e2 = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0])
        P = np.array([0.01, 0.02, -0.03]) + rng.uniform(-0.1, 0.1, (300, 1)) * e1 + rng.uniform(-0.06, 0.06, (300, 1)) * e2
    elif name == "outlier_pivot":
        P = np.array([0.3, -0.2, 0.5]) + rng.uniform(-0.025, 0.025, (5000, 3))
        P[0] = P[1:].mean(0) + np.array([0.6, 0.0, 0.8])
    elif name == "mirrored":
        v = rng.standard_normal((3000, 3))
        P = v / np.linalg.norm(v, axis=1, keepdims=True) * np.array([0.09, 0.06, 0.03]) + np.array([0.01, 0.0, 0.02])
    else:
        raise KeyError(name)
    P = P.astype(F32)
    Q = apply64(T, P * np.array([1, 1, -1]) if name == "mirrored" else P).astype(F32)
    return P, Q


def unit_vectors(n, seed):
    """n fp32 unit vectors (to fp32 rounding), no zero components"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F32)


def on_threshold_cases():
    """Constructed pairs whose score is a known, exactly representable value: (kind, a, b, score).  The products and sums of
    the first four are exact; in the last, 3/5 and 4/5 round, and 0.5 * fl(0.6) + 0.25 * fl(0.8) is 0.5 again, exactly
    (test_pairs_ref.py checks every stated score against the references)."""
    return [
        (0, [1.0, 0.0, 0.0], [0.75, 0.0, 0.0], 0.75),
        (0, [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], 0.75),
        (0, [0.25, -0.5, 1.0], [1.0, 0.5, 0.625], 0.625),       # 0.25 - 0.25 + 0.625
        (1, [0.0, 0.0, 0.75], [0.0, 0.0, -2.0], 0.75),          # |b| = 2, -bz/|b| = 1
        (1, [0.5, 0.25, 0.0], [-3.0, -4.0, 0.0], 0.5),          # |b| = 5
    ]
