"""Host reference of ObjectSegmentationPlane::getSegmentedObjectsExceptPlane after its crop (not a test module): the loop of
objectsegmentationplane.cpp:296-319 written over plane_ref.plane_segment, and getClusters (:324) over
cluster_ref.reference_clusters.

    m = n0 = number of points (non-finite ones included)
    while float(m) > keep_fraction * float(n0):          # the test comes BEFORE each fit, in double
        [max_planes > 0 and that many planes peeled: stop MAX_PLANES]
        a fresh SACSegmentation::segment of the remainder, re-indexed 0..m-1 in ascending original order, same parameters and seed
        no model, or no inlier: stop NO_INLIERS
        the remainder loses the inliers (ExtractIndices negative: the order is kept)
"""
from __future__ import annotations

import numpy as np

import cluster_ref
import plane_ref

FRACTION, NO_INLIERS, MAX_PLANES = 0, 1, 2


def peel(pts, keep_fraction: float = 0.3, max_planes: int = 0, **plane_kw):
    """Returns a dict: coeffs (k, 4) float32, counts (k,), iterations (k,), inliers (per round, ORIGINAL indices ascending),
    remainders (per round, the ORIGINAL indices the round's fit saw), labels (n,), rest_idx, stop, last (the last fit's dict or
    None)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n0 = len(pts)
    rest = np.arange(n0, dtype=np.int32)
    labels = np.full(n0, -1, np.int32)
    coeffs, counts, its, inliers, remainders = [], [], [], [], []
    stop, last = FRACTION, None
    while float(len(rest)) > float(keep_fraction) * float(n0):
        if max_planes > 0 and len(coeffs) >= max_planes:
            stop = MAX_PLANES
            break
        last = plane_ref.plane_segment(pts[rest], **plane_kw)
        if not last["found"] or len(last["inliers"]) == 0:
            stop = NO_INLIERS
            break
        took = rest[last["inliers"]]
        labels[took] = len(coeffs)
        remainders.append(rest)
        inliers.append(took)
        coeffs.append(last["coeff"])
        counts.append(len(took))
        its.append(last["iterations"])
        keep = np.ones(len(rest), bool)
        keep[last["inliers"]] = False
        rest = rest[keep]
    return dict(coeffs=np.asarray(coeffs, np.float32).reshape(-1, 4), counts=np.asarray(counts, np.int32), iterations=np.asarray(its, np.int64),
                inliers=inliers, remainders=remainders, labels=labels, rest_idx=rest, stop=stop, last=last)


def except_plane(pts, keep_fraction: float = 0.3, max_planes: int = 0, tolerance: float = 0.05, min_size: int = 300, max_size: int = 100000,
                 **plane_kw):
    """(clusters as ORIGINAL indices of pts, ascending, in getClusters' order; the peel's dict)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    p = peel(pts, keep_fraction, max_planes, **plane_kw)
    rest = p["rest_idx"]
    local = cluster_ref.reference_clusters(pts[rest], tolerance, min_size, max_size) if len(rest) else []
    return [rest[np.asarray(c, np.int64)].astype(np.int32) for c in local], p
