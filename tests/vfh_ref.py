"""A literal restatement of pcl::VFHEstimation::computeFeature / computePointSPFHSignature (PCL 1.7.x, features/impl/vfh.hpp)
with PCL's defaults, and of flann::ChiSquareDistance with an exact k-nearest search: what vfh.hip is compared with.

The pair features come from oracle.pair_features (the oracle's computePairFeatures, whose transcendental bits are the
device's); the bins are fp64 as in PCL; centroids and bin values are sequential fp32 sums.

Choices where PCL 1.7.x leaves the bits to Eigen (named in DESIGN 4.18 too):
  - compute3DCentroid leaves w = 1, so d_vp_p = (vp - c, -1) before it is normalised; setCentroidToUse takes a Vector3f, w = 0;
  - normalize(): the squared norm is summed x, y, z, w and every component is DIVIDED by the norm (Eigen >= 3.3; 3.2 multiplies by
    the reciprocal);
  - `centroid /= n` divides every component.
"""
from __future__ import annotations

import math

import numpy as np

import oracle

F = np.float32
NB = 45
NB_VP = 128
VP_OFF = 180
D_PI = float(F(1.0) / (F(2.0) * F(math.pi)))   # d_pi_ = 1.0f / (2.0f * static_cast<float>(M_PI)), widened


def replay(count: int, incr) -> np.float32:
    """`count` sequential float additions of incr from 0: what `hist[i] += hist_incr` leaves after count hits."""
    h = F(0.0)
    incr = F(incr)
    for _ in range(int(count)):
        h = F(h + incr)
    return h


def _seq_mean(a: np.ndarray) -> np.ndarray:
    """Sequential fp32 column sums of a (n, 3) in row order, divided by n."""
    s = [F(0.0), F(0.0), F(0.0)]
    for row in a:
        for d in range(3):
            s[d] = F(s[d] + row[d])
    n = F(len(a))
    return np.array([F(s[d] / n) for d in range(3)], F)


def _bin(u: float, nb: int):
    """floor(u) clamped to [0, nb): (bin, distance of u to the nearest integer edge, clamped?)"""
    h = int(math.floor(u))
    clamped = h < 0 or h >= nb
    return min(max(h, 0), nb - 1), abs(u - round(u)), clamped


def vfh(xyz, nrm, viewpoint=(0.0, 0.0, 0.0), given_centroid=None, given_normal=None) -> dict:
    """computeFeature of one cloud.  Returns sig (308,) float32, counts (308,) int32, bins (n, 4) uint8 (f1, f2, f3: 255 for a
    rejected pair; viewpoint bin), edge (n, 4) float64 (distance of each binned value, in bin units, to the nearest bin edge; nan
    for a rejected pair), clamped (n, 4) bool, rejected (int), centroid, normal_centroid, d_vp_p."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, F).reshape(-1, 3)
    n = len(xyz)
    counts = np.zeros(308, np.int32)
    bins = np.zeros((n, 4), np.uint8)
    edge = np.full((n, 4), np.nan)
    clamped = np.zeros((n, 4), bool)
    out = dict(sig=np.zeros(308, F), counts=counts, bins=bins, edge=edge, clamped=clamped, rejected=0)
    if n == 0:
        return out
    if given_centroid is not None:
        c, cw = np.asarray(given_centroid, F), F(0.0)
    else:
        c, cw = _seq_mean(xyz), F(1.0)
    nc = np.asarray(given_normal, F) if given_normal is not None else _seq_mean(nrm)
    vp = np.asarray(viewpoint, F)
    d = [F(vp[0] - c[0]), F(vp[1] - c[1]), F(vp[2] - c[2]), F(F(0.0) - cw)]
    sq = F(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])) + F(d[3] * d[3]))
    with np.errstate(divide="ignore", invalid="ignore"):
        nv = np.sqrt(sq)
        dvp = [F(x / nv) for x in d]
    rejected = 0
    for i in range(n):
        ok, (f1, f2, f3, _f4) = oracle.pair_features(c, nc, xyz[i], nrm[i])
        if ok:
            b, e, cl = _bin(NB * ((float(F(f1)) + math.pi) * D_PI), NB)
            bins[i, 0], edge[i, 0], clamped[i, 0] = b, e, cl
            counts[b] += 1
            b, e, cl = _bin(NB * ((float(F(f2)) + 1.0) * 0.5), NB)
            bins[i, 1], edge[i, 1], clamped[i, 1] = b, e, cl
            counts[NB + b] += 1
            b, e, cl = _bin(NB * ((float(F(f3)) + 1.0) * 0.5), NB)
            bins[i, 2], edge[i, 2], clamped[i, 2] = b, e, cl
            counts[2 * NB + b] += 1
        else:
            bins[i, :3] = 255
            rejected += 1
        v = nrm[i]
        dot = F(F(F(F(v[0] * dvp[0]) + F(v[1] * dvp[1])) + F(v[2] * dvp[2])) + F(F(0.0) * dvp[3]))
        b, e, cl = _bin(((float(dot) + 1.0) * 0.5) * NB_VP, NB_VP)
        bins[i, 3], edge[i, 3], clamped[i, 3] = b, e, cl
        counts[VP_OFF + b] += 1
    with np.errstate(divide="ignore"):
        incr = F(100.0) / F(n - 1)               # 100.0f / static_cast<float>(indices.size() - 1)
    incr_vp = F(100.0 / float(n))               # static_cast<float>(hist_incr), hist_incr a double
    sig = out["sig"]
    for b in range(308):
        if counts[b]:
            sig[b] = replay(counts[b], incr if b < 3 * NB else incr_vp)
    out.update(rejected=rejected, centroid=c, normal_centroid=nc, d_vp_p=np.array(dvp, F))
    return out


def chi2(a, b) -> np.float32:
    """flann::ChiSquareDistance in fp32, dimension by dimension."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    r = F(0.0)
    for x, y in zip(a, b):
        s = F(x + y)
        if s > 0:
            df = F(x - y)
            r = F(r + F(F(df * df) / s))
    return r


def chi2_rows(rows, q) -> np.ndarray:
    """chi2(q, row) of every row: the same sequential fp32 sum, vectorised over the rows."""
    rows = np.asarray(rows, F).reshape(-1, 308)
    q = np.asarray(q, F)
    r = np.zeros(len(rows), F)
    for d in range(308):
        s = rows[:, d] + q[d]
        df = q[d] - rows[:, d]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (df * df) / s
        r = np.where(s > 0, r + t, r).astype(F)
    return r


def knn(rows, queries, k: int):
    """Exact k nearest rows by (distance, row): (indices (q, k) int32, distances (q, k) float32), -1 / +inf past the rows."""
    rows = np.asarray(rows, F).reshape(-1, 308)
    queries = np.asarray(queries, F).reshape(-1, 308)
    idx = np.full((len(queries), k), -1, np.int32)
    dist = np.full((len(queries), k), np.inf, F)
    for i, q in enumerate(queries):
        d = chi2_rows(rows, q)
        order = np.lexsort((np.arange(len(rows)), d))[:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[order]
    return idx, dist


def object_name(names, idx_row, dist_row, thresh: float = 120.0):
    """getObjectName's decision (objectdetection.cpp:179-193): it reads neighbour [1], not [0]."""
    if len(idx_row) > 1 and idx_row[1] >= 0 and float(dist_row[1]) < thresh:
        return names[int(idx_row[1])].split("_")[0]
    return "ObjectNotFound"


# ---------------------------------------------------------------------------------------------------------------------------
# test clouds


def sphere_patch(n: int, seed: int, radius: float = 0.08, centre=(0.02, -0.01, 0.9), cap: float = 0.6):
    """n points of a sphere's cap facing the origin, with the outward normals flipped towards it."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(cap, 1.0, n)
    ph = rng.uniform(0.0, 2.0 * math.pi, n)
    s = np.sqrt(1.0 - u * u)
    d = np.stack([s * np.cos(ph), s * np.sin(ph), -u], 1)   # towards the camera at the origin
    return (np.asarray(centre) + radius * d).astype(F), d.astype(F)


def box_cloud(n: int, seed: int, half=(0.05, 0.03, 0.04), centre=(-0.03, 0.02, 0.8), yaw: float = 0.5, pitch: float = 0.4):
    """n points of the three faces of a rotated box that see the origin, with their normals."""
    rng = np.random.default_rng(seed)
    pts, nrm = _box_faces(rng, n, np.asarray(half))
    R = _rot(yaw, pitch)
    return _visible(pts @ R.T + np.asarray(centre), nrm @ R.T)


def _rot(yaw: float, pitch: float) -> np.ndarray:
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Rx @ Ry


def _visible(pts, nrm):
    keep = np.einsum("ij,ij->i", nrm, -pts) > 0.05 * np.linalg.norm(pts, axis=1)
    return pts[keep].astype(F), nrm[keep].astype(F)


def _box_faces(rng, n, half):
    face = rng.integers(0, 6, n)
    uv = rng.uniform(-1.0, 1.0, (n, 2))
    pts = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    for f in range(6):
        m = face == f
        a, sgn = f // 2, 1.0 if f % 2 else -1.0
        o = [x for x in range(3) if x != a]
        pts[m, a] = sgn * half[a]
        pts[m, o[0]] = uv[m, 0] * half[o[0]]
        pts[m, o[1]] = uv[m, 1] * half[o[1]]
        nrm[m, a] = sgn
    return pts, nrm


def _cylinder(rng, n, r=0.035, h=0.11):
    side = rng.uniform(0, 1, n) < 0.75
    ph = rng.uniform(0, 2 * math.pi, n)
    y = rng.uniform(-h / 2, h / 2, n)
    rr = r * np.sqrt(rng.uniform(0, 1, n))
    top = rng.uniform(0, 1, n) < 0.5
    pts = np.where(side[:, None], np.stack([r * np.cos(ph), y, r * np.sin(ph)], 1),
                   np.stack([rr * np.cos(ph), np.where(top, h / 2, -h / 2), rr * np.sin(ph)], 1))
    nrm = np.where(side[:, None], np.stack([np.cos(ph), 0 * y, np.sin(ph)], 1),
                   np.stack([0 * y, np.where(top, 1.0, -1.0), 0 * y], 1))
    return pts, nrm


def _cap(rng, n, r=0.06, cap=0.2):
    u = rng.uniform(cap, 1.0, n)
    ph = rng.uniform(0, 2 * math.pi, n)
    s = np.sqrt(1 - u * u)
    d = np.stack([s * np.cos(ph), u, s * np.sin(ph)], 1)
    return r * d - np.array([0, r * 0.5, 0]), d


SHAPES = ("box", "cylinder", "cap")
TRAIN_VIEWS = 6
VIEW_STEP = 0.02   # radians of yaw between training views; the queries lie half way between views 2 and 3
RECOGNITION_SEED = 7
RECOGNITION_POINTS = 3000


def shape_view(shape: str, yaw: float, pitch: float, seed: int, n: int = RECOGNITION_POINTS):
    """The points of `shape`, turned by (yaw, pitch) and set 0.8 m in front of the camera, that see the origin; normals towards it."""
    rng = np.random.default_rng(seed)
    if shape == "box":
        pts, nrm = _box_faces(rng, n, np.array([0.05, 0.03, 0.04]))
    elif shape == "cylinder":
        pts, nrm = _cylinder(rng, n)
    else:
        pts, nrm = _cap(rng, n)
    R = _rot(yaw, pitch)
    return _visible(pts @ R.T + np.array([0.0, 0.0, 0.8]), nrm @ R.T)


_recognition = None


def recognition_set():
    """Three shapes, six training views each ('shape_view'), and one unseen view of each as queries.  Computed once:
    {names, rows (18, 308), queries: [(xyz, nrm)], query_sigs (3, 308), expected: [shape names]}."""
    global _recognition
    if _recognition is None:
        names, rows, queries, sigs = [], [], [], []
        for si, shape in enumerate(SHAPES):
            for v in range(TRAIN_VIEWS):
                xyz, nrm = shape_view(shape, VIEW_STEP * v, 0.45, RECOGNITION_SEED + 100 * si + v)
                names.append(f"{shape}_{v}")
                rows.append(vfh(xyz, nrm)["sig"])
            xyz, nrm = shape_view(shape, VIEW_STEP * 2.5, 0.45, RECOGNITION_SEED + 100 * si + 50)
            queries.append((xyz, nrm))
            sigs.append(vfh(xyz, nrm)["sig"])
        _recognition = dict(names=names, rows=np.array(rows, F), queries=queries, query_sigs=np.array(sigs, F), expected=list(SHAPES))
    return _recognition
