"""Host reference of ope_region_grow: pcl::RegionGrowing (PCL 1.7/1.8 segmentation/impl/region_growing.hpp) restated literally
and sequentially — the sort of the seeds, growRegion's queue, validatePoint with its seed flag and the curvature rule,
assembleRegions and extract's size filter — plus the scenes the CPU and GPU tests share.

Inputs of the flood are arrays: points, normals, curvature and the k-NN lists.  For the scenes the lists come from oracle.KdTree
over the finite points and the normals from the oracle's normal estimation.  Two rules are this project's where PCL leaves the
matter open: equal curvatures rank by original index (std::sort's order among equals is implementation-defined), and a NaN
curvature ranks last."""
import math
from collections import deque
from functools import lru_cache

import numpy as np

import oracle

DEG = math.pi / 180.0


def cos_threshold(theta):
    """c = (float)cos((double)(float)theta): what PCL's cosf(theta_threshold_) gives wherever cosf is correctly rounded."""
    return np.float32(math.cos(float(np.float32(theta))))


def knn_lists(pts, k, with_next=False):
    """(n, k) int32: the k nearest FINITE points of every finite point (itself included), nearest first, as original indices;
    -1 where there are fewer, and in the rows of non-finite points.  with_next: also the squared distances of entries
    0 .. k (one more than the list), +inf where there is none: the boundary-tie check reads columns k - 1 and k."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    fin = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    out = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k + 1), np.inf, np.float32)
    if len(fin):
        tree = oracle.KdTree(pts[fin])
        kk = min(k + 1, len(fin))
        idx, dd, _ = tree.knn(pts[fin], kk)
        m = min(k, kk)
        out[fin, :m] = fin[idx[:, :m]]
        d2[fin, :kk] = dd
    return (out, d2) if with_next else out


def abs_dots(normals, nbrs):
    """|n_v . n_u| for every list entry, float, (x*x' + y*y') + z*z' with every operation rounded once (NaN where v = -1)."""
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    v = np.where(nbrs >= 0, nbrs, 0)
    a, b = nrm[v], nrm[:, None, :]
    with np.errstate(invalid="ignore"):
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + (a[..., 2] * b[..., 2]).astype(np.float32)
        dot = np.abs(dot.astype(np.float32))
    dot[nbrs < 0] = np.nan
    return dot


def seed_order(curvature, finite):
    """The finite points by (curvature ascending, index ascending), NaN curvatures last."""
    cur = np.asarray(curvature, np.float32)
    idx = np.nonzero(finite)[0]
    nan = np.isnan(cur[idx])
    key = np.where(nan, np.float32(np.inf), cur[idx])
    return idx[np.lexsort((idx, key, nan))]


def region_grow_pcl(pts, normals, curvature, nbrs, theta=10.0 * DEG, curvature_threshold=1.0, min_size=500, max_size=1000000):
    """applySmoothRegionGrowingAlgorithm + assembleRegions + extract's filter, literally.  Returns (clusters, margin, segments):
    the kept regions in segment order (int32 arrays of indices, ascending), the smallest | |dot| - c | over all list entries, and the
    number of segments before the filter."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    cur = np.asarray(curvature, np.float32)
    finite = np.isfinite(pts).all(axis=1)
    c = cos_threshold(theta)
    thr = np.float32(curvature_threshold)
    dots = abs_dots(normals, nbrs)
    valid = nbrs >= 0
    with np.errstate(invalid="ignore"):
        fails = dots < c                      # validatePoint: `if (dot_product < cosine_threshold_) return false`; NaN passes
        margin = np.abs(dots.astype(np.float64) - float(c))
    margin = float(np.nanmin(np.where(valid & (nbrs != np.arange(n)[:, None]), margin, np.nan))) if valid.any() and n > 1 else math.inf
    if math.isnan(margin):
        margin = math.inf
    labels = np.full(n, -1, np.int64)

    def validate_point(point, j):
        """(belongs, is_a_seed) of neighbour j of `point` (smooth mode: the normal of `point`, not of the initial seed)."""
        nghbr = nbrs[point, j]
        is_a_seed = True
        if fails[point, j]:
            return False, is_a_seed
        if cur[nghbr] > thr:                  # curvature_flag_
            is_a_seed = False
        return True, is_a_seed                # (residual_flag_ is off)

    def grow_region(initial_seed, segment):
        seeds = deque([initial_seed])
        labels[initial_seed] = segment
        while seeds:
            curr = seeds.popleft()
            for j in range(nbrs.shape[1]):
                index = nbrs[curr, j]
                if index < 0 or labels[index] != -1:
                    continue
                belongs, is_a_seed = validate_point(curr, j)
                if not belongs:
                    continue
                labels[index] = segment
                if is_a_seed:
                    seeds.append(index)

    order = seed_order(cur, finite)
    segments = 0
    for seed in order:                        # "the next unlabelled point of the sorted list"
        if labels[seed] != -1:
            continue
        grow_region(int(seed), segments)
        segments += 1
    clusters = clusters_of_labels(labels, min_size, max_size)
    return clusters, margin, segments


def clusters_of_labels(labels, min_size, max_size):
    """assembleRegions + extract: regions by label value ascending, each region's indices ascending, sizes filtered."""
    labels = np.asarray(labels)
    out = []
    keep = labels >= 0
    if not keep.any():
        return out
    idx = np.nonzero(keep)[0]
    order = np.argsort(labels[idx], kind="stable")
    srt = labels[idx][order]
    cuts = np.nonzero(np.diff(srt))[0] + 1
    for part in np.split(idx[order], cuts):
        if min_size <= len(part) <= max_size:
            out.append(part.astype(np.int32))
    return out


def labels_of(clusters, n, cap=None):
    lab = np.full(n, -1, np.int32)
    for k, c in enumerate(clusters if cap is None else clusters[:cap]):
        lab[c] = k
    return lab


def offsets_of(clusters):
    return np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ scenes
class Scene:
    """points, normals, curvature, the graph's k, and whatever the region grow takes besides."""

    def __init__(self, name, pts, normals, curvature, k, theta=10.0 * DEG, normals_k=None):
        self.name, self.k, self.theta, self.normals_k = name, k, theta, normals_k
        self.pts = np.ascontiguousarray(pts, np.float32)
        self.normals = np.ascontiguousarray(normals, np.float32)
        self.curvature = np.ascontiguousarray(curvature, np.float32)
        self.nbrs, self.d2 = knn_lists(self.pts, k, with_next=True)
        self._ref = {}

    def reference(self, min_size=1, max_size=1000000, theta=None):
        key = (min_size, max_size, theta)
        if key not in self._ref:
            self._ref[key] = region_grow_pcl(self.pts, self.normals, self.curvature, self.nbrs, self.theta if theta is None else theta, 1.0,
                                             min_size, max_size)
        return self._ref[key]


def _flat_normals(n):
    nrm = np.zeros((n, 3), np.float32)
    nrm[:, 2] = 1.0
    return nrm


def one_way_points():
    """Four collinear points at x = 0, 1, 1.1, 1.2 and k = 2.  In float, 1.1f - 1.0f == 1.2f - 1.1f exactly: the second
    neighbour of x = 1.1 would be a boundary tie, which the scenes must not have, so the last point sits one ulp below 1.2f and
    x = 1.1 lists x = 1.2.  Edges: 0 -> 1, 1 -> 1.1, 1.1 <-> 1.2; nothing leads back to x = 0."""
    x = np.array([0.0, 1.0, 1.1, 1.2], np.float32)
    x[3] = np.nextafter(x[3], np.float32(0))
    pts = np.zeros((4, 3), np.float32)
    pts[:, 0] = x
    return pts


@lru_cache(maxsize=None)
def one_way(first):
    """first: x = 0 has the smallest curvature (it takes all four); otherwise the largest (it is a region of its own)."""
    cur = np.array([0.01 if first else 0.09, 0.02, 0.03, 0.04], np.float32)
    return Scene("one_way_first" if first else "one_way_last", one_way_points(), _flat_normals(4), cur, 2)


CHAIN_N = 2000


@lru_cache(maxsize=None)
def chain(with_links):
    """2 000 points along a line, the spacing growing by 1 % per step: with k = 2 every point but the first lists its
    PREDECESSOR, so every link i -> i - 1 is one-way, except the closest pair 0 <-> 1 (the closest pair of any point set is
    mutual).  with_links: the ranks ascend in the direction of the links (from the far end towards the start): one region,
    reached hop by hop.  Otherwise against them: nothing flows, 1 998 singletons and the pair {0, 1}."""
    step = 1e-3 * 1.01 ** np.arange(CHAIN_N - 1, dtype=np.float64)
    pts = np.zeros((CHAIN_N, 3), np.float32)
    pts[1:, 0] = np.cumsum(step)
    i = np.arange(CHAIN_N, dtype=np.float64)
    cur = (1e-4 * (1 + (CHAIN_N - 1 - i if with_links else i))).astype(np.float32)
    return Scene("chain_with" if with_links else "chain_against", pts, _flat_normals(CHAIN_N), cur, 2)


CREASE_SEED = 2      # the first seeds whose scene meets the three input conditions (test_region_grow_ref.py)
SCENE4_SEED = 485


@lru_cache(maxsize=None)
def crease():
    """Two 40 x 40 noisy planar patches meeting at 30 degrees; oracle normals at k = 10.  The second patch's first row lies on the
    crease, and the lattice is a little denser along the crease than across it, so that the 10 nearest of a point stay within
    its own row and the two next to it: the rows beside the crease keep their patch's normal, the row on it sits halfway (15
    degrees from either), and the patches part at 10 degrees and join at 40.  (On a square lattice with the crease between two
    rows the normals turn in four steps of under 10 degrees and the patches join at 10 degrees too.)  The scene sits near the
    origin: the oracle's single-pass float covariance returns a curvature of exactly 0 for flat patches a metre away."""
    rng = np.random.default_rng(CREASE_SEED)
    hu, hv = 0.01, 0.008
    u, v = np.meshgrid(np.arange(40) * hu, np.arange(40) * hv, indexing="ij")
    a = np.stack([-(u.ravel() + hu), v.ravel(), np.zeros(1600)], 1)
    t = 30.0 * DEG
    b = np.stack([u.ravel() * math.cos(t), v.ravel(), u.ravel() * math.sin(t)], 1)
    pts = np.concatenate([a, b]) + rng.normal(0, 3.0e-4, (3200, 3)) + np.array([0.0, -0.16, 0.1])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    nrm, cur = oracle.normals_knn(pts, 10)
    return Scene("crease", pts, nrm, cur, 10, normals_k=10)


@lru_cache(maxsize=None)
def scene4():
    """About 6 000 points: a sphere cap (the largest region, of uniform curvature: its seed ranks after the flat faces'), the
    three faces of a box corner, and scattered specks; oracle normals at k = 30."""
    rng = np.random.default_rng(SCENE4_SEED)
    # sphere cap: radius 0.12, polar angle up to 60 degrees, 3 000 points
    m = 3000
    ct = rng.uniform(math.cos(60 * DEG), 1.0, m)
    ph = rng.uniform(0, 2 * math.pi, m)
    st = np.sqrt(1 - ct * ct)
    cap = 0.12 * np.stack([st * np.cos(ph), st * np.sin(ph), -ct], 1) + np.array([-0.2, 0.0, 0.45])
    # box corner: three faces of 0.15 m, a 28 x 28 jittered lattice each
    g = (np.arange(28) + 0.5) * (0.15 / 28)
    p, q = [w.ravel() for w in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(p)
    faces = [np.stack([p, q, z], 1), np.stack([p, z, q], 1), np.stack([z, p, q], 1)]
    faces = [f + rng.uniform(-0.001, 0.001, f.shape) * (np.abs(f) > 0) for f in faces]
    rot = _rotation(np.array([1.0, 0.4, 0.2]), 0.6)
    box = np.concatenate(faces) @ rot.T + np.array([0.1, -0.05, 0.3])
    specks = rng.uniform([-0.5, -0.4, 0.1], [0.5, 0.4, 0.6], (130, 3))
    pts = np.concatenate([cap, box, specks]) + rng.normal(0, 5.0e-4, (m + 3 * 784 + 130, 3))
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    nrm, cur = oracle.normals_knn(pts, 30)
    return Scene("scene4", pts, nrm, cur, 15, normals_k=30)


def _rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def gpu_scenes():
    return [one_way(True), one_way(False), chain(True), chain(False), crease(), scene4()]
