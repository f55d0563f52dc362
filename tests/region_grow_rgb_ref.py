"""Host reference of ope_region_grow_rgb: pcl::RegionGrowingRGB (PCL 1.7/1.8 segmentation/impl/region_growing_rgb.hpp and the
inherited parts of region_growing.hpp; normal, curvature and residual tests off) restated literally and sequentially, as DESIGN.md
§4.19 words it: the queue flood over the point edges, the segment colours, findRegionsKNN with its priority queue of (dist, t),
the first merge pass as PCL's loop over the segments, findRegionNeighbours, the sequential small-region merge, the two-pointer pass
over the empty regions and extract's size filter.  Plus the parallel forms the device uses (min-index reachability, the parent
formula), which the CPU tests compare with the literal ones, and the scenes the GPU tests run.

Inputs are arrays: points, colour words (r << 16 | g << 8 | b, top byte ignored) and the k-NN lists, which for the scenes come
from oracle.KdTree over the finite points (region_grow_ref.knn_lists).  Where PCL's result is implementation-defined the rule is
this project's: every sort by distance orders equal distances by segment index ascending, (FLT_MAX, 0) included."""
import heapq
from collections import deque

import numpy as np

from region_grow_ref import knn_lists, labels_of, offsets_of, one_way_points  # noqa: F401  (re-exported for the tests)

FLT_MAX = float(np.finfo(np.float32).max)
INT_MAX = 2 ** 31 - 1


def squared(x):
    """(float)x * (float)x in float: what PCL's setters store"""
    return float(np.float32(x) * np.float32(x))


def channels(rgb):
    rgb = np.asarray(rgb, np.uint32)
    return np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], -1).astype(np.int64)


def color_dist(a, b):
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    return int((d * d).sum())


def list_d2(pts, nbrs):
    """(dx*dx + dy*dy) + dz*dz in float, every operation rounded once, for every list entry (+inf where there is none)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    v = np.where(nbrs >= 0, nbrs, 0)
    with np.errstate(invalid="ignore"):
        d = pts[:, None, :] - pts[v]
        out = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + (d[..., 2] * d[..., 2]).astype(np.float32)).astype(np.float32)
    out[nbrs < 0] = np.inf
    return out


# ------------------------------------------------------------------------------------------------------------ step 4
def flood_segments(n, finite, edges):
    """PCL's applySmoothRegionGrowingAlgorithm with normal_flag_ false: seeds by index ascending, growRegion's queue.  edges[u]: the
    v with u -> v.  Returns the segment of every point (-1: non-finite), segments numbered in seed order."""
    seg = np.full(n, -1, np.int64)
    count = 0
    for seed in range(n):
        if not finite[seed] or seg[seed] >= 0:
            continue
        seg[seed] = count
        queue = deque([seed])
        while queue:
            u = queue.popleft()
            for v in edges[u]:
                if seg[v] < 0:
                    seg[v] = count
                    queue.append(v)
        count += 1
    return seg, count


def min_reach_segments(n, finite, edges):
    """The device's form: segment(v) = the smallest index among the points that reach v, v included (a fixed point of
    L[v] = min(L[v], L[u]) over the edges u -> v), numbered densely by seed."""
    L = np.arange(n, dtype=np.int64)
    changed = True
    while changed:
        changed = False
        for u in range(n):
            if not finite[u]:
                continue
            for v in edges[u]:
                if L[u] < L[v]:
                    L[v] = L[u]
                    changed = True
    seeds = sorted({int(L[v]) for v in range(n) if finite[v]})
    number = {s: i for i, s in enumerate(seeds)}
    return np.array([number[int(L[v])] if finite[v] else -1 for v in range(n)], np.int64), len(seeds)


# ------------------------------------------------------------------------------------------------------------ step 6
def kept_neighbours(pairs, k):
    """findRegionsKNN's cut: of {t: dist} the k smallest by (dist, t), ascending — a priority queue of pairs"""
    return heapq.nsmallest(k, ((d, t) for t, d in pairs.items()))


# ------------------------------------------------------------------------------------------------------------ step 7
def merge_a_sequential(kept, means, d2_thr, r2_thr):
    """PCL's loop over the segments.  kept[i]: [(dist, x)].  Returns (region of every segment, H)."""
    S = len(kept)
    label = [-1] * S
    H = 0
    for i in range(S):
        if label[i] < 0:
            label[i] = H
            H += 1
        for d, x in kept[i]:
            if not (d > d2_thr) and label[x] < 0 and color_dist(means[i], means[x]) < r2_thr:
                label[x] = label[i]
    return label, H


def merge_a_parent(kept, means, d2_thr, r2_thr):
    """The parallel form: parent(x) = the smallest i < x that keeps x and passes both tests; the region is the root, regions
    numbered by root ascending."""
    S = len(kept)
    parent = [-1] * S
    for x in range(S):
        cands = [i for i in range(x) if any(t == x and not (d > d2_thr) for d, t in kept[i]) and color_dist(means[i], means[x]) < r2_thr]
        if cands:
            parent[x] = min(cands)
    label, H = [-1] * S, 0
    for x in range(S):
        if parent[x] < 0:
            label[x] = H
            H += 1
        else:
            label[x] = label[parent[x]]
    return label, H


# ------------------------------------------------------------------------------------------------------------ step 10
def two_pointer_order(sizes):
    """PCL's pass that closes the empty regions: the order of the regions after it (a list of region numbers) and the number of
    swaps it made"""
    order = list(range(len(sizes)))
    swaps = 0
    i, j = 0, len(sizes) - 1
    while i < j:
        while i < j and sizes[order[i]] > 0:
            i += 1
        while i < j and sizes[order[j]] == 0:
            j -= 1
        if i != j:
            order[i], order[j] = order[j], order[i]
            swaps += 1
    return order, swaps


# ------------------------------------------------------------------------------------------------------------ the whole
def region_grow_rgb_pcl(pts, rgb, nbrs, distance_threshold=0.1, point_color_threshold=10.0, region_color_threshold=10.0, min_size=700,
                        max_size=INT_MAX, k=100):
    """RegionGrowingRGB::extract.  nbrs: (n, k) lists of original indices, -1 where none.  Returns (clusters, info): the clusters in
    PCL's order as int32 arrays of indices ascending, and a dict of what the steps did."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    finite = np.isfinite(pts).all(axis=1)
    ch = channels(rgb)
    P2, R2, D2 = squared(point_color_threshold), squared(region_color_threshold), squared(distance_threshold)
    d2 = list_d2(pts, nbrs)
    # 3. point edges
    edges = [[] for _ in range(n)]
    for u in range(n):
        if finite[u]:
            edges[u] = [int(v) for v in nbrs[u] if v >= 0 and v != u and not (color_dist(ch[u], ch[v]) > P2)]
    listed = [set(int(v) for v in nbrs[u] if v >= 0) for u in range(n)]
    one_way = sum(1 for u in range(n) for v in edges[u] if u not in listed[v])
    # 4. segments
    seg, S = flood_segments(n, finite, edges)
    # 5. segment colours
    sums = np.zeros((S, 3), np.int64)
    counts = np.zeros(S, np.int64)
    for v in range(n):
        if seg[v] >= 0:
            sums[seg[v]] += ch[v]
            counts[seg[v]] += 1
    means = [[int(np.uint32(np.float32(sums[s, c]) / np.float32(counts[s]))) for c in range(3)] for s in range(S)]
    # 6. segment neighbours: directed, over the lists of the segment's own points
    dist = [dict() for _ in range(S)]
    for u in range(n):
        if seg[u] < 0:
            continue
        for j, v in enumerate(nbrs[u]):
            if v < 0 or seg[v] == seg[u]:
                continue
            t, d = int(seg[v]), float(d2[u, j])
            if t not in dist[seg[u]] or d < dist[seg[u]][t]:
                dist[seg[u]][t] = d
    kept = [kept_neighbours(dist[s], k) for s in range(S)]
    # 7. merge A
    region, H = merge_a_sequential(kept, means, D2, R2)
    rcount = [0] * H
    members = [[] for _ in range(H)]
    for s in range(S):
        rcount[region[s]] += int(counts[s])
        members[region[s]].append(s)
    # 8. region neighbours
    lists = []
    for r in range(H):
        lst = [(d, x) for s in members[r] for d, x in kept[s] if region[x] != r]
        lists.append(sorted(lst))
    # 9. merge B
    absorbed = 0
    for r in range(H):
        if rcount[r] >= min_size:
            continue
        if not lists[r] or lists[r][0][0] == FLT_MAX:
            continue
        q = region[lists[r][0][1]]
        for s in members[r]:
            region[s] = q
            members[q].append(s)
        members[r] = []
        rcount[q] += rcount[r]
        rcount[r] = 0
        lists[q] = [(FLT_MAX, 0) if region[x] == q else (d, x) for d, x in lists[q]]
        lists[q] += [(d, x) for d, x in lists[r] if region[x] != q]
        lists[r] = []
        lists[q].sort()
        absorbed += 1
    # 10. output
    order, swaps = two_pointer_order(rcount)
    points = [[] for _ in range(H)]
    for v in range(n):
        if seg[v] >= 0:
            points[region[seg[v]]].append(v)
    clusters = [np.asarray(points[r], np.int32) for r in order if min_size <= len(points[r]) <= max_size]
    info = dict(segments=S, segment_pairs=sum(len(d) for d in dist), homogeneous_regions=H, regions_absorbed=absorbed,
                regions_before_size_filter=sum(1 for c in rcount if c > 0), one_way_edges=one_way, swaps=swaps, seg=seg, kept=kept,
                truncated=sum(1 for s in range(S) if len(dist[s]) > k), region_sizes=[len(points[r]) for r in order])
    return clusters, info


# ------------------------------------------------------------------------------------------------------------------ scenes
def word(r, g, b):
    return (int(r) << 16) | (int(g) << 8) | int(b)


def grid(nx, ny, seed, x0=0.0, y0=0.0, z=0.8, spacing=0.005):
    """a jittered planar grid at 5 mm spacing (jitter up to +-1 mm in the plane, +-0.5 mm off it), row by row"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(nx), np.arange(ny))
    p = np.stack([x0 + spacing * u.ravel(), y0 + spacing * v.ravel(), np.full(nx * ny, z)], 1)
    p[:, :2] += rng.uniform(-0.001, 0.001, (nx * ny, 2))
    p[:, 2] += rng.uniform(-0.0005, 0.0005, nx * ny)
    return p.astype(np.float32)


class Scene:
    def __init__(self, name, pts, rgb, k=100, **params):
        self.name, self.k, self.params = name, k, params
        self.pts = np.ascontiguousarray(pts, np.float32)
        self.rgb = np.ascontiguousarray(rgb, np.uint32)
        self.nbrs, self.d2 = knn_lists(self.pts, k, with_next=True)
        self._ref = {}

    def free_of_boundary_ties(self):
        """no point's k-th and (k + 1)-th neighbour distances are equal (FLANN's list would be undefined there too)"""
        a, b = self.d2[:, self.k - 1], self.d2[:, self.k]
        return not bool((np.isfinite(b) & (a == b)).any())

    def reference(self, **over):
        key = tuple(sorted(over.items()))
        if key not in self._ref:
            kw = dict(self.params)
            kw.update(over)
            self._ref[key] = region_grow_rgb_pcl(self.pts, self.rgb, self.nbrs, k=self.k, **kw)
        return self._ref[key]


def two_colours():
    pts = grid(50, 40, 1)
    rgb = np.where(pts[:, 0] < 0.1225, word(200, 30, 30), word(30, 30, 200))
    return Scene("two_colours", pts, rgb)


def chain():
    """30 stripes of 2 columns whose red steps by 8 (64 <= 100): one segment by chaining"""
    pts = grid(60, 30, 2)
    col = np.rint(pts[:, 0] / 0.005).astype(int) // 2
    rgb = np.array([word(10 + 8 * c, 90, 90) for c in col])
    return Scene("chain", pts, rgb)


def steps_of_12():
    """six stripes of 10 columns stepping by 12 (144 > 100): six segments, none merged by colour, all below min_size"""
    pts = grid(60, 30, 3)
    col = np.rint(pts[:, 0] / 0.005).astype(int) // 10
    rgb = np.array([word(40 + 12 * c, 90, 90) for c in col])
    return Scene("steps_of_12", pts, rgb)


def merge_a(distance_threshold=0.1):
    """two patches (100, 100, 100) / (107, 100, 100) across a 15 mm gap; point threshold 5 (49 > 25), region threshold 10 (49 < 100)"""
    a, b = grid(30, 30, 4), grid(30, 30, 5, x0=29 * 0.005 + 0.015)
    pts = np.concatenate([a, b])
    rgb = np.array([word(100, 100, 100)] * len(a) + [word(107, 100, 100)] * len(b))
    return Scene("merge_a" if distance_threshold == 0.1 else "distance_threshold", pts, rgb, point_color_threshold=5.0, region_color_threshold=10.0,
                 distance_threshold=distance_threshold)


def salt():
    """single points of a foreign colour inside a patch: one-point segments, absorbed by merge B"""
    pts = grid(50, 40, 6)
    rgb = np.full(len(pts), word(60, 140, 60))
    rgb[[333, 777, 1234, 1650]] = word(250, 250, 10)
    return Scene("salt", pts, rgb)


def truncation():
    """region_neighbour_number 8: a stripe bordered by more than 8 one-point segments, so that the cut to the K nearest bites.  Two of
    them, A and B, sit at exactly the same distance (2^-10 m along x) either side of one point of the stripe, nearer than anything
    else: the stripe's two nearest neighbours have equal distances, and the segment index orders them."""
    pts = grid(40, 40, 7)
    colx = np.rint(pts[:, 0] / 0.005).astype(int)
    rowy = np.rint(pts[:, 1] / 0.005).astype(int)
    rgb = np.where(colx < 20, word(60, 60, 160), word(160, 60, 60))
    salt_at = (colx == 19) & (rowy % 3 == 0)            # 14 one-point segments along the border
    rgb = np.where(salt_at, word(250, 250, 10), rgb)
    m = 20 * 40 + 10                                    # a point inside the left stripe
    x, y, z = np.float32(np.rint(pts[m, 0] * 1024) / 1024), np.float32(np.rint(pts[m, 1] * 1024) / 1024), np.float32(0.8)
    d = np.float32(2.0 ** -10)
    pts[m] = (x, y, z)
    pts = np.concatenate([pts, np.array([[x - d, y, z], [x + d, y, z]], np.float32)])
    rgb = np.concatenate([rgb, [word(250, 10, 250), word(10, 250, 250)]])
    return Scene("truncation", pts, rgb, k=8, min_size=50)


def one_way_edges():
    """an isolated point beside a dense patch: it lists the patch, the patch does not list it"""
    pts = np.concatenate([grid(40, 40, 8), np.array([[-0.05, 0.1, 0.8]], np.float32)])
    rgb = np.full(len(pts), word(90, 90, 90))
    return Scene("one_way_edges", pts, rgb)


def small_cloud(n, k=100):
    """fewer finite points than K"""
    pts = grid(10, 10, 9)[:n]
    rgb = np.where(np.arange(n) % 2 == 0, word(10, 10, 10), word(200, 200, 200))
    return Scene("small_%d" % n, pts, rgb, k=k, min_size=1)


def search_cloud(k):
    """3 000 points with 5 non-finite among them, four colours in quadrants, salt: every step runs at this K"""
    pts = grid(60, 50, 10)
    rng = np.random.default_rng(11)
    rgb = np.where(pts[:, 0] < 0.15, 1, 0) * 2 + np.where(pts[:, 1] < 0.125, 1, 0)
    rgb = np.array([word(40, 40, 40), word(40, 200, 40), word(200, 40, 40), word(40, 40, 200)])[rgb]
    rgb[rng.choice(len(pts), 40, replace=False)] = word(255, 255, 0)
    pts[[7, 500, 1501, 2222, 2999], [0, 1, 2, 0, 1]] = np.nan
    return Scene("search_k%d" % k, pts, rgb, k=k, min_size=50)
