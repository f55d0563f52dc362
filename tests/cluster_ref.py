"""Host references of pcl::EuclideanClusterExtraction for the cluster tests (not a test module).

reference_clusters: the graph "d2 <= r2" (float32, FLANN's order (dx*dx + dy*dy) + dz*dz, r2 = float(double(float tol)^2)) from
    cKDTree candidate pairs filtered by the exact predicate, its components (scipy.sparse.csgraph), PCL's size filter and order.
pcl_bfs: a literal port of PCL 1.8's extractEuclideanClusters (seed queue, brute-force radius search, the first sorted result
    skipped as the query) with the reverse-iterator std::sort of comparePointClusters, which is stable for up to 16 clusters.
"""
from __future__ import annotations

import numpy as np


def r2_of(tol: float) -> np.float32:
    t = float(np.float32(tol))
    return np.float32(t * t)


def flann_d2(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def order_clusters(comps, min_size: int, max_size: int):
    """comps: lists of indices.  Keep sizes in [min_size, max_size], indices ascending, order by (size desc, min index asc)."""
    keep = [np.sort(np.asarray(c, np.int64)).astype(np.int32) for c in comps if min_size <= len(c) <= max_size]
    keep.sort(key=lambda c: (-len(c), int(c[0])))
    return keep


def reference_clusters(pts, tol: float = 0.05, min_size: int = 300, max_size: int = 100000):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    pts = np.asarray(pts, np.float32)
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    fidx = np.nonzero(fin)[0]
    comps = [[int(i)] for i in np.nonzero(~fin)[0]]
    if len(fidx):
        fp = pts[fidx]
        pairs = cKDTree(fp.astype(np.float64)).query_pairs(float(np.float32(tol)) * (1 + 1e-5), output_type="ndarray")
        if len(pairs):
            ok = flann_d2(fp[pairs[:, 0]], fp[pairs[:, 1]]) <= r2_of(tol)
            pairs = pairs[ok]
        g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(fidx), len(fidx)))
        nc, lab = connected_components(g, directed=False)
        order = np.argsort(lab, kind="stable")
        bounds = np.searchsorted(lab[order], np.arange(nc + 1))
        comps += [fidx[order[bounds[k]:bounds[k + 1]]] for k in range(nc)]
    out = order_clusters(comps, min_size, max_size)
    assert sum(len(c) for c in out) <= n
    return out


def labels_of(clusters, n: int) -> np.ndarray:
    lab = np.full(n, -1, np.int32)
    for k, c in enumerate(clusters):
        lab[c] = k
    return lab


def pcl_bfs(pts, tol: float, min_size: int, max_size: int):
    """PCL 1.8 extractEuclideanClusters over a kd-tree that holds the finite points, then EuclideanClusterExtraction::extract's
    std::sort (clusters.rbegin(), clusters.rend(), comparePointClusters)."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    r2 = r2_of(tol)
    processed = np.zeros(n, bool)
    clusters = []
    for i in range(n):
        if processed[i]:
            continue
        seed_queue = [i]
        processed[i] = True
        sq_idx = 0
        while sq_idx < len(seed_queue):
            q = seed_queue[sq_idx]
            if not fin[q]:       # the tree does not hold it: no neighbours
                sq_idx += 1
                continue
            d2 = flann_d2(pts, pts[q])
            nb = np.nonzero(fin & (d2 <= r2))[0]
            nb = nb[np.lexsort((nb, d2[nb]))]      # radiusSearch, sorted by distance
            for j in nb[1:]:                        # nn_indices[0] is taken for the query itself
                if processed[j]:
                    continue
                seed_queue.append(int(j))
                processed[j] = True
            sq_idx += 1
        if min_size <= len(seed_queue) <= max_size:
            clusters.append(sorted(set(seed_queue)))
    rev = clusters[::-1]
    rev = sorted(rev, key=len)                      # stable, as libstdc++'s insertion sort is for <= 16 elements
    return [np.asarray(c, np.int32) for c in rev[::-1]]
