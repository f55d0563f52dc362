#!/usr/bin/env python3
"""Times ope_region_grow on a 307 200-point synthetic frame without a table: the room of tests/peel_scenes.py (three planar
patches, four blobs, noise; three quarters of the points) plus curved objects standing free (two spheres and a cylinder, 0.3 mm
noise).  The call estimates the normals itself (k = 30) and runs with the reference's parameters.  The comparison line is the
composition a user has without it: ope_normals, ope_knn_search (k = 15) with its download, then the flood on the host, rewritten
for numpy / scipy as the labelling the device computes (the strongly connected components of the edge graph, then the smallest
rank over all ancestors by propagation over the condensed graph).  Host clock around synchronised calls, median [min-max] ms over
--reps calls after --warmup (the composition: --host-reps); launches, synchronisations, sweeps and one-way edges from the stats;
the per-kernel times of one profiled call (ope_profile_kernels), summed into normals, graph, labelling and output.  One JSON line."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ope = importlib.import_module("object-pose-estimation_amd")
from peel_scenes import SCENES, room_scene  # noqa: E402

GROUPS = {"graph": ("rg_graph_kernel",),
          "labelling": ("rg_key_kernel", "rg_sort_ranks", "rg_rank_kernel", "rg_mutual_kernel", "rg_flatten_kernel", "rg_sweep_kernel"),
          "output": ("rg_pos_kernel", "rg_size_kernel", "rg_flag_kernel", "rg_scan_regions", "rg_order_kernel", "rg_scan_offsets", "rg_label_kernel",
                     "rg_sort_labels")}


def frame(points, seed=7):
    rng = np.random.default_rng(seed)
    n_room = int(points * 0.75)
    room = room_scene(SCENES["three"], scale=n_room / 20000.0)
    left = points - len(room)
    parts = []
    for share, centre, radius in ((0.4, (-0.2, -0.1, 1.0), 0.12), (0.3, (0.15, -0.25, 0.85), 0.09)):
        m = int(left * share)
        v = rng.normal(size=(m, 3))
        parts.append(np.asarray(centre) + radius * v / np.linalg.norm(v, axis=1, keepdims=True))
    m = left - sum(len(p) for p in parts)
    a, h = rng.uniform(0, 2 * math.pi, m), rng.uniform(-0.15, 0.15, m)
    parts.append(np.column_stack([0.25 + 0.06 * np.cos(a), h - 0.1, 1.2 + 0.06 * np.sin(a)]))
    curved = np.concatenate(parts) + rng.normal(0, 3e-4, (left, 3))
    pts = np.concatenate([room, curved.astype(np.float32)])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def host_flood(nrm, cur, nbrs, theta, min_size, max_size):
    """The labelling on the host: edges by the float predicate, scipy's strongly connected components, the smallest rank over all
    ancestors by propagation over the condensed graph, the size filter and the seed order."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n, k = nbrs.shape
    c = np.float32(math.cos(float(np.float32(theta))))
    v = np.where(nbrs >= 0, nbrs, 0)
    a, b = nrm[v], nrm[:, None, :]
    dot = np.abs(((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + (a[..., 2] * b[..., 2]).astype(np.float32)).astype(np.float32))
    ok = (nbrs >= 0) & ~(dot < c)
    u = np.repeat(np.arange(n), k)[ok.ravel()]
    w = nbrs.ravel()[ok.ravel()]
    rank = np.empty(n, np.int64)
    rank[np.lexsort((np.arange(n), cur))] = np.arange(n)
    _, comp = connected_components(csr_matrix((np.ones(len(u), np.int8), (u, w)), shape=(n, n)), connection="strong")
    L = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(L, comp, rank)
    cu, cw = comp[u], comp[w]
    cross = cu != cw
    cu, cw = cu[cross], cw[cross]
    while True:
        new = L.copy()
        np.minimum.at(new, cw, L[cu])
        if (new == L).all():
            break
        L = new
    lab = L[comp]
    seeds, counts = np.unique(lab, return_counts=True)
    keep = (counts >= min_size) & (counts <= max_size)
    return [np.flatnonzero(lab == s) for s in seeds[keep]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=307200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    ctx = ope.Context(0)
    pts = frame(a.points)
    cloud = ctx.upload(pts)
    p = ope.default_region_params()
    seen = {}

    def device():
        clusters, _, stats = ctx.region_grow(cloud, p)
        seen["device"] = (clusters, stats)

    def composed():
        c2 = ctx.upload(pts)
        nrm, cur = ctx.normals(c2, p.normals_k)
        ix = ctx.build_index(c2)
        nbrs, _ = ctx.knn(c2, ix, p.number_of_neighbours)
        seen["composed"] = host_flood(np.asarray(nrm, np.float32), np.asarray(cur, np.float32), np.asarray(nbrs), p.smoothness_threshold,
                                      p.min_size, p.max_size)

    out = {"points": int(cloud.n)}
    out["region_grow"] = timed(device, a.reps, a.warmup)
    clusters, stats = seen["device"]
    out["region_grow"].update(regions=len(clusters), sizes=[len(c) for c in clusters[:8]], **stats)
    out["composition"] = timed(composed, a.host_reps, 1)
    host = seen["composed"]
    out["composition"].update(regions=len(host), same_clusters=[c.tolist() for c in host] == [c.tolist() for c in clusters])
    out["ranges_overlap"] = not (out["region_grow"]["max_ms"] < out["composition"]["min_ms"])
    ctx.profile_kernels(True)
    device()
    prof = ctx.profile_kernels_read()
    ctx.profile_kernels(False)
    us = {k: round(v["ms"] * 1e3, 1) for k, v in prof.items() if isinstance(v, dict)}
    out["kernels_us"] = us
    split = {g: round(sum(us.get(k, 0.0) for k in names), 1) for g, names in GROUPS.items()}
    split["normals"] = round(sum(t for k, t in us.items() if not k.startswith("rg_")), 1)
    out["split_us"] = split
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
