#!/usr/bin/env python3
"""Times ope_vfh_recognise on K raw candidate clusters of the reference's size (C1: the inputs of tools/coarse_batch_bench.py, the
drill scene cluster, moved copies and synthetic distractors of ~4 000 points) against a table of --rows trained signatures:
  batched      one ope_vfh_recognise call over all K clusters, normals already on the clouds;
  loop         K single-cluster ope_vfh_recognise calls;
  host         the path the call replaces: ope_normals on the device per cluster, download, the VFH histogram in numpy
               (vectorised fp64, the layout of tests/vfh_ref.py) and the chi-square search in numpy;
  estimate     the batched call on clouds WITHOUT normals (one ope_normals per cluster inside the call);
  replay       the flat worst case on its own: one cluster of --flat points with equal normals, so that one viewpoint bin takes
               every addition; vfh_signature_kernel's time from ope_profile_kernels.
Host clock around synchronised calls, median [min-max] ms over --reps calls after --warmup; per-kernel times of one profiled
batched call.  One JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
ope = importlib.import_module("object-pose-estimation_amd")
import coarse_batch_bench as cbb  # noqa: E402  (candidates)

D_PI = float(np.float32(1.0) / (np.float32(2.0) * np.float32(math.pi)))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def host_vfh(xyz, nrm):
    """The 308-bin signature in vectorised numpy (fp64 features, count * increment): what a user computes without the call."""
    p, n = xyz.astype(np.float64), nrm.astype(np.float64)
    c, nc = p.mean(0), n.mean(0)
    dvp = np.append(-c, -1.0)
    dvp /= np.linalg.norm(dvp)
    d = p - c
    f4 = np.linalg.norm(d, axis=1)
    ok = f4 > 0
    f4 = np.where(ok, f4, 1.0)
    a1, a2 = d @ nc / f4, np.einsum("ij,ij->i", n, d) / f4
    swap = np.arccos(np.clip(np.abs(a1), 0, 1)) > np.arccos(np.clip(np.abs(a2), 0, 1))
    A = np.where(swap[:, None], n, nc[None, :])
    B = np.where(swap[:, None], nc[None, :], n)
    D = np.where(swap[:, None], -d, d)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(D, A)
    vn = np.linalg.norm(v, axis=1)
    ok &= vn > 0
    v /= np.where(vn > 0, vn, 1.0)[:, None]
    w = np.cross(A, v)
    f2 = np.einsum("ij,ij->i", v, B)
    f1 = np.arctan2(np.einsum("ij,ij->i", w, B), np.einsum("ij,ij->i", A, B))
    sig = np.zeros(308, np.float32)
    m = len(p)
    for off, u in ((0, 45 * ((f1 + math.pi) * D_PI)), (45, 45 * ((f2 + 1) * 0.5)), (90, 45 * ((f3 + 1) * 0.5))):
        b = np.clip(np.floor(u[ok]), 0, 44).astype(np.int64)
        sig[off:off + 45] = np.bincount(b, minlength=45) * np.float32(100.0 / max(m - 1, 1))
    b = np.clip(np.floor(((n @ dvp[:3] + 1) * 0.5) * 128), 0, 127).astype(np.int64)
    sig[180:] = np.bincount(b, minlength=128) * np.float32(100.0 / m)
    return sig


def host_chi2(rows, q, k):
    s = rows + q
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(s > 0, (rows - q) ** 2 / s, 0).sum(1)
    return np.argsort(d, kind="stable")[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--flat", type=int, default=307200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    ctx = ope.Context(0)
    raw = cbb.candidates(max(a.clusters))
    rng = np.random.default_rng(0)
    out = {"rows": a.rows, "sizes": [len(c) for c in raw[:8]]}
    # the table: the clusters' own signatures first, then perturbed copies up to --rows
    with_n = [ctx.upload(c) for c in raw]
    sigs = ctx.vfh(with_n)   # (leaves the normals on the clouds)
    rows = np.concatenate([sigs, np.abs(sigs[rng.integers(0, len(sigs), max(a.rows - len(sigs), 0))] +
                                        rng.normal(0, 0.5, (max(a.rows - len(sigs), 0), 308))).astype(np.float32)])[:a.rows]
    db = ctx.vfh_db(rows)
    for k in a.clusters:
        cl = with_n[:k]
        r = {"points": int(sum(c.n for c in cl))}
        r["batched"] = timed(lambda: ctx.vfh_recognise(db, cl), a.reps, a.warmup)
        r["batched"].update(ctx.vfh_stats())
        r["loop"] = timed(lambda: [ctx.vfh_recognise(db, [c]) for c in cl], a.reps, a.warmup)

        def host():
            for c in raw[:k]:
                cd = ctx.upload(c)
                nrm, _ = ctx.normals(cd, 30)
                host_chi2(rows, host_vfh(c, np.asarray(nrm, np.float32)), 15)

        def estimate():
            ctx.vfh_recognise(db, [ctx.upload(c) for c in raw[:k]])

        r["host"] = timed(host, a.host_reps, 1)
        r["estimate"] = timed(estimate, a.host_reps, 1)
        r["batched_faster_than_loop"] = r["batched"]["max_ms"] < r["loop"]["min_ms"]
        ctx.profile_kernels(True)
        ctx.vfh_recognise(db, cl)
        r["kernels_us"] = {n: round(v["ms"] * 1e3, 1) for n, v in ctx.profile_kernels_read().items()}
        ctx.profile_kernels(False)
        out[f"clusters_{k}"] = r
    # the replay loop at its longest
    xy = rng.uniform(-0.3, 0.3, (a.flat, 2))
    flat = ctx.upload(np.column_stack([xy, np.full(a.flat, 0.9)]).astype(np.float32), np.tile(np.array([0, 0, -1], np.float32), (a.flat, 1)))
    ts = []
    for _ in range(a.warmup + a.reps):
        ctx.profile_kernels(True)
        ctx.vfh([flat])
        ts.append({n: v["ms"] * 1e3 for n, v in ctx.profile_kernels_read().items()})
        ctx.profile_kernels(False)
    ts = ts[a.warmup:]
    out["flat"] = {"points": a.flat,
                   "call": timed(lambda: ctx.vfh([flat]), a.reps, a.warmup),
                   "kernels_us": {n: {"median": round(statistics.median(t[n] for t in ts), 1), "min": round(min(t[n] for t in ts), 1),
                                      "max": round(max(t[n] for t in ts), 1)} for n in ts[0]}}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
