#!/usr/bin/env python3
"""Times ope_prerejective on the C1 key points (the decimated drill model against the C1 scene cluster: uniform sampling at 1 cm,
normals with k = 30, FPFH at 3 cm, as estimateCoarsePose makes them) at the reference's parameters (50 000 iterations of 3
samples, randomness 5, similarity 0.8, distance 0.15, fraction 0.25):
  prerejective   the call, with and without the inlier list; its kernels from ope_profile_kernels; survivors, launches, syncs;
  sacia          ope_sacia at the reference's parameters (400 x 5) on the same clouds: what a coarse call costs today;
  reference      tests/prerejective_ref.py on the CPU (--ref-iterations of the 50 000, one run), scaled to 50 000.
Host clock around synchronised calls, median [min-max] ms over --reps calls after --warmup.  One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ope = importlib.import_module("object-pose-estimation_amd")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(ROOT, "tests", "golden")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-iterations", type=int, default=5000, help="0 skips the CPU reference")
    a = ap.parse_args()
    ctx = ope.Context(0)
    model, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    g = np.load(os.path.join(GOLD, "drill_scene_c1.npz"))
    keys, feats = [], []
    for cloud in (np.ascontiguousarray(model, np.float32), np.ascontiguousarray(g["scene"], np.float32)):
        k = cloud[ctx.uniform_sampling(ctx.upload(cloud), 0.01)]
        c = ctx.upload(k)
        ctx.normals(c, 30)
        keys.append(k)
        feats.append(ctx.fpfh(c, 0.03))
    s, t = ctx.upload(keys[0]), ctx.upload(keys[1])
    ix = ctx.build_index(t)
    p = ope.default_prerejective_params(max_iterations=a.iterations)
    out = {"source_keys": len(keys[0]), "target_keys": len(keys[1]), "iterations": a.iterations}
    r = ctx.prerejective(s, feats[0], t, ix, feats[1], p)
    st = ctx.prerejective_stats()
    out["result"] = {"converged": r.converged, "best_iteration": r.best_iteration, "inliers": r.inliers, "error": r.error,
                     "frobenius_to_gt": round(float(np.linalg.norm(r.T.astype(np.float64) - g["gt"])), 4)}
    out["stats"] = dict(st, survivor_share=round(st["survivors"] / st["iterations"], 4))
    out["prerejective"] = timed(lambda: ctx.prerejective(s, feats[0], t, ix, feats[1], p), a.reps, a.warmup)
    out["prerejective_with_inliers"] = timed(lambda: ctx.prerejective(s, feats[0], t, ix, feats[1], p, with_inliers=True), a.reps, a.warmup)
    ts = []
    for _ in range(a.warmup + a.reps):
        ctx.profile_kernels(True)
        ctx.prerejective(s, feats[0], t, ix, feats[1], p, with_inliers=True)
        ts.append({n: v["ms"] * 1e3 for n, v in ctx.profile_kernels_read().items()})
        ctx.profile_kernels(False)
    ts = ts[a.warmup:]
    out["kernels_us"] = {n: {"median": round(statistics.median(x[n] for x in ts), 1), "min": round(min(x[n] for x in ts), 1),
                             "max": round(max(x[n] for x in ts), 1)} for n in ts[0]}
    sp = ope.default_sacia_params()
    out["sacia"] = timed(lambda: ctx.sacia(s, feats[0], t, ix, feats[1], sp), a.reps, a.warmup)
    if a.ref_iterations > 0:
        import prerejective_ref as ref
        t0 = time.perf_counter()
        w = ref.align(keys[0], feats[0], keys[1], feats[1], max_iterations=a.ref_iterations)
        dt = time.perf_counter() - t0
        out["reference_cpu"] = {"iterations": a.ref_iterations, "seconds": round(dt, 2), "survivors": int(w["survived"].sum()),
                                "seconds_scaled_to_iterations": round(dt * a.iterations / a.ref_iterations, 1)}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
