"""Batched final pose at the reference's size (C1): one ope_final_pose_batch call against the composition it replaces and
against K sequential estimateFinalPose chains.

Inputs are those of tools/coarse_batch_bench.py (its candidates(): the decimated drill model and K raw clusters, the C1 scene
cluster first).  The composition is what a caller had to write before the call existed, in four phases timed one by one:
  coarse   one ope_coarse_pose_batch;
  inputs   per cluster, the model moved by its coarse pose on the host (float32, transformPointCloud's order) and, for it and
           for the cluster: NaN removal, upload, uniform_sampling(0.008), normals(30), NaN-normal drop, upload;
  index    per cluster, build_index of the fine target;
  icp      one icp_batch with getFitnessScore, then the selection rule (rosinterface.cpp:256).
K sequential chains are what the facade runs per estimateFinalPose call, K times without stopping early: the single-path coarse chain (features of both sides,
index, SAC-IA), the fine inputs, the index, ope_icp_run and ope_fitness.

Host clock around each synchronous call, 5 warm-up and 20 timed repetitions, median and min-max.

    python tools/final_batch_bench.py [--ks 1,8,32] [--warmup 5] [--reps 20] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import coarse_batch_bench as cbb  # noqa: E402  (candidates, timed, the single-path chains)

ope = importlib.import_module("object-pose-estimation_amd")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
DBL_MAX = cbb.DBL_MAX


def transform_f32(T, p):
    M = np.asarray(T, np.float32)
    out = p.copy()
    for r in range(3):
        out[:, r] = ((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]
    return out


def stat(t):
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = ope.Context(0)
    model, _ = pcd.read_pcd(os.path.join(cbb.GOLD, "drill_model_decimated.pcd"))
    model = np.ascontiguousarray(model, np.float32)
    ks = [int(k) for k in a.ks.split(",")]
    clouds = cbb.candidates(max(ks))
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    fp = ope.default_icp_params(**cbb.FINE)
    rows = []
    for k in ks:
        sub, sub_clouds = cs[:k], clouds[:k]

        def composition(times=None):
            t0 = time.perf_counter()
            coarse = ctx.coarse_pose_batch(m, sub)
            t1 = time.perf_counter()
            src = [ctx.upload(*cbb.fine_inputs(ctx, transform_f32(r.T, model))) for r in coarse]
            tgt = [ctx.upload(*cbb.fine_inputs(ctx, c)) for c in sub_clouds]
            t2 = time.perf_counter()
            ix = [ctx.build_index(t) for t in tgt]
            t3 = time.perf_counter()
            out = ctx.icp_batch(src, ix, fp, None, fitness_max_range=DBL_MAX)
            sel = next((j for j, r in enumerate(out) if r.fitness < 1e-4 or r.align_strength > 0.4), -1)
            t4 = time.perf_counter()
            if times is not None:
                for name, d in zip(("coarse", "inputs", "index", "icp"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    times.setdefault(name, []).append(d * 1e3)
                times.setdefault("total", []).append((t4 - t0) * 1e3)
            return sel

        def sequential():
            # all K chains (the batch does not stop early either); the first accepted cluster
            sel = -1
            for i, (c, raw) in enumerate(zip(sub, sub_clouds)):
                T, _, _ = cbb.chain(ctx, m, c, 1 + i)   # (the model's features too: every coarse call computes them)
                s = ctx.upload(*cbb.fine_inputs(ctx, transform_f32(T, model)))
                ix = ctx.build_index(ctx.upload(*cbb.fine_inputs(ctx, raw)))
                r = ctx.icp(s, ix, fp)
                fit = ctx.fitness(s, ix, r.T)[0]
                if sel < 0 and (fit < 1e-4 or r.align_strength > 0.4):
                    sel = i
            return sel

        for _ in range(a.warmup):
            composition()
        ph = {}
        for _ in range(a.reps):
            composition(ph)
        tb = cbb.timed(lambda: ctx.final_pose_batch(m, sub), a.warmup, a.reps)
        ts = cbb.timed(sequential, a.warmup, a.reps)
        res, sel = ctx.final_pose_batch(m, sub)
        row = dict(K=k, final_batch_ms=tb, composition_ms=stat(ph["total"]), phases_ms={n: stat(v) for n, v in ph.items() if n != "total"},
                   sequential_ms=ts, selected=sel, selected_composition=composition(), selected_sequential=sequential())
        rows.append(row)
        p = row["phases_ms"]
        print(f"K={k:3d} | final_pose_batch {tb[0]:8.3f} ms [{tb[1]:.3f}-{tb[2]:.3f}] | composition {row['composition_ms'][0]:8.3f} ms "
              f"[{row['composition_ms'][1]:.3f}-{row['composition_ms'][2]:.3f}] (coarse {p['coarse'][0]:.3f}, inputs {p['inputs'][0]:.3f}, "
              f"index {p['index'][0]:.3f}, icp {p['icp'][0]:.3f}) | {k} sequential {ts[0]:8.3f} ms [{ts[1]:.3f}-{ts[2]:.3f}] | "
              f"selected {sel} / {row['selected_composition']} / {row['selected_sequential']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
