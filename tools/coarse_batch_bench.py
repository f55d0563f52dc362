"""Batched coarse stage at the reference's size (C1): one ope_coarse_pose_batch call against K single-path coarse chains.

Inputs are raw clouds, as estimateCoarsePose gets them: the decimated drill model (3 946 points, 634 key points at 1 cm) and K
candidate clusters, the C1 scene cluster (1 642 points, 361 key points) plus seeded, rigidly moved copies of it and synth
distractors.  A single-path chain is what the facade runs per coarse call (poseestimator.cpp:16-73): uniform sampling, normals,
FPFH, index and SAC-IA, the model side included; "model once" runs the model side once and the cluster side K times.  The chains
go through the Python binding like the batch call.

Host clock around each synchronous call, 5 warm-up and 20 timed repetitions, median and min-max.  Kernel times come from a
separate run under rocprofv3 --kernel-trace --stats (--reps 3).  --chain also times the whole candidate loop: the batched coarse
stage, the per-candidate fine inputs (NaN removal, uniform sampling at 8 mm, normals) and their indexes, one icp_batch with
getFitnessScore, and the selection rule (rosinterface.cpp:243-262).

    python tools/coarse_batch_bench.py [--ks 1,8,32] [--warmup 5] [--reps 20] [--chain] [--json out.json]
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
ope = importlib.import_module("object-pose-estimation_amd")
synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(ROOT, "tests", "golden")
DBL_MAX = float(np.finfo(np.float64).max)
FINE = dict(max_iterations=100, transformation_epsilon=1e-8, euclidean_fitness_epsilon=1e-8, corr_mode=1, k_normal_shooting=20,
            use_surface_normal_rej=1, surface_normal_thr=0.7)


def candidates(k, seed=0):
    """Raw clusters: the scene cluster first, then moved copies (odd positions) and synth distractors (even positions)."""
    scene = np.load(os.path.join(GOLD, "drill_scene_c1.npz"))["scene"]
    rng = np.random.default_rng(seed)
    c = scene.mean(0)
    out = []
    for j in range(k):
        if j == 0:
            cloud = scene
        elif j % 2:
            R = synth.rot_xyz(*(rng.uniform(30, 90, 3) * rng.choice([-1, 1], 3))).astype(np.float32)
            cloud = ((scene - c) @ R.T + c + rng.uniform(0.08, 0.15, 3) * rng.choice([-1, 1], 3)).astype(np.float32)
        else:
            d = synth.model_surface(4000, seed=100 + j) * np.float32(rng.uniform(0.6, 1.2))
            cloud = (d - d.mean(0) + c + rng.uniform(-0.01, 0.01, 3)).astype(np.float32)
        out.append(np.ascontiguousarray(cloud, np.float32))
    return out


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def features(ctx, cloud):
    """The single path's coarse features of one uploaded cloud: key-point cloud (with normals) and its FPFH rows."""
    kc, _ = ctx.uniform_sampling_cloud(cloud, 0.01)
    ctx.normals(kc, 30, fetch=False)
    return kc, ctx.fpfh(kc, 0.03)


def chain(ctx, model, cluster, seed, model_feats=None):
    """One facade-style coarse call: features of both sides (model side unless given), the cluster's index, SAC-IA."""
    mk, mf = model_feats or features(ctx, model)
    tk, tf = features(ctx, cluster)
    return ctx.sacia(mk, mf, tk, ctx.build_index(tk), tf, ope.default_sacia_params(seed=seed))


def fine_inputs(ctx, cloud):
    cloud = cloud[np.isfinite(cloud).all(1)]
    keys = cloud[ctx.uniform_sampling(ctx.upload(cloud), 0.008)]
    nrm, _ = ctx.normals(ctx.upload(keys), 30)
    ok = np.isfinite(nrm).all(1)
    return keys[ok], nrm[ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", action="store_true", help="also time the whole candidate loop (coarse batch -> fine inputs -> icp_batch)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = ope.Context(0)
    model, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    model = np.ascontiguousarray(model, np.float32)
    ks = [int(k) for k in a.ks.split(",")]
    clouds = candidates(max(ks))
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    res = ctx.coarse_pose_batch(m, cs)
    print(f"model {len(model)} points, {res[0].n_src_keys} key points; clusters {min(len(c) for c in clouds)}-"
          f"{max(len(c) for c in clouds)} points, {min(r.n_tgt_keys for r in res)}-{max(r.n_tgt_keys for r in res)} key points")
    mfeat = features(ctx, m)
    fp = ope.default_icp_params(**FINE)
    rows = []
    for k in ks:
        sub = cs[:k]
        tb = timed(lambda: ctx.coarse_pose_batch(m, sub), a.warmup, a.reps)
        ts = timed(lambda: [chain(ctx, m, c, 1 + i) for i, c in enumerate(sub)], a.warmup, a.reps)
        to = timed(lambda: [chain(ctx, m, c, 1 + i, mfeat) for i, c in enumerate(sub)], a.warmup, a.reps)
        row = dict(K=k, batch_ms=tb, chains_ms=ts, chains_model_once_ms=to, speedup=ts[0] / tb[0], speedup_model_once=to[0] / tb[0])
        line = (f"K={k:3d} | batch {tb[0]:8.3f} ms [{tb[1]:.3f}-{tb[2]:.3f}] | {k} chains {ts[0]:8.3f} ms [{ts[1]:.3f}-{ts[2]:.3f}] "
                f"x{row['speedup']:.1f} | model once {to[0]:8.3f} ms [{to[1]:.3f}-{to[2]:.3f}] x{row['speedup_model_once']:.1f}")
        if a.chain:
            sub_clouds = clouds[:k]

            def loop():
                coarse = ctx.coarse_pose_batch(m, sub)
                src = [ctx.upload(*fine_inputs(ctx, (model.astype(np.float64) @ r.T[:3, :3].T.astype(np.float64)
                                                      + r.T[:3, 3]).astype(np.float32))) for r in coarse]
                ix = [ctx.build_index(ctx.upload(*fine_inputs(ctx, c))) for c in sub_clouds]
                out = ctx.icp_batch(src, ix, fp, None, fitness_max_range=DBL_MAX)
                return next((j for j, r in enumerate(out) if r.fitness < 1e-4 or r.align_strength > 0.4), None)

            tl = timed(loop, a.warmup, a.reps)
            row["candidate_loop_ms"] = tl
            row["selected"] = loop()
            line += f" | candidate loop {tl[0]:8.3f} ms [{tl[1]:.3f}-{tl[2]:.3f}] (selected {row['selected']})"
        rows.append(row)
        print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
