"""Batched correspondence coarse stage at the reference's size (C1) and parameters (CorrespondenceRejectorSampleConsensus with 10 000
iterations at 0.08): one ope_corr_sac_pose_batch call against the loop it replaces.

Inputs are those of tools/coarse_batch_bench.py (its candidates(): the decimated drill model, 634 key points, and K raw clusters of
the C1 candidate size, the scene cluster first).
  batch      (a) one corr_sac_pose_batch over the K uploaded clusters;
  loop       (b) per cluster, in the same process: the single path's uniform sampling, normals, FPFH (on the device, no upload of
             key points needed) and one coarse_pose_correspondences (ope_feature_correspondences + ope_corr_sac); the model's features
             are computed ONCE outside the loop, which favours the loop (the facade computes them per coarse call);
  final      one final_pose_batch_correspondences against K estimateFinalPose chains (loop (b) with the model's features per call,
             then the fine inputs, the index, ope_icp_run and ope_fitness), without stopping early;
  kernels    per-kernel times of (a) from ope_profile_kernels, in microseconds;
  host       the host's share of (a): the time of a profiled call minus the sum of its kernel times (the draws are serial on the
             host; copies, launches and synchronisations are in it too).
Host clock around each synchronous call, --warmup and --reps repetitions, median [min-max] ms.

    python tools/corr_sac_batch_bench.py [--ks 1,8,32] [--iterations 10000] [--threshold 0.08] [--warmup 5] [--reps 20] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import coarse_batch_bench as cbb  # noqa: E402  (candidates, timed, the single path's features)
import final_batch_bench as fbb   # noqa: E402  (transform_f32)

ope = importlib.import_module("object-pose-estimation_amd")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--threshold", type=float, default=0.08)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-final", action="store_true", help="skip the two final-pose forms")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = ope.Context(0)
    model, _ = pcd.read_pcd(os.path.join(cbb.GOLD, "drill_model_decimated.pcd"))
    model = np.ascontiguousarray(model, np.float32)
    ks = [int(k) for k in a.ks.split(",")]
    clouds = cbb.candidates(max(ks))
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    p = ope.default_corr_sac_params(max_iterations=a.iterations, inlier_threshold=a.threshold)
    fp = ope.default_icp_params(**cbb.FINE)
    mfeat = cbb.features(ctx, m)
    rows = []

    def single(c, model_feats=None):
        mk, mf = model_feats or cbb.features(ctx, m)
        tk, tf = cbb.features(ctx, c)
        return ctx.coarse_pose_correspondences(mk, mf, tk, tf, p)

    for k in ks:
        sub, sub_clouds = cs[:k], clouds[:k]
        res = ctx.corr_sac_pose_batch(m, sub, None, p)
        st = ctx.corr_sac_batch_stats()
        loop_res = [single(c, mfeat) for c in sub]
        same = sum(int(r.best == s.best and r.inliers == s.inliers and r.T_svd.tobytes() == s.T_svd.tobytes()) for r, s in zip(res, loop_res))
        tb = cbb.timed(lambda: ctx.corr_sac_pose_batch(m, sub, None, p), a.warmup, a.reps)
        tl = cbb.timed(lambda: [single(c, mfeat) for c in sub], a.warmup, a.reps)
        # per-kernel times of (a), and the host's share: the call minus its kernels
        ks_us, host = [], []
        for _ in range(a.warmup + a.reps):
            ctx.profile_kernels(True)
            t = cbb.timed(lambda: ctx.corr_sac_pose_batch(m, sub, None, p), 0, 1)[0]
            rec = ctx.profile_kernels_read()
            ctx.profile_kernels(False)
            ks_us.append({n: v["ms"] * 1e3 for n, v in rec.items()})
            host.append(t - sum(v["ms"] for v in rec.values()))
        ks_us, host = ks_us[a.warmup:], host[a.warmup:]
        kern = {n: round(statistics.median(x.get(n, 0.0) for x in ks_us), 1) for n in ks_us[0]}
        row = dict(K=k, iterations=a.iterations, stats=st, poses_equal_to_loop=same, batch_ms=tb, loop_ms=tl, speedup=tl[0] / tb[0],
                   ranges_apart=tb[2] < tl[1], kernels_us=kern, kernels_total_ms=round(sum(kern.values()) / 1e3, 3),
                   host_share_ms=(round(statistics.median(host), 3), round(min(host), 3), round(max(host), 3)))
        line = (f"K={k:3d} | batch {tb[0]:8.3f} ms [{tb[1]:.3f}-{tb[2]:.3f}] | loop {tl[0]:8.3f} ms [{tl[1]:.3f}-{tl[2]:.3f}] x{row['speedup']:.2f} "
                f"apart {row['ranges_apart']} | kernels {row['kernels_total_ms']:.3f} ms, host {row['host_share_ms'][0]:.3f} ms | hypotheses "
                f"{st['hypotheses']}, draw lists {st['draw_lists']}, launches {st['launches']}, syncs {st['host_syncs']}, poses equal {same}/{k}")
        if not a.no_final:
            def chains():
                sel = -1
                for i, (c, raw) in enumerate(zip(sub, sub_clouds)):
                    r = single(c)   # (the model's features too: every coarse call computes them)
                    s = ctx.upload(*cbb.fine_inputs(ctx, fbb.transform_f32(r.T_svd, model)))
                    ix = ctx.build_index(ctx.upload(*cbb.fine_inputs(ctx, raw)))
                    f = ctx.icp(s, ix, fp)
                    fit = ctx.fitness(s, ix, f.T)[0]
                    if sel < 0 and (fit < 1e-4 or f.align_strength > 0.4):
                        sel = i
                return sel

            tf = cbb.timed(lambda: ctx.final_pose_batch_correspondences(m, sub, None, p), a.warmup, a.reps)
            tc = cbb.timed(chains, a.warmup, a.reps)
            row.update(final_batch_ms=tf, final_chains_ms=tc, final_speedup=tc[0] / tf[0], final_ranges_apart=tf[2] < tc[1],
                       selected=ctx.final_pose_batch_correspondences(m, sub, None, p)[1], selected_chains=chains())
            line += (f" | final batch {tf[0]:8.3f} ms [{tf[1]:.3f}-{tf[2]:.3f}] | {k} chains {tc[0]:8.3f} ms [{tc[1]:.3f}-{tc[2]:.3f}] "
                     f"x{row['final_speedup']:.2f} apart {row['final_ranges_apart']} selected {row['selected']} / {row['selected_chains']}")
        rows.append(row)
        print(line, flush=True)
        print("        kernels (us): " + ", ".join(f"{n} {v}" for n, v in sorted(kern.items(), key=lambda kv: -kv[1])), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
