"""Euclidean cluster extraction on the device (ope_euclidean_clusters): ms per call, kernel launches and host synchronisations.

Cases (the cloud is uploaded once; each call is synchronous, timed with the host clock; 3 warm-up and 10 timed calls; median
and min-max):
  tabletop-20k   synth.tabletop_objects(): a C1-size non-plane cloud, tolerance 0.05, 300 .. 1e5 points;
  tabletop-300k  the same frame at 16x the density (a whole cropped Kinect frame), same parameters;
  c3-0.05        the 1 M C3 frame (synth.config_clouds("C3")) at 0.05: one component above max_size, zero clusters (the worst case);
  c3-0.005       the same frame at 0.005;
  clumps-128k    an adversarial cloud: 4 x 4 x 4 clumps of 2 000 points each, 1.2 tolerances apart at 0.05, so that dense
                 neighbouring cells hold no joining pair and every point pair of them is compared.
Then the hand-over to the pose stage on tabletop-20k: euclidean_clusters_cloud -> final_pose_batch against euclidean_clusters ->
host gather of scene[idx_k] -> one upload per cluster -> final_pose_batch (what a caller does without the _cloud form).

    python tools/cluster_bench.py [--cases tabletop-20k,tabletop-300k,c3-0.05,c3-0.005,clumps-128k] [--json out.json]
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
MODEL = os.path.join(ROOT, "tests", "golden", "drill_model_decimated.pcd")
WARMUP, REPS = 3, 10


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def cloud_of(name):
    if name == "tabletop-20k":
        return synth.tabletop_objects()[0], 0.05
    if name == "tabletop-300k":
        return synth.tabletop_objects(n_drill=128000, density=1.0e6)[0], 0.05
    if name == "clumps-128k":
        rng = np.random.default_rng(7)
        centres = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.06
        return (centres[:, None, :] + rng.uniform(-0.002, 0.002, (64, 2000, 3))).reshape(-1, 3).astype(np.float32), 0.05
    if name.startswith("c3-"):
        return synth.config_clouds("C3")[0], float(name[3:])
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="tabletop-20k,tabletop-300k,c3-0.05,c3-0.005,clumps-128k")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = ope.Context(0)
    rows = []
    for name in a.cases.split(","):
        pts, tol = cloud_of(name)
        cloud = ctx.upload(pts)
        med, lo, hi = timed(lambda: ctx.euclidean_clusters(cloud, tolerance=tol))
        got = ctx.euclidean_clusters(cloud, tolerance=tol)
        s = ctx.cluster_stats()
        row = dict(case=name, n=len(pts), tolerance=tol, clusters=len(got), sizes=[len(c) for c in got][:8], ms=med, ms_min=lo, ms_max=hi,
                   **s)
        print(json.dumps(row), flush=True)
        rows.append(row)
        cloud.free()
    # the hand-over to the pose stage
    pts, _ = cloud_of("tabletop-20k")
    model = ctx.upload(np.ascontiguousarray(pcd.read_pcd(MODEL)[0], np.float32))
    scene = ctx.upload(pts)

    def device_form():
        clouds, _ = ctx.euclidean_clusters_cloud(scene)
        ctx.final_pose_batch(model, clouds)

    def host_form():
        idx = ctx.euclidean_clusters(scene)
        clouds = [ctx.upload(pts[i]) for i in idx]
        ctx.final_pose_batch(model, clouds)

    def cut_device():
        ctx.euclidean_clusters_cloud(scene)

    def cut_host():
        idx = ctx.euclidean_clusters(scene)
        [ctx.upload(pts[i]) for i in idx]

    for name, fn in (("cloud-form+final_pose_batch", device_form), ("indices+host-upload+final_pose_batch", host_form),
                     ("cloud-form", cut_device), ("indices+host-upload", cut_host)):
        med, lo, hi = timed(fn)
        row = dict(case=name, ms=med, ms_min=lo, ms_max=hi)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
