#!/usr/bin/env python3
"""Times ope_region_grow_rgb on a 307 200-point synthetic coloured frame: a 640 x 480 depth-like surface (z = 0.8 m +- 5 cm, 0.2 mm
noise, 3 000 non-finite points), coloured in patches of 80 x 80 pixels in eight colours with up to 3 levels of channel noise, and
2 000 salt points of random colours.  The reference's parameters (K = 100, thresholds 0.1 / 10 / 10, min 700).  Prints one JSON line
per call (the first includes what a first call pays): host clock around the synchronised call, the stats, the clusters and the
per-kernel times (ope_profile_kernels), then one unprofiled call."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ope = importlib.import_module("object-pose-estimation_amd")
ctx = ope.Context(0)
rng = np.random.default_rng(1)
W, H = 640, 480
u, v = np.meshgrid(np.arange(W), np.arange(H))
z = 0.8 + 0.05 * np.sin(u / 40.0) * np.cos(v / 55.0)
pts = np.stack([(u - 320) * z / 570.0, (v - 240) * z / 570.0, z], -1).reshape(-1, 3)
pts += rng.normal(0, 2e-4, pts.shape)
pts = pts.astype(np.float32)
pts[rng.choice(len(pts), 3000, replace=False)] = np.nan
# patches of 80 x 80 pixels in eight colours, a little channel noise, salt
patch = ((u // 80) + 3 * (v // 80)) % 8
base = np.array([[200, 30, 30], [30, 200, 30], [30, 30, 200], [200, 200, 30], [30, 200, 200], [200, 30, 200], [120, 120, 120], [240, 240, 240]])
col = base[patch.ravel()] + rng.integers(0, 4, (W * H, 3))
salt = rng.choice(W * H, 2000, replace=False)
col[salt] = rng.integers(0, 256, (2000, 3))
rgb = ((col[:, 0] << 16) | (col[:, 1] << 8) | col[:, 2]).astype(np.uint32)
cloud = ctx.upload(pts)
cloud.set_rgb(rgb)
out = {}
for rep in range(3):
    ctx.profile_kernels(True)
    t = time.perf_counter()
    clusters, labels, stats = ctx.region_grow_rgb(cloud)
    wall = time.perf_counter() - t
    rec = ctx.profile_kernels_read()
    ctx.profile_kernels(False)
    out = dict(wall_ms=wall * 1e3, stats=stats, clusters=len(clusters), sizes=sorted(len(c) for c in clusters)[-5:],
               kernels={k: round(r["ms"], 3) for k, r in sorted(rec.items(), key=lambda kv: -kv[1]["ms"])})
    print(json.dumps(out), flush=True)
t = time.perf_counter()
clusters2, _, _ = ctx.region_grow_rgb(cloud)
print("unprofiled wall ms", (time.perf_counter() - t) * 1e3, "same", all(np.array_equal(a, b) for a, b in zip(clusters, clusters2)))
ctx.close()
