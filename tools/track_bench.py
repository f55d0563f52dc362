"""Later frames at the reference's size (C1): `detect_and_localize --track` (ope::ObjectTracker::localize, ope_track_pose)
against `--track-loop` (the reference's loop through the facade: host compute3DCentroid, estimateFinalPose one call at a time).

Each case is a sequence of identical frames after one first frame, so every later frame takes the same branch:
  gated-skip    a copy of the model (moved) and K - 1 distractors 20+ cm away; the fine fit scores <= 1e-4, the coarse stage is
                skipped;
  gated-coarse  the C1 scene cluster (a partial view: the fit scores ~1.3e-4 > 1e-4) and the distractors: every frame runs SAC-IA;
  realign       the scene cluster alternating between two places 10 cm apart: the frames re-align all clusters (batched).
The driver times each frame with the host clock around the synchronised call; after the first frame, 5 warm-up and 20 timed
frames; median and min-max.  The branch of every timed frame is reported too.

    python tools/track_bench.py [--ks 1,8,32] [--cases gated-skip,gated-coarse,realign] [--json out.json]
"""
import argparse
import collections
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
EXE = os.path.join(ROOT, "object-pose-estimation_amd", "build", "detect_and_localize")
MODEL = os.path.join(ROOT, "tests", "golden", "drill_model_decimated.pcd")
WARMUP, REPS = 5, 20


def clusters(k, noisy, shift):
    scene = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "drill_scene_c1.npz"))["scene"], np.float32)
    c = scene.mean(0)
    if noisy:
        obj = scene.copy()
    else:
        m, _ = pcd.read_pcd(MODEL)
        obj = (np.asarray(m, np.float32) - np.asarray(m, np.float32).mean(0) + c).astype(np.float32)
    obj = (obj + np.asarray(shift, np.float32)).astype(np.float32)
    out = [obj]
    for j in range(k - 1):
        a = 2 * np.pi * j / max(k - 1, 1)
        d = synth.model_surface(4000, seed=100 + j) * np.float32(0.8)
        out.append((d - d.mean(0) + c + np.float32(0.25 + 0.01 * j) * np.array([np.cos(a), np.sin(a), 0], np.float32)).astype(np.float32))
    return out


def run_case(case, k, tmp):
    frames = []
    for f in range(1 + WARMUP + REPS):
        shift = [0.1 * (f % 2), 0, 0] if case == "realign" else [0, 0, 0]
        frames.append(clusters(k, case != "gated-skip", shift))
    paths = []
    for f, cl in enumerate(frames):
        paths.append([])
        for j, c in enumerate(cl):
            p = os.path.join(tmp, f"{case}_{k}_{f}_{j}.pcd")
            pcd.write_pcd(p, c)
            paths[-1].append(p)
    res = {}
    for mode in ("--track", "--track-loop"):
        args = [EXE, mode, MODEL, "--time"]
        for f in paths:
            args += ["--frame", *f]
        r = subprocess.run(args, capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        ms = [float(ln.split()[4]) for ln in r.stdout.splitlines() if ln.startswith("time frame ")]
        br = [ln.split()[4] for ln in r.stdout.splitlines() if ln.startswith("track frame ")]
        t = np.array(ms[1 + WARMUP:])
        res[mode.strip("-")] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                "branches": dict(collections.Counter(br[1 + WARMUP:]))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--cases", default="gated-skip,gated-coarse,realign")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists(EXE):
        import __graft_entry__ as g
        g.build()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in a.cases.split(","):
            for k in [int(x) for x in a.ks.split(",")]:
                r = run_case(case, k, tmp)
                out[f"{case} K={k}"] = r
                print(f"{case:13s} K={k:2d}  " + "  ".join(f"{m}: {v['median_ms']:.2f} [{v['min_ms']:.2f}-{v['max_ms']:.2f}] ms {v['branches']}"
                                                      for m, v in r.items()), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
