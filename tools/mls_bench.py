#!/usr/bin/env python3
"""Times ope_mls_smooth_cloud (radius 0.02, order 2) on the decimated drill model and on 100 k- and 1 M-point synthetic models
(synth.model_surface).  One JSON line per case:
  call_ms          median [min-max] over --reps calls after --warmup of the WHOLE call, a host clock around work that ends in a
                   device synchronise: the temporary index, both walks, the scan, the new cloud's allocation and Morton ordering,
                   and freeing it (what a caller pays, not a kernel time)
  kernels          HIP-event times of mls_plane_kernel (walk A) and mls_fit_kernel (walk B) from ope_profile_kernels, medians over
                   --reps profiled calls, with their algorithmic bytes (16 per neighbour visited + the per-point records) as GB/s
                   and their fp64 operations, counted from the source (walk A 18 per neighbour, walk B 64 and one exp), as GFLOP/s,
                   each beside the chip's peak (8 TB/s HBM, 78.6 TFLOP/s fp64 vector, public spec sheet)
  neighbours_per_point, and for scale spfh_kernel_ms: ope_fpfh's first pass on the same cloud and radius (the same walk from the
  root, fp32 pair features and LDS histograms per neighbour).
Each kernel's share of the call under a tracer: `rocprofv3 --kernel-trace --stats -- python tools/mls_bench.py --sizes 100000 --no-drill`."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ope = importlib.import_module("object-pose-estimation_amd")
synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


HBM_GBPS = 8000.0      # MI355X peak
FP64_GFLOPS = 78600.0   # fp64 vector peak


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
    ap.add_argument("--sizes", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--no-drill", action="store_true")
    ap.add_argument("--radius", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = ope.Context(0)
    cases = [] if a.no_drill else [("drill_model_decimated", pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))[0])]
    cases += [("model_surface_%d" % n, synth.model_surface(n, 1)) for n in a.sizes]
    for name, pts in cases:
        cloud = ctx.upload(pts)

        def run():
            out, _ = ctx.mls_smooth(cloud, a.radius, as_cloud=True)
            out.free()

        out = {"case": name, "points": int(len(pts)), "radius": a.radius}
        out["call_ms"] = timed(run, a.reps, a.warmup)
        st = ctx.mls_stats()
        out["stats"] = st
        out["neighbours_per_point"] = round(st["neighbours_total"] / max(st["n_in"], 1), 1)
        samples = {"mls_plane_kernel": [], "mls_fit_kernel": []}
        nbytes = {}
        for _ in range(a.reps):
            ctx.profile_kernels(True)
            run()
            prof = ctx.profile_kernels_read()
            ctx.profile_kernels(False)
            for k in samples:
                samples[k].append(prof[k]["ms"])
                nbytes[k] = prof[k]["algorithmic_bytes"]
        flops = {"mls_plane_kernel": 18.0, "mls_fit_kernel": 64.0}
        out["kernels"] = {}
        for k, ts in samples.items():
            ms = statistics.median(ts)
            out["kernels"][k] = {"median_ms": round(ms, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                                 "GBps": round(nbytes[k] / (ms * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(nbytes[k] / (ms * 1e-3) / 1e9 / HBM_GBPS, 4),
                                 "fp64_GFLOPs": round(flops[k] * st["neighbours_total"] / (ms * 1e-3) / 1e9, 1),
                                 "share_of_fp64_peak": round(flops[k] * st["neighbours_total"] / (ms * 1e-3) / 1e9 / FP64_GFLOPS, 4)}
        ctx.normals(cloud, k=12, fetch=False)
        ctx.profile_kernels(True)
        ctx.fpfh(cloud, a.radius)
        prof = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        out["spfh_kernel_ms"] = round(prof.get("spfh_kernel", {}).get("ms", float("nan")), 3)
        print(json.dumps(out), flush=True)
        cloud.free()
    ctx.close()


if __name__ == "__main__":
    main()
