#!/usr/bin/env python3
"""Times the frame's way onto the device, on rendered table-top depth images of 640 x 480 and 1280 x 960:
  (a) host:   the conversion on the host, ope_cloud_upload of the host cloud, ope_pass_through_cloud.  The conversion timed
              here is NUMPY ONLY (rgbd2Pcl's arithmetic, vectorised float32), not the C++ façade's: ope::DataGrabber::rgbd2Pcl
              runs the reference's scalar loop, and `detect_and_localize --depth-host --time` times that one (its
              `time ingest` lines, against those of `--depth --time`);
  (b) device: ope_depth_to_cloud with the crop;
  (c) each followed by ope_tabletop_segment.
Median [min-max] ms over --reps calls after --warmup, (a) and (b) alternating; every call ends synchronised.  One JSON line per
size, with the stats of (b) and its bytes against the HBM roofline (image bytes in, 16 B + 4 B per point out).
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/depth_bench.py --sizes 480x640 --reps 5`, in a run of its own."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ope = importlib.import_module("object-pose-estimation_amd")
synth = importlib.import_module("object-pose-estimation_amd.synth")

HBM_GBPS = 8000.0   # MI355X peak


def host_convert(img, p):
    """rgbd2Pcl + depthToMeter (datagrabber.cpp:65-174) in numpy float32: the points in column-major pixel order."""
    f32 = np.float32
    rows, cols = img.shape
    d = img.T.reshape(-1)
    z = d.astype(f32) / f32(p.scale)
    y = ((np.tile(np.arange(rows, dtype=f32), cols) - f32(p.c_row)) * z) / f32(p.f_row)
    x = ((np.repeat(np.arange(cols, dtype=f32), rows) - f32(p.c_col)) * z) / f32(p.f_col)
    keep = (d != 0) & ~(z.astype(np.float64) > p.z_max)
    return np.stack([x[keep], y[keep], z[keep]], axis=1)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["480x640", "960x1280"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ctx = ope.Context(0)
    par = ope.default_depth_params("kinect")
    lo, hi = np.float32([-0.8, -1.0, 0.3]), np.float32([0.8, 1.0, 1.9])
    for size in a.sizes:
        rows, cols = (int(v) for v in size.split("x"))
        img = synth.tabletop_depth_image(rows, cols)
        if (rows, cols) != (480, 640):
            # the same scene through a sensor of that resolution: the intrinsics scale with it
            k = rows / 480.0
            par_s = ope.default_depth_params("kinect", f_row=par.f_row * k, c_row=(par.c_row + 0.5) * k - 0.5, f_col=par.f_col * k,
                                             c_col=(par.c_col + 0.5) * k - 0.5)
            depth = importlib.import_module("object-pose-estimation_amd.depth")
            pts, _ = synth.tabletop_frame(rows * cols)
            img = depth.render_depth(pts.astype(np.float64) - synth.TABLETOP_DEPTH_CAMERA_SHIFT, par_s, rows, cols)
        else:
            par_s = par

        def host(segment):
            cloud = ctx.upload(host_convert(img, par_s))
            crop, _ = ctx.pass_through_cloud(cloud, lo, hi)
            return ctx.tabletop_segment(crop) if segment else crop

        def device(segment):
            crop = ctx.depth_to_cloud(img, par_s, lo, hi)
            return ctx.tabletop_segment(crop) if segment else crop

        def convert_only():
            return host_convert(img, par_s)

        out = {"case": size}
        for segment in (False, True):
            ta, tb = [], []
            for r in range(a.warmup + a.reps):
                for fn, ts in ((host, ta), (device, tb)):
                    t0 = time.perf_counter()
                    fn(segment)
                    ctx.sync()
                    if r >= a.warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
            tag = "+tabletop_segment" if segment else ""
            out["host" + tag], out["device" + tag] = stats(ta), stats(tb)
        tc = []
        for r in range(a.reps):
            t0 = time.perf_counter()
            convert_only()
            tc.append((time.perf_counter() - t0) * 1e3)
        out["host_conversion_alone"] = stats(tc)
        c = device(False)
        st = ctx.depth_stats()
        byts = 2.0 * rows * cols * 2 + 20.0 * c.n          # the image read by both passes, 16 B + 4 B per point written
        out["device_stats"] = dict(st, roofline_us=round(byts / (HBM_GBPS * 1e9) * 1e6, 3), bytes=int(byts))
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
