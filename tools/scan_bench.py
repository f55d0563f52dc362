#!/usr/bin/env python3
"""Times a COLOURED frame's way onto the device, on rendered table-top depth images of 640 x 480 and 1280 x 960 with a random BGR
image of the same size:
  (a) host:   what the code before the colour payload needs for the same result: the conversion of both images on the host (numpy
              float32, vectorised; the colours gathered through the kept pixels), ope_cloud_upload, ope_pass_through_cloud with its
              index list, and, in the second pair of columns, ope_tabletop_segment + ope_euclidean_clusters_cloud followed by
              the gather of every cluster's colours on the host through the composed index lists;
  (b) device: ope_depth_to_cloud_rgb with the crop, the same device stages on the coloured cloud, one ope_cloud_download_rgb per
              cluster (the same result on the host: the clusters' colours).
Median [min-max] ms over --reps calls after --warmup, (a) and (b) alternating; every call ends synchronised, and the device
clouds a call made are freed after its clock has stopped.  One JSON line per size.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/scan_bench.py --sizes 480x640 --reps 5`, in a run of its own."""
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
depth = importlib.import_module("object-pose-estimation_amd.depth")


def host_convert(img, bgr, p):
    """rgbd2Pcl(rgb, depth) (BuildModel datagrabber.cpp:9-64) in numpy float32: points and colour words, columns outer."""
    f32 = np.float32
    rows, cols = img.shape
    d = img.T.reshape(-1)
    z = d.astype(f32) / f32(p.scale)
    y = ((np.tile(np.arange(rows, dtype=f32), cols) - f32(p.c_row)) * z) / f32(p.f_row)
    x = ((np.repeat(np.arange(cols, dtype=f32), rows) - f32(p.c_col)) * z) / f32(p.f_col)
    keep = (d != 0) & ~(z.astype(np.float64) > p.z_max)
    c = bgr.transpose(1, 0, 2).reshape(-1, 3)[keep].astype(np.uint32)
    return np.stack([x[keep], y[keep], z[keep]], axis=1), c[:, 2] << 16 | c[:, 1] << 8 | c[:, 0]


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
        k = rows / 480.0   # the same scene through a sensor of that resolution: the intrinsics scale with it
        par_s = ope.default_depth_params("kinect", f_row=par.f_row * k, c_row=(par.c_row + 0.5) * k - 0.5, f_col=par.f_col * k,
                                         c_col=(par.c_col + 0.5) * k - 0.5)
        pts, _ = synth.tabletop_frame(rows * cols)
        img = depth.render_depth(pts.astype(np.float64) - synth.TABLETOP_DEPTH_CAMERA_SHIFT, par_s, rows, cols)
        bgr = np.random.default_rng(1).integers(0, 256, (rows, cols, 3)).astype(np.uint8)

        # both return (the colours of the result on the host, the device clouds the call made: freed by the caller, off the clock)
        def host(segment):
            xyz, rgb = host_convert(img, bgr, par_s)
            up = ctx.upload(xyz)
            crop, idx = ctx.pass_through_cloud(up, lo, hi, want_idx=True)
            rgb = rgb[idx]
            if not segment:
                return [rgb], [up, crop]
            seg = ctx.tabletop_segment(crop)
            clouds, ci = ctx.euclidean_clusters_cloud(seg.not_plane)
            return [rgb[seg.not_plane_idx][i] for i in ci], [up, crop, seg.plane, seg.not_plane] + clouds

        def device(segment):
            crop = ctx.depth_to_cloud(img, par_s, lo, hi, bgr=bgr)
            if not segment:
                return [crop.download_rgb()], [crop]
            seg = ctx.tabletop_segment(crop)
            clouds, _ = ctx.euclidean_clusters_cloud(seg.not_plane)
            return [c.download_rgb() for c in clouds], [crop, seg.plane, seg.not_plane] + clouds

        def release(made):
            for c in made:
                if c is not None:
                    c.free()

        out = {"case": size}
        for segment in (False, True):
            (ha, ma), (hb, mb) = host(segment), device(segment)
            assert len(ha) == len(hb) >= 1 and all(np.array_equal(x, y) for x, y in zip(ha, hb))   # the same result, before it is timed
            release(ma + mb)
            out["result" + ("+segmentation+clusters" if segment else "")] = [int(len(x)) for x in hb]
            ta, tb = [], []
            for r in range(a.warmup + a.reps):
                for fn, ts in ((host, ta), (device, tb)):
                    t0 = time.perf_counter()
                    _, made = fn(segment)
                    ctx.sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    release(made)
                    if r >= a.warmup:
                        ts.append(dt)
            tag = "+segmentation+clusters" if segment else ""
            out["host" + tag], out["device" + tag] = stats(ta), stats(tb)
        ctx.depth_to_cloud(img, par_s, lo, hi, bgr=bgr).free()
        out["device_stats"] = ctx.depth_stats()
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
