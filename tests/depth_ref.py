"""The depth-to-cloud conversion of the reference, restated in numpy float32 and vectorised: DataGrabber::rgbd2Pcl with
depthToMeter (DetectAndLocalize/src/datagrabber.cpp:65-174) and ProcessingPcd::getPassThrough (rosinterface.cpp:212).
tests/test_depth_ref.py pins it against a plain double loop in the reference's own order."""
import numpy as np

# (fx, fy, cx, cy) as the reference's float variables hold them (datagrabber.cpp:133-136, 146-149, 159-162)
PRESETS = {
    "euclid": (306.178, 306.929, 158.523, 122.747),
    "kinect": (525.0, 525.0, 319.5, 239.5),
    "astra": (570.342, 570.342, 314.5, 235.5),
}


def preset(sensor):
    """dict(f_row, c_row, f_col, c_col, scale, z_max): rgbd2Pcl passes the ROW as p_FeatX, so cx / fx act on the row."""
    fx, fy, cx, cy = (np.float32(v) for v in PRESETS[sensor])
    return dict(f_row=fx, c_row=cx, f_col=fy, c_col=cy, scale=np.float32(1000.0), z_max=2.0)


def depth_to_cloud(depth, p, lo=None, hi=None):
    """(points float32 (n, 3) in the reference's order — columns outer, rows inner —, pixel index row * cols + col of each)."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 2
    rows, cols = depth.shape
    f32 = np.float32
    # column-major traversal: element k of the flattened transposed image is (row k % rows, col k // rows)
    d = depth.T.reshape(-1)
    row = np.tile(np.arange(rows, dtype=np.int64), cols)
    col = np.repeat(np.arange(cols, dtype=np.int64), rows)
    z = d.astype(f32) / f32(p["scale"])
    y = ((row.astype(f32) - f32(p["c_row"])) * z) / f32(p["f_row"])
    x = ((col.astype(f32) - f32(p["c_col"])) * z) / f32(p["f_col"])
    assert z.dtype == y.dtype == x.dtype == np.float32
    keep = (d != 0) & ~(z.astype(np.float64) > float(p["z_max"]))
    pts = np.stack([x, y, z], axis=1)
    if lo is not None:
        lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
        with np.errstate(invalid="ignore"):
            keep &= np.isfinite(pts).all(axis=1) & ~((pts > hi) | (pts < lo)).any(axis=1)
    return np.ascontiguousarray(pts[keep]), (row * cols + col)[keep].astype(np.int32)
