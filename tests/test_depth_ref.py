"""tests/depth_ref.py (vectorised numpy float32) against a plain double loop written in the reference's own order with
np.float32 scalars: rgbd2Pcl's column-outer / row-inner loop, depthToMeter's three float operations with the ROW as p_FeatX
(DetectAndLocalize/src/datagrabber.cpp:77-115, 169-171) and getPassThrough's inclusive limits (rosinterface.cpp:212)."""
import numpy as np
import pytest

import depth_ref as dr

F = np.float32


def loop_reference(depth, sensor, lo=None, hi=None):
    fx, fy, cx, cy = (F(v) for v in dr.PRESETS[sensor])
    scl = F(1000.0)
    rows, cols = depth.shape
    pts, pix = [], []
    for j in range(cols):            # datagrabber.cpp:77
        for i in range(rows):        # :79
            d = F(depth[i, j])
            if d <= F(0):            # :127,142,155: X = Y = Z = 0, then "Z == 0" at :90
                continue
            Z = d / scl              # :169
            X = (F(i) - cx) * Z / fx  # :170 (p_FeatX is the row)
            Y = (F(j) - cy) * Z / fy  # :171
            assert all(type(v) is np.float32 for v in (X, Y, Z))
            if float(Z) > 2.0:       # :90
                continue
            p = (Y, X, Z)            # :98-100: .x = Y, .y = X
            if lo is not None and any(p[k] > hi[k] or p[k] < lo[k] for k in range(3)):   # passthrough.hpp
                continue
            pts.append(p)
            pix.append(i * cols + j)
    return np.array(pts, F).reshape(-1, 3), np.array(pix, np.int32)


def small_image(rows, cols, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(400, 2400, (rows, cols)).astype(np.uint16)
    img[rng.random((rows, cols)) < 0.25] = 0
    img.flat[0] = 2000    # kept: 2.0 is not > 2.0
    img.flat[1] = 2001    # dropped
    img.flat[2] = 0
    img.flat[3] = 1
    img.flat[rows * cols - 1] = 65535
    return img


@pytest.mark.parametrize("sensor", ["kinect", "astra", "euclid"])
@pytest.mark.parametrize("shape", [(7, 5), (1, 9), (11, 1), (13, 17)])
def test_vectorised_equals_the_loop(sensor, shape):
    img = small_image(*shape, seed=shape[0] * 31 + shape[1])
    want_p, want_i = loop_reference(img, sensor)
    got_p, got_i = dr.depth_to_cloud(img, dr.preset(sensor))
    assert got_p.dtype == np.float32 and got_p.tobytes() == want_p.tobytes()
    assert np.array_equal(got_i, want_i)
    assert len(got_i) and 0 < len(got_i) < img.size


def test_order_is_column_major_and_the_principal_point_is_swapped():
    img = np.full((3, 4), 1000, np.uint16)
    p, pix = dr.depth_to_cloud(img, dr.preset("kinect"))
    assert pix.tolist() == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]   # rows run inside a column
    # cx = 319.5 acts on the row and lands in .y, cy = 239.5 on the column and lands in .x
    assert p[0].tolist() == [F(0 - 239.5) * F(1) / F(525), F(0 - 319.5) * F(1) / F(525), 1.0]
    assert p[1, 1] == F(1 - 319.5) * F(1) / F(525) and p[1, 0] == p[0, 0]


def test_zero_and_the_range_limit():
    img = np.array([[0, 2000, 2001, 1999, 1]], np.uint16)
    p, pix = dr.depth_to_cloud(img, dr.preset("astra"))
    assert pix.tolist() == [1, 3, 4]
    assert p[:, 2].tolist() == [2.0, F(1999) / F(1000), F(1) / F(1000)]


def test_crop_limits_are_inclusive():
    img = small_image(9, 8, 5)
    par = dr.preset("kinect")
    p, pix = dr.depth_to_cloud(img, par)
    k = len(p) // 2
    lo, hi = p.min(0).copy(), p.max(0).copy()
    lo[0], hi[1] = p[k, 0], p[k, 1]              # point k sits ON two limits
    got_p, got_i = dr.depth_to_cloud(img, par, lo, hi)
    want_p, want_i = loop_reference(img, "kinect", lo, hi)
    assert got_p.tobytes() == want_p.tobytes() and np.array_equal(got_i, want_i)
    assert pix[k] in got_i and len(got_i) < len(pix)
    inside = ((p >= lo) & (p <= hi)).all(axis=1)
    assert np.array_equal(got_i, pix[inside])
