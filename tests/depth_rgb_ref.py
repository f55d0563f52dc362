"""The two-image overload DataGrabber::rgbd2Pcl(p_imageRgb, p_imageDepth) of the reference (BuildModel/src/datagrabber.cpp:9-64)
restated in numpy: the geometry, the drop rule and the order are tests/depth_ref.py's; the colour of a point is that of its pixel
in a CV_8UC3 image, bytes 0, 1, 2 being b, g, r (:48-51), packed as PointXYZRGB::rgb packs it: r << 16 | g << 8 | b."""
import numpy as np

import depth_ref as dr


def depth_to_cloud_rgb(depth, bgr, p, lo=None, hi=None):
    """(points float32 (n, 3), pixel index of each, colour word uint32 of each), columns outer, rows inner."""
    depth, bgr = np.asarray(depth), np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.shape == depth.shape + (3,)
    rows, cols = depth.shape
    pts, pix = dr.depth_to_cloud(depth, p, lo, hi)
    # the image in the loop's order: element col * rows + row of the transposed image is pixel (row, col)
    t = bgr.transpose(1, 0, 2).reshape(-1, 3).astype(np.uint32)
    k = (pix % cols).astype(np.int64) * rows + pix // cols
    b, g, r = t[k, 0], t[k, 1], t[k, 2]
    return pts, pix, ((r << np.uint32(16)) | (g << np.uint32(8)) | b).astype(np.uint32)
