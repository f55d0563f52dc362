"""tests/depth_rgb_ref.py against a 2 x 3 image worked out by hand: the drop rule (a zero depth, a pixel with Z > 2.0, a pixel with
Z == 2.0 that stays), the column-outer order and the channel order B, G, R -> r << 16 | g << 8 | b."""
import numpy as np

import depth_ref as dr
import depth_rgb_ref as drr


def test_hand_computed_2x3_image():
    depth = np.array([[1000, 0, 500],
                      [2500, 1500, 2000]], np.uint16)
    # pixel k = row * 3 + col holds b = 10 k + 1, g = 10 k + 2, r = 10 k + 3
    bgr = np.zeros((2, 3, 3), np.uint8)
    for k in range(6):
        bgr[k // 3, k % 3] = (10 * k + 1, 10 * k + 2, 10 * k + 3)
    pts, pix, rgb = drr.depth_to_cloud_rgb(depth, bgr, dr.preset("kinect"))
    # columns outer: (0,0) kept, (1,0) Z = 2.5 dropped | (0,1) zero dropped, (1,1) kept | (0,2) kept, (1,2) Z = 2.0 kept
    assert pix.tolist() == [0, 4, 2, 5]
    assert pts[:, 2].tolist() == [1.0, 1.5, 0.5, 2.0]
    assert rgb.dtype == np.uint32
    assert rgb.tolist() == [0x030201, 0x2B2A29, 0x171615, 0x353433]
    assert (rgb >> 24).max() == 0
    # the same points as the depth-only conversion, byte for byte
    want, want_pix = dr.depth_to_cloud(depth, dr.preset("kinect"))
    assert pts.tobytes() == want.tobytes() and np.array_equal(pix, want_pix)


def test_crop_keeps_colour_with_its_point():
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 2300, (9, 7)).astype(np.uint16)
    bgr = rng.integers(0, 256, (9, 7, 3)).astype(np.uint8)
    lo, hi = np.float32([-0.5, -0.6, 0.3]), np.float32([0.5, 0.2, 1.4])
    pts, pix, rgb = drr.depth_to_cloud_rgb(depth, bgr, dr.preset("astra"), lo, hi)
    assert 0 < len(pix) < 63
    flat = bgr.reshape(-1, 3).astype(np.uint32)
    assert np.array_equal(rgb, flat[pix, 2] << 16 | flat[pix, 1] << 8 | flat[pix, 0])
