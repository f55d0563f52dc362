"""ope_depth_to_cloud_rgb on the device: the cloud is ope_depth_to_cloud's byte for byte, the colours are tests/depth_rgb_ref.py's
and those of `bgr` gathered through out_pixel; the booked launches and synchronisations do not depend on the image; the
OPE_EINVAL cases launch nothing.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import depth_ref as dr
import depth_rgb_ref as drr
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 200), (200, 1), (70, 130), (64, 64))
LO, HI = np.float32([-0.25, -0.3, 0.4]), np.float32([0.2, 0.25, 1.6])


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


def images(shape, seed):
    """depth with about 20 % zeros and a few values above z_max * scale; random colours; for 70 x 130 both images are views
    with padded, different row strides"""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    pad_d, pad_c = (11, 5) if shape == (70, 130) else (0, 0)
    d = rng.integers(300, 2001, (rows, cols + pad_d)).astype(np.uint16)
    d[rng.random(d.shape) < 0.2] = 0
    d[rng.random(d.shape) < 0.03] = 2600
    c = rng.integers(0, 256, (rows, cols + pad_c, 3)).astype(np.uint8)
    if shape == (1, 1):
        d[0, 0] = 1234
    return d[:, :cols], c[:, :cols]


@pytest.mark.parametrize("crop", [False, True], ids=["full", "crop"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_coloured_ingest_equals_the_reference(ctx, shape, crop):
    ope = load_pkg()
    depth, bgr = images(shape, 100 + shape[0])
    if shape == (70, 130):
        assert depth.strides[0] == 2 * 141 and bgr.strides[0] == 3 * 135
    lo, hi = (LO, HI) if crop else (None, None)
    for sensor in ("kinect", "euclid"):
        par = ope.default_depth_params(sensor)
        want_p, want_i, want_c = drr.depth_to_cloud_rgb(depth, bgr, dr.preset(sensor), lo, hi)
        plain, ppix = ctx.depth_to_cloud(depth, par, lo, hi, want_pixels=True)
        assert not plain.has_rgb
        cloud, pix = ctx.depth_to_cloud(depth, par, lo, hi, want_pixels=True, bgr=bgr)
        st = ctx.depth_stats()
        assert cloud.has_rgb and cloud.n == len(want_i) == st["kept"] and st["pixels"] == depth.size
        assert np.array_equal(pix, want_i) and np.array_equal(pix, ppix)
        assert ctx.download(cloud).tobytes() == ctx.download(plain).tobytes() == want_p.tobytes()
        got = cloud.download_rgb()
        flat = np.ascontiguousarray(bgr).reshape(-1, 3).astype(np.uint32)
        assert got.dtype == np.uint32 and np.array_equal(got, want_c)
        assert np.array_equal(got, flat[pix, 2] << 16 | flat[pix, 1] << 8 | flat[pix, 0])
        # the same cloud inside as well: the next filter leaves the same survivors, with their colours
        if cloud.n:
            a, ia = ctx.pass_through_cloud(cloud, LO + np.float32(0.02), HI, want_idx=True)
            b, ib = ctx.pass_through_cloud(plain, LO + np.float32(0.02), HI, want_idx=True)
            assert np.array_equal(ia, ib) and ctx.download(a).tobytes() == ctx.download(b).tobytes()
            assert np.array_equal(a.download_rgb(), want_c[ia]) and not b.has_rgb


def test_all_zero_depth_gives_an_empty_coloured_cloud(ctx):
    depth, bgr = np.zeros((70, 65), np.uint16), np.full((70, 65, 3), 9, np.uint8)
    for lo, hi in ((None, None), (LO, HI)):
        cloud, pix = ctx.depth_to_cloud(depth, None, lo, hi, want_pixels=True, bgr=bgr)
        assert cloud.n == 0 and len(pix) == 0 and cloud.has_rgb
        assert cloud.download_rgb().shape == (0,)
        sel = ctx.select(cloud, np.zeros(0, np.int32))
        assert sel.n == 0 and sel.has_rgb


def test_booked_launches_do_not_depend_on_the_image(ctx):
    seen = {}
    for shape in ((1, 1), (70, 130)):
        depth, bgr = images(shape, 7)
        for crop in (False, True):
            for want_pixels in (False, True):
                lo, hi = (LO, HI) if crop else (None, None)
                ctx.depth_to_cloud(depth, None, lo, hi, want_pixels=want_pixels, bgr=bgr)
                a = ctx.depth_stats()
                ctx.depth_to_cloud(depth, None, lo, hi, want_pixels=want_pixels)
                b = ctx.depth_stats()
                # one for one the sequence of the depth-only call
                assert (a["launches"], a["host_syncs"]) == (b["launches"], b["host_syncs"])
                seen.setdefault((crop, want_pixels), set()).add((a["launches"], a["host_syncs"]))
    print("[depth rgb] (crop, pixels) -> (launches, host syncs)", seen)
    assert all(len(v) == 1 for v in seen.values()), seen


def test_error_cases_launch_nothing(ctx):
    ope = load_pkg()
    L = ope.lib()
    img = np.full((4, 6), 1000, np.uint16)
    bgr = np.full((4, 6, 3), 200, np.uint8)
    par = ope.default_depth_params()
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    h, n = C.c_void_p(), C.c_size_t()

    def call(ctx_h=ctx.h, depth=img.ctypes.data, rows=4, cols=6, stride=12, colour=bgr.ctypes.data, cstride=18, p=par, lo_=None, hi_=None,
             out=C.byref(h)):
        return L.ope_depth_to_cloud_rgb(ctx_h, depth, rows, cols, stride, colour, cstride, C.byref(p) if p is not None else None, lo_, hi_,
                                        out, None, C.byref(n))

    before = ctx.depth_to_cloud(img, bgr=bgr)
    stats = ctx.depth_stats()
    bad = lambda **kw: ope.default_depth_params(**kw)
    cases = {
        "NULL bgr": dict(colour=None), "short bgr stride": dict(cstride=17),
        "NULL ctx": dict(ctx_h=None), "NULL depth": dict(depth=None), "NULL params": dict(p=None), "NULL out": dict(out=None),
        "no rows": dict(rows=0), "no cols": dict(cols=0, cstride=0), "too many pixels": dict(rows=1 << 16, cols=1 << 15, stride=1 << 16, cstride=3 << 15),
        "short stride": dict(stride=10), "odd stride": dict(stride=13),
        "scale 0": dict(p=bad(scale=0.0)), "scale nan": dict(p=bad(scale=float("nan"))), "f_row 0": dict(p=bad(f_row=0.0)),
        "f_col < 0": dict(p=bad(f_col=-525.0)), "f_row inf": dict(p=bad(f_row=float("inf"))),
        "c_row nan": dict(p=bad(c_row=float("nan"))), "c_col inf": dict(p=bad(c_col=float("inf"))),
        # 5 bytes per padded pixel: 6.8 M pixels in a row are above the block, where the depth-only call takes 16.7 M
        "a row above the staging block": dict(rows=1, cols=7 << 20, stride=14 << 20, cstride=21 << 20),
        "lo alone": dict(lo_=fp(lo)), "hi alone": dict(hi_=fp(hi)),
    }
    for name, kw in cases.items():
        assert call(**kw) == ope.OPE_EINVAL, name
        assert ctx.depth_stats() == stats, name      # nothing launched
    assert call() == ope.OPE_OK and n.value == 24
    L.ope_cloud_free(h)
    after = ctx.depth_to_cloud(img, bgr=bgr)
    assert ctx.download(after).tobytes() == ctx.download(before).tobytes()
    assert np.array_equal(after.download_rgb(), before.download_rgb())
    assert np.array_equal(after.download_rgb(), np.full(24, 0xC8C8C8, np.uint32))
