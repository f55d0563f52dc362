"""ope_color_filter / ope_color_filter_cloud (ProcessingPcd::getFilterRgb's condition: lo < channel < hi for r, g and b, strict
integer comparisons) against a numpy mask on a 64 x 48 coloured cloud.  The channels are functions of the point's original index
that take every value 0..255, so a wrong gather or a wrong channel shows.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu

W, H = 64, 48
N = W * H


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    """an organised 64 x 48 cloud with 40 non-finite points; r, g, b by index, and a top byte that must play no part"""
    rng = np.random.default_rng(5)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    pts = np.stack([0.01 * u.ravel(), 0.01 * v.ravel(), 1.0 + 0.001 * rng.standard_normal(N)], 1).astype(np.float32)
    pts[rng.choice(N, 40, replace=False), rng.integers(0, 3, 40)] = np.nan
    i = np.arange(N, dtype=np.uint32)
    r, g, b = (i * 7 + 3) & 255, (i * 13 + 101) & 255, (i // 5 + 17) & 255
    col = ((i * 2654435761) & np.uint32(0xFF000000)) | (r << 16) | (g << 8) | b
    return pts, col.astype(np.uint32), r.astype(np.int64), g.astype(np.int64), b.astype(np.int64)


def mask_of(scene, lo, hi):
    _, _, r, g, b = scene
    return (r > lo[0]) & (r < hi[0]) & (g > lo[1]) & (g < hi[1]) & (b > lo[2]) & (b < hi[2])


def coloured(ctx, scene):
    c = ctx.upload(scene[0])
    c.set_rgb(scene[1])
    return c


LIMITS = {
    "all": ((-1, -1, -1), (256, 256, 256)),
    "none_r": ((200, -1, -1), (201, 256, 256)),      # an empty open interval
    "none_inverted": ((-1, 90, -1), (256, 40, 256)),
    "some": ((20, 50, 30), (180, 200, 160)),
    "one_channel": ((-1, -1, 99), (256, 256, 140)),
    "beyond_a_byte": ((-500, -1, -1), (1000, 128, 256)),
}


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_indices_equal_the_numpy_mask(ctx, scene, name):
    lo, hi = LIMITS[name]
    want = np.flatnonzero(mask_of(scene, lo, hi)).astype(np.int32)
    got = ctx.color_filter(coloured(ctx, scene), lo, hi)
    print("[color_filter] %s keeps %d of %d" % (name, len(want), N))
    if name == "all":
        assert len(want) == N
    elif name.startswith("none"):
        assert len(want) == 0
    else:
        assert 0 < len(want) < N
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_a_channel_equal_to_a_limit_is_refused(ctx, scene):
    """lo = v and hi = v + 2 keep exactly the points whose channel is v + 1, for each channel in turn"""
    _, _, r, g, b = scene
    c = coloured(ctx, scene)
    for ch, vals in enumerate((r, g, b)):
        lo, hi = [-1, -1, -1], [256, 256, 256]
        lo[ch], hi[ch] = 99, 101
        got = ctx.color_filter(c, lo, hi)
        assert (vals == 99).any() and (vals == 101).any() and (vals == 100).any()
        assert np.array_equal(got, np.flatnonzero(vals == 100))
    # the extremes: 0 passes only below a negative limit, 255 only below 256
    assert np.array_equal(ctx.color_filter(c, (0, -1, -1), (256, 256, 256)), np.flatnonzero(r > 0))
    assert np.array_equal(ctx.color_filter(c, (-1, -1, -1), (255, 256, 256)), np.flatnonzero(r < 255))


def test_non_finite_points_pass_by_colour_alone(ctx, scene):
    pts = scene[0]
    bad = np.flatnonzero(~np.isfinite(pts).all(1))
    assert len(bad) == 40
    lo, hi = LIMITS["some"]
    m = mask_of(scene, lo, hi)
    assert m[bad].any() and not m[bad].all()
    got = ctx.color_filter(coloured(ctx, scene), lo, hi)
    assert np.array_equal(np.intersect1d(got, bad), bad[m[bad]])


def test_the_top_byte_plays_no_part(ctx, scene):
    pts, col = scene[0], scene[1]
    lo, hi = LIMITS["some"]
    a = ctx.upload(pts); a.set_rgb(col & np.uint32(0x00FFFFFF))
    b = ctx.upload(pts); b.set_rgb(col | np.uint32(0xFF000000))
    assert np.array_equal(ctx.color_filter(a, lo, hi), ctx.color_filter(b, lo, hi))


@pytest.mark.parametrize("name", ["all", "none_r", "some"])
def test_cloud_form_equals_select(ctx, scene, name):
    pts, col = scene[0], scene[1]
    lo, hi = LIMITS[name]
    c = coloured(ctx, scene)
    nrm = np.random.default_rng(9).standard_normal((N, 3)).astype(np.float32)
    c.set_normals(nrm)
    want = np.flatnonzero(mask_of(scene, lo, hi)).astype(np.int32)
    out, idx = ctx.color_filter(c, lo, hi, as_cloud=True)
    assert np.array_equal(idx, want) and out.n == len(want) and out.has_rgb
    sel = ctx.select(c, want)
    assert ctx.download(out).tobytes() == ctx.download(sel).tobytes() == pts[want].tobytes()
    assert np.array_equal(out.download_rgb(), col[want])
    if len(want):
        assert out.download_normals()[0].tobytes() == sel.download_normals()[0].tobytes() == nrm[want].tobytes()


def test_a_cloud_without_colours_is_refused(ctx, scene):
    ope = load_pkg()
    plain = ctx.upload(scene[0])
    for as_cloud in (False, True):
        with pytest.raises(ope.OpeError) as e:
            ctx.color_filter(plain, (0, 0, 0), (255, 255, 255), as_cloud=as_cloud)
        assert e.value.code == ope.OPE_EINVAL


def test_an_empty_coloured_cloud_gives_nothing(ctx):
    e = ctx.upload(np.zeros((0, 3), np.float32))
    e.set_rgb(np.zeros(0, np.uint32))
    assert ctx.color_filter(e, (-1, -1, -1), (256, 256, 256)).shape == (0,)
    out, idx = ctx.color_filter(e, (-1, -1, -1), (256, 256, 256), as_cloud=True)
    assert out.n == 0 and len(idx) == 0
