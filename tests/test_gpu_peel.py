"""ope_plane_peel against tests/peel_ref.py: every comparison is exact (array_equal, bytes).  The scenes are peel_scenes' room
frames (three patches that do not touch, four blobs, noise); every test asserts its expectations on the REFERENCE first."""
import ctypes as C

import numpy as np
import pytest

import peel_ref as pf
from conftest import load_pkg
from peel_scenes import SCENES, noise_with_nans, room_scene

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


_ref = {}


def ref_of(name, seed, max_planes=0):
    """the scene and the reference's peel of it, computed once and shared"""
    key = (name, seed, max_planes)
    if key not in _ref:
        pts = room_scene(SCENES[name])
        pts.setflags(write=False)
        _ref[key] = (pts, pf.peel(pts, max_planes=max_planes, seed=seed))
    return _ref[key]


def check(ctx, pts, want, seed=12345, max_planes=0, clouds=True):
    ope = load_pkg()
    cloud = ctx.upload(pts)
    got = ctx.plane_peel(cloud, ope.default_plane_params(seed=seed), max_planes=max_planes, want_cloud=clouds, want_labels=True)
    print("[peel] n %d planes %d (ref %d) counts %s (ref %s) iterations %s rest %d (ref %d) stop %d (ref %d) launches %d syncs %d" %
          (len(pts), len(got.counts), len(want["counts"]), got.counts.tolist(), want["counts"].tolist(), got.iterations.tolist(),
           len(got.rest_idx), len(want["rest_idx"]), got.stop, want["stop"], got.stats["launches"], got.stats["host_syncs"]))
    assert got.stats["n_planes"] == len(want["coeffs"]) and got.stop == want["stop"]
    assert got.coeffs.tobytes() == want["coeffs"].tobytes()
    assert np.array_equal(got.counts, want["counts"]) and np.array_equal(got.iterations, want["iterations"])
    assert np.array_equal(got.labels, want["labels"])
    assert got.stats["n_rest"] == len(want["rest_idx"]) and np.array_equal(got.rest_idx, want["rest_idx"])
    if clouds:
        sel = ctx.select(cloud, want["rest_idx"])
        assert got.rest.n == sel.n == len(want["rest_idx"])
        assert ctx.download(got.rest).tobytes() == ctx.download(sel).tobytes() == pts[want["rest_idx"]].tobytes()
    return got


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("seed", SEEDS)
def test_peel_equals_the_reference(ctx, name, seed):
    pts, want = ref_of(name, seed)
    counts = want["counts"].tolist()
    if name == "three":
        assert sorted(counts) == [3000, 5000, 8000] and len(want["rest_idx"]) == 4000
    elif name == "exact":
        assert counts == [8000, 6000] and len(want["rest_idx"]) == 6000 and want["stop"] == pf.FRACTION
    else:
        assert counts[:2] == [8000, 5999] and len(counts) == 3
    check(ctx, pts, want, seed=seed)


def test_peel_without_refinement(ctx):
    ope = load_pkg()
    pts = ref_of("three", 1)[0]
    want = pf.peel(pts, seed=1, optimize_coefficients=0)
    assert len(want["coeffs"]) >= 3
    cloud = ctx.upload(pts)
    got = ctx.plane_peel(cloud, ope.default_plane_params(seed=1, optimize_coefficients=0), want_labels=True)
    assert got.coeffs.tobytes() == want["coeffs"].tobytes() and np.array_equal(got.counts, want["counts"])
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(got.rest_idx, want["rest_idx"]) and got.stop == want["stop"]


def test_the_cap_stops_the_loop(ctx):
    ope = load_pkg()
    pts, want = ref_of("exact", 1, max_planes=1)
    assert want["stop"] == pf.MAX_PLANES and want["counts"].tolist() == [8000] and len(want["rest_idx"]) == 12000
    got = check(ctx, pts, want, seed=1, max_planes=1)
    assert got.stop == ope.PEEL_MAX_PLANES


def test_rest_carries_colours_and_normals(ctx):
    ope = load_pkg()
    pts, want = ref_of("three", 2)
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(len(pts), 3)).astype(np.float32)
    rgb = rng.integers(0, 1 << 24, len(pts)).astype(np.uint32)
    cloud = ctx.upload(pts)
    cloud.set_normals(nrm)
    cloud.set_rgb(rgb)
    got = ctx.plane_peel(cloud, ope.default_plane_params(seed=2), want_cloud=True)
    assert np.array_equal(got.rest_idx, want["rest_idx"])
    sel = ctx.select(cloud, want["rest_idx"])
    assert np.array_equal(got.rest.download_rgb(), sel.download_rgb()) and np.array_equal(got.rest.download_rgb(), rgb[want["rest_idx"]])
    (gn, gc), (sn, sc) = got.rest.download_normals(), sel.download_normals()
    assert gn.tobytes() == sn.tobytes() and gc.tobytes() == sc.tobytes() and gn.tobytes() == nrm[want["rest_idx"]].tobytes()
    assert ctx.download(got.rest).tobytes() == ctx.download(sel).tobytes()


@pytest.mark.parametrize("name", ["three", "over"])
def test_peel_equals_the_loop_of_public_calls_on_the_device(ctx, name):
    ope = load_pkg()
    pts, want = ref_of(name, 3)
    assert len(want["coeffs"]) == 3
    p = ope.default_plane_params(seed=3)
    cur, n0, coeffs = ctx.upload(pts), len(pts), []
    while float(cur.n) > 0.3 * float(n0):
        one = ctx.plane_segment(cur, p, want_clouds=True)
        if not one.found or len(one.inliers) == 0:
            break
        coeffs.append(one.coeff)
        cur = one.not_plane
    got = ctx.plane_peel(ctx.upload(pts), p, want_cloud=True)
    assert np.asarray(coeffs, np.float32).tobytes() == got.coeffs.tobytes() and len(coeffs) == 3
    assert cur.n == got.rest.n and ctx.download(cur).tobytes() == ctx.download(got.rest).tobytes()


def test_degenerate_clouds(ctx):
    ope = load_pkg()
    for pts, planes, stop, rest in ((np.zeros((0, 3), np.float32), 0, pf.FRACTION, 0),
                                    (np.array([[0, 0, 1], [1, 0, 1.5], [0, 1, 2]], np.float32), 1, pf.FRACTION, 0),
                                    (np.tile(np.array([[0.25, -1.0, 2.0]], np.float32), (500, 1)), 0, pf.NO_INLIERS, 500)):
        want = pf.peel(pts)
        assert (len(want["coeffs"]), want["stop"], len(want["rest_idx"])) == (planes, stop, rest)
        check(ctx, pts, want)
    assert (ope.PEEL_FRACTION, ope.PEEL_NO_INLIERS, ope.PEEL_MAX_PLANES) == (pf.FRACTION, pf.NO_INLIERS, pf.MAX_PLANES)


@pytest.mark.parametrize("seed", SEEDS)
def test_structureless_noise_with_nan_rows(ctx, seed):
    # about twenty rounds: a wrong double-buffer swap or a stale m does not survive them
    pts, bad = noise_with_nans()
    want = pf.peel(pts, seed=seed)
    assert len(want["coeffs"]) in (19, 20) and np.isin(bad, want["rest_idx"]).all()
    got = check(ctx, pts, want, seed=seed)
    assert np.isin(bad, got.rest_idx).all() and (got.labels[bad] == -1).all()


def _raw_peel(ctx, cloud, plane=None, peel=None, cap=0, coeffs=None, counts=None, its=None, label=None, rest_idx=None, want_rest=True):
    ope = load_pkg()
    lib = C.CDLL(ope.LIB_PATH)
    lib.ope_plane_peel.restype = C.c_int
    r = ope.PeelResult(-7, -7, -7, -7, -7)
    h = C.c_void_p(0x1234)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = lib.ope_plane_peel(ctx.h, cloud.h, C.byref(plane) if plane is not None else None, C.byref(peel) if peel is not None else None,
                            C.c_size_t(cap), ptr(coeffs, C.c_float), ptr(counts, C.c_int32), ptr(its, C.c_int64), ptr(label, C.c_int32),
                            ptr(rest_idx, C.c_int32), C.byref(h) if want_rest else None, C.byref(r))
    return rc, r, h


def test_cap_planes_smaller_than_the_planes_peeled(ctx):
    ope = load_pkg()
    pts, want = ref_of("three", 1)
    assert len(want["coeffs"]) == 3
    cloud = ctx.upload(pts)
    coeffs = np.full((3, 4), -77.0, np.float32)
    counts = np.full(3, -77, np.int32)
    its = np.full(3, -77, np.int64)
    rc, r, h = _raw_peel(ctx, cloud, ope.default_plane_params(seed=1), None, 2, coeffs, counts, its)
    assert rc == 0 and r.n_planes == 3 and r.n_rest == 4000 and r.stop == pf.FRACTION
    ope.Cloud(ctx, h, r.n_rest).free()
    assert coeffs[:2].tobytes() == want["coeffs"][:2].tobytes() and (coeffs[2] == -77.0).all()
    assert counts.tolist() == want["counts"][:2].tolist() + [-77]
    assert its.tolist() == want["iterations"][:2].tolist() + [-77]


def test_launches_and_syncs_per_plane_are_constant(ctx):
    ope = load_pkg()
    seen = {}
    for n, scale in ((20000, 1.0), (5000, 0.25)):   # the same make-up at a quarter of the points
        pts = room_scene(SCENES["three"], scale=scale)
        want = pf.peel(pts, seed=1)
        assert len(want["coeffs"]) == 3 and len(pts) == n
        cloud = ctx.upload(pts)
        for k in (1, 2, 3):
            got = ctx.plane_peel(cloud, ope.default_plane_params(seed=1), max_planes=k, want_cloud=True, want_labels=True)
            assert got.stats["n_planes"] == k
            seen[(n, k)] = (got.stats["launches"], got.stats["host_syncs"])
    print("[peel] launches, syncs:", seen)
    for n in (20000, 5000):
        (l1, s1), (l2, s2), (l3, s3) = (seen[(n, k)] for k in (1, 2, 3))
        assert l2 - l1 == l3 - l2 > 0 and s2 - s1 == s3 - s2 and 0 < s2 - s1 <= 2
    assert all(seen[(20000, k)] == seen[(5000, k)] for k in (1, 2, 3))
    one = ctx.plane_segment(ctx.upload(pts), ope.default_plane_params(seed=1))
    assert seen[(5000, 2)][0] - seen[(5000, 1)][0] <= one.stats["launches"]   # a round costs no more launches than one plane_segment fit


def test_bad_arguments_launch_nothing(ctx):
    ope = load_pkg()
    cloud = ctx.upload(room_scene(SCENES["three"])[:1000])
    bad = [(ope.default_plane_params(distance_threshold=-1.0), None), (ope.default_plane_params(probability=1.0), None),
           (ope.default_plane_params(max_iterations=1024), None), (None, ope.PeelParams(float("nan"), 0)), (None, ope.PeelParams(-0.1, 0)),
           (None, ope.PeelParams(float("inf"), 0)), (None, ope.PeelParams(0.3, -1))]
    for plane, peel in bad:
        rc, r, h = _raw_peel(ctx, cloud, plane, peel)
        assert rc == -1   # OPE_EINVAL
        assert h.value is None
        assert (r.n_planes, r.n_rest, r.stop, r.launches, r.host_syncs) == (0, 0, 0, 0, 0)
        st = ctx.plane_stats()
        assert st["launches"] == 0 and st["host_syncs"] == 0
    with pytest.raises(ope.OpeError):
        ctx.plane_peel(cloud, keep_fraction=-1.0)
