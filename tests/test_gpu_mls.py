"""ope_mls_smooth / ope_mls_smooth_cloud against tests/mls_ref.py (pcl::MovingLeastSquares with upsampling NONE in numpy float64).

Exact: the output indices, the count and every field of the statistics.  Floating point: the device accumulates the same sums in
another order (two tree walks instead of a sorted list), builds P W P^T from moments, and calls the device library's exp, atan2, cos
and sin; both sides then round fp64 results to float.  MEASURED on an MI355X (gfx950, ROCm 7.2) against the reference on the base
cloud (5 545 points, the 2 500-point clump included), largest difference per component:
    positions 0.0 m, curvature 0.0, normals (up to sign) 0.0
-- the fp64 differences (~1e-16 relative) never reached a float rounding boundary in the 38 703 values compared.  The base-cloud test
asserts 4 x those, i.e. equality; that is trivially below 1/100 of the median displacement the reference applies (5.36e-4 m), so neither
an identity nor a plane-only result can pass.  The other clouds of this file were not part of that measurement: there a value may
differ where the two fp64 results straddle a float rounding boundary (~1e-8 of the values), and then by exactly one float ulp of
that value, which is what `within_one_ulp` allows -- the precision of the output format, nothing wider.
A measured bound of 0 leaves no room for what the measurement did not vary: if the base-cloud test turns red by ONE float ulp in a few
values after a change of the device library's exp / atan2 / cos / sin or of the tree (leaf size, Morton order: another order of the
sums), that means "measure again and write the new figures here", not "the kernel is wrong"; anything larger than an ulp is a bug.
(At 0 the condition `4 x bound <= median displacement / 100` holds trivially; it is kept for the figures that follow a re-measurement.)
Denoising, noisy sphere (sigma 0.5 mm, R 0.1 m, radius 0.02): RMS radial error after / before 0.493227 for the reference and
0.493227 for the device; asserted <= 1.05 x the reference's.
"""
import ctypes as C

import numpy as np
import pytest

import mls_ref
from mls_ref import RADIUS

pytestmark = pytest.mark.gpu

# largest |device - reference| per component on the base cloud, measured on an MI355X (gfx950, ROCm 7.2)
POS_MEASURED = 0.0     # metres
CURV_MEASURED = 0.0
NRM_MEASURED = 0.0
SPHERE_RATIO_MEASURED = 0.493227
SPHERE_RATIO_REFERENCE = 0.493227


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base():
    xyz, _ = mls_ref.base_cloud()
    nbh = mls_ref.neighbourhoods(xyz, RADIUS)
    ref = mls_ref.mls_smooth(xyz, RADIUS, compute_normals=True, nbh=nbh)
    return dict(xyz=xyz, nbh=nbh, ref=ref)


def up_to_sign(a, b):
    """max |a - (+-)b| per row-wise best sign"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max())


def within_one_ulp(a, b, signed=True):
    """Every component of float32 a equals b or its float neighbour; signed=False: rows are (near-)unit vectors that may also match
    with the opposite sign, and a component that cancels to zero in fp64 (a normal along an axis: 0 on one side, 2e-17 on the other)
    is compared absolutely at 1e-15, four fp64 epsilons of the vector's length -- nine orders below a float ulp of that length."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    if signed:
        return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol).all())
    tol = np.maximum(tol, 1e-15)
    ok = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol
    ko = np.abs(a.astype(np.float64) + b.astype(np.float64)) <= tol
    return bool((ok.all(axis=1) | ko.all(axis=1)).all())


def test_radius_boundary_is_clear(base):
    assert mls_ref.pairs_near_radius(base["xyz"], RADIUS, ulps=4) == 0   # nothing is excluded from the comparison
    counts = np.diff(base["nbh"][1])
    assert counts.max() >= 2500 and np.count_nonzero(counts < 3) >= 9 and np.count_nonzero((counts >= 3) & (counts < 6)) >= 10


def test_base_cloud_against_the_reference(ope, ctx, base):
    ref = base["ref"]
    xyz, idx, nrm, curv = ctx.mls_smooth(ctx.upload(base["xyz"]), RADIUS, compute_normals=True)
    assert np.array_equal(idx, ref["idx"]) and len(xyz) == ref["stats"]["n_out"]
    assert ctx.mls_stats() == ref["stats"]
    assert ref["stats"]["n_dropped"] == 16 and ref["stats"]["n_plane_only"] == 19
    dp = float(np.abs(xyz.astype(np.float64) - ref["xyz"].astype(np.float64)).max())
    dc = float(np.abs(curv.astype(np.float64) - ref["curvature"].astype(np.float64)).max())
    dn = up_to_sign(nrm, ref["normals"])
    disp = np.linalg.norm(ref["xyz64"] - base["xyz"][ref["idx"]].astype(np.float64), axis=1)
    moved = float(np.linalg.norm(xyz.astype(np.float64) - base["xyz"][idx].astype(np.float64), axis=1).max())
    print(f"\n[mls] base cloud: max |d position| = {dp:.7e} m, max |d curvature| = {dc:.7e}, max |d normal| = {dn:.7e}; "
          f"median displacement of the reference = {np.median(disp):.4e} m, largest device displacement = {moved:.4e} m")
    assert 4 * POS_MEASURED <= np.median(disp) / 100
    assert dp <= 4 * POS_MEASURED
    assert dc <= 4 * CURV_MEASURED
    assert dn <= 4 * NRM_MEASURED


def test_host_form_equals_cloud_form_and_colours_travel(ope, ctx, base):
    pts = base["xyz"]
    rgb = (np.arange(len(pts), dtype=np.uint64) * 2654435761 & 0xffffffff).astype(np.uint32)
    cloud = ctx.upload(pts)
    cloud.set_rgb(rgb)
    xyz, idx, nrm, curv = ctx.mls_smooth(cloud, RADIUS, compute_normals=True)
    out, idx2 = ctx.mls_smooth(cloud, RADIUS, compute_normals=True, as_cloud=True)
    assert out.n == len(idx) and np.array_equal(idx, idx2)
    assert ctx.download(out).tobytes() == xyz.tobytes()
    assert out.has_rgb and np.array_equal(out.download_rgb(), rgb[idx])
    assert np.isfinite(xyz).all()
    n_dev, c_dev = out.download_normals()   # the attached normals and their fourth component are the host form's, byte for byte
    assert n_dev.tobytes() == nrm.tobytes() and c_dev.tobytes() == curv.tobytes()
    # the output is a cloud like any other: an index builds over it and normals are estimated on it
    ix = ctx.build_index(out)
    n2, _ = ctx.normals(out, k=12)
    assert np.isfinite(n2).all()
    ix.free()
    plain, _ = ctx.mls_smooth(ctx.upload(pts), RADIUS, as_cloud=True)
    assert not plain.has_rgb and ctx.download(plain).tobytes() == xyz.tobytes()
    with pytest.raises(ope.OpeError):   # normals were not asked for: none attached
        plain.download_normals()


@pytest.mark.parametrize("kw", [dict(order=0), dict(order=1), dict(order=2), dict(polynomial_fit=False), dict(sqr_gauss_param=1e-4)],
                         ids=["order0", "order1", "order2", "plane", "gauss"])
def test_options(ope, ctx, kw):
    rng = np.random.default_rng(21)
    pts = np.r_[mls_ref.paraboloid_patch(rng, 700, side=0.13), mls_ref.sphere_points(rng, 500, max_polar=np.radians(50.0))]
    ref = mls_ref.mls_smooth(pts, RADIUS, compute_normals=True, **kw)
    cloud = ctx.upload(pts)
    xyz, idx, nrm, curv = ctx.mls_smooth(cloud, RADIUS, compute_normals=True, **kw)
    assert np.array_equal(idx, ref["idx"]) and ctx.mls_stats() == ref["stats"]
    print(f"\n[mls] {kw}: max |d position| = {np.abs(xyz.astype(np.float64) - ref['xyz']).max():.3e} m, max |d curvature| = "
          f"{np.abs(curv.astype(np.float64) - ref['curvature']).max():.3e}, max |d normal| = {up_to_sign(nrm, ref['normals']):.3e}")
    assert within_one_ulp(xyz, ref["xyz"]) and within_one_ulp(curv, ref["curvature"]) and within_one_ulp(nrm, ref["normals"], signed=False)
    # normals off: the same positions byte for byte, and the plane's normal
    xyz0, idx0 = ctx.mls_smooth(cloud, RADIUS, **kw)
    assert xyz0.tobytes() == xyz.tobytes() and np.array_equal(idx0, idx)
    if kw.get("polynomial_fit", True) is False:
        assert ref["stats"]["n_plane_only"] == ref["stats"]["n_out"]


def test_determinism_and_independence_of_far_points(ope, ctx, base):
    pts = base["xyz"]
    a = ctx.mls_smooth(ctx.upload(pts), RADIUS, compute_normals=True)
    b = ctx.mls_smooth(ctx.upload(pts), RADIUS, compute_normals=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    far = np.random.default_rng(4).uniform(30.0, 40.0, (100, 3)).astype(np.float32)   # another tree, another order of the sums
    c = ctx.mls_smooth(ctx.upload(np.r_[pts, far]), RADIUS, compute_normals=True)
    m = len(a[1])
    assert np.array_equal(c[1][:m], a[1])
    assert c[0][:m].tobytes() == a[0].tobytes() and c[2][:m].tobytes() == a[2].tobytes() and c[3][:m].tobytes() == a[3].tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_clouds(ope, ctx, n):
    pts = np.array([[0.5, 0.5, 1.0], [0.505, 0.5, 1.0], [0.5, 0.505, 1.001]], np.float32)[:n].reshape(n, 3)
    ref = mls_ref.mls_smooth(pts, RADIUS, compute_normals=True)
    xyz, idx, nrm, curv = ctx.mls_smooth(ctx.upload(pts), RADIUS, compute_normals=True)
    assert np.array_equal(idx, ref["idx"]) and ctx.mls_stats() == ref["stats"] and len(idx) == (3 if n == 3 else 0)
    if n == 3:
        assert within_one_ulp(xyz, ref["xyz"]) and within_one_ulp(nrm, ref["normals"], signed=False)
    out, idx2 = ctx.mls_smooth(ctx.upload(pts), RADIUS, as_cloud=True)
    assert out.n == len(idx) and not out.has_rgb
    coloured = ctx.upload(pts)
    coloured.set_rgb(np.arange(n, dtype=np.uint32))
    out, _ = ctx.mls_smooth(coloured, RADIUS, as_cloud=True)
    assert out.n == len(idx) and out.has_rgb


def test_all_non_finite_cloud(ope, ctx):
    pts = np.full((9, 3), np.nan, np.float32)
    pts[3] = [np.inf, 0, 0]
    xyz, idx = ctx.mls_smooth(ctx.upload(pts), RADIUS)
    assert len(idx) == 0 and ctx.mls_stats() == dict(n_in=9, n_out=0, n_plane_only=0, n_dropped=9, neighbours_total=0)
    out, _ = ctx.mls_smooth(ctx.upload(pts), RADIUS, as_cloud=True)
    assert out.n == 0


def test_bad_arguments_launch_nothing(ope, ctx):
    cloud = ctx.upload(np.zeros((4, 3), np.float32))
    L = ope.lib()
    n = C.c_size_t(7)
    ctx.profile_kernels(True)
    for p in (ope.default_mls_params(radius=0.0), ope.default_mls_params(radius=-1.0), ope.default_mls_params(radius=0.02, order=3),
              ope.default_mls_params(radius=0.02, order=-1), ope.default_mls_params(radius=float("nan"))):
        assert L.ope_mls_smooth(ctx.h, cloud.h, C.byref(p), None, None, None, None, C.byref(n)) == ope.OPE_EINVAL and n.value == 0
        h = C.c_void_p()
        assert L.ope_mls_smooth_cloud(ctx.h, cloud.h, C.byref(p), C.byref(h), None, C.byref(n)) == ope.OPE_EINVAL and not h.value
    assert L.ope_mls_smooth(ctx.h, cloud.h, None, None, None, None, None, C.byref(n)) == ope.OPE_EINVAL
    assert L.ope_mls_smooth(ctx.h, cloud.h, C.byref(ope.default_mls_params(radius=0.02)), None, None, None, None, None) == ope.OPE_EINVAL
    assert not any(k.startswith("mls_") for k in ctx.profile_kernels_read())
    ctx.profile_kernels(False)


def test_collinear_points_stay_finite_and_near(ope, ctx):
    # rank-deficient neighbourhoods: Eigen's result is not defined well enough to compare; the outputs must be finite and within the radius
    d = np.array([0.48, -0.6, 0.64])
    pts = (np.array([0.7, 0.8, 0.9]) + np.linspace(-0.008, 0.008, 8)[:, None] * d).astype(np.float32)
    xyz, idx = ctx.mls_smooth(ctx.upload(pts), RADIUS)
    assert len(idx) == 8 and np.isfinite(xyz).all()
    assert np.linalg.norm(xyz.astype(np.float64) - pts[idx], axis=1).max() <= RADIUS


def test_denoises_a_noisy_sphere_as_the_reference_does(ope, ctx):
    pts = mls_ref.sphere_points(np.random.default_rng(mls_ref.BASE_SEED), 2000)
    ref = mls_ref.mls_smooth(pts, RADIUS)
    xyz, idx = ctx.mls_smooth(ctx.upload(pts), RADIUS)
    assert np.array_equal(idx, ref["idx"])
    before = mls_ref.radial_rms(pts[idx])
    ratio_ref, ratio_dev = mls_ref.radial_rms(ref["xyz"]) / before, mls_ref.radial_rms(xyz) / before
    print(f"\n[mls] noisy sphere: RMS radial error after / before: reference {ratio_ref:.6f}, device {ratio_dev:.6f}")
    assert abs(ratio_ref - SPHERE_RATIO_REFERENCE) < 5e-6 and abs(ratio_dev - SPHERE_RATIO_MEASURED) < 5e-6   # (tests/test_mls_ref.py prints the former)
    assert ratio_dev <= 1.05 * ratio_ref
