"""ope_mls_upsample / ope_mls_upsample_cloud against tests/mls_upsample_ref.py (pcl::MovingLeastSquares with upsampling
VOXEL_GRID_DILATION in numpy float64 / float32).

The cloud: mls_upsample_ref.upsample_cloud (two surfaces of 1 500 points, isolated points, pairs, triples, quintuples, 10 exact
duplicates, 7 non-finite points), radius 0.03, order 4, voxel 0.002.  Figures of the reference itself, computed on the CPU
(tests/test_mls_upsample_ref.py asserts them, so the cloud cannot silently stop covering them): neighbour counts of the surface
points 25..114, median 82, 68 % at or above 5 nr_coeff = 75; 2 899 voxels without dilation and 52 685 with one round; the keep rule
drops 862 (30 %) and 9 686 (18 %) of them; 9 and 207 voxels have an invalid nearest point.
Undecided voxels (|d_before - d_after| <= 8 float ulps of d_before in the reference; the device may keep or drop them, every other
voxel must agree): 0 of 2 899 and 2 of 52 685 (0.004 %), far below the 1 % the comparison tolerates.

Exact: n_voxels, data_size, n_valid, n_invalid_nearest, n_polynomial, and the sequence of idx over the decided voxels.
Floating point: the device accumulates the same fp64 sums in another order (tree walks, P W P^T from moments) and both sides round to
float.  MEASURED on an MI355X (gfx950, ROCm 7.2) on the decided voxels of this cloud, 0 and 1 dilation rounds, largest difference per
component:
    positions 0.0 m, normals (up to sign) 0.0, curvature 0.0
-- the fp64 differences never reached a float rounding boundary in the values compared (2 028 and 42 792 output points), and the device
decided the two undecided voxels as the reference did.  The base-cloud test asserts 4 x those, i.e. equality; that is below 1/100 of the
reference's median |result - pos| (1.07e-3 m and 1.64e-3 m) and of its median |n_disp| over the polynomial voxels (1.91e-3 m and 1.89e-3 m),
so neither an identity nor a plane-only result can pass.  A measured bound of 0 leaves no room for what the measurement did not vary: if
the base-cloud test turns red by ONE float ulp in a few values after a change of the device library's exp / atan2 / cos / sin or of the
tree (another order of the sums), that means "measure again and write the new figures here", not "the kernel is wrong"; anything larger
than an ulp is a bug.  Clouds outside that measurement get `within_one_ulp` and nothing wider.
"""
import ctypes as C

import numpy as np
import pytest

import mls_ref
import mls_upsample_ref as R
from mls_upsample_ref import ORDER, RADIUS, VOXEL

pytestmark = pytest.mark.gpu

# largest |device - reference| per component over the decided voxels of the base cloud (0 and 1 dilation rounds together), measured
# on an MI355X (gfx950, ROCm 7.2)
POS_MEASURED = 0.0     # metres
NRM_MEASURED = 0.0
CURV_MEASURED = 0.0


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base():
    xyz, n_surface = R.upsample_cloud()
    nbh = mls_ref.neighbourhoods(xyz, RADIUS)
    res = R.mls_results(xyz, RADIUS, ORDER, nbh=nbh)
    ref = [R.mls_upsample(xyz, RADIUS, ORDER, compute_normals=True, voxel_size=VOXEL, dilation_iterations=it, results=res) for it in (0, 1)]
    return dict(xyz=xyz, n_surface=n_surface, nbh=nbh, res=res, ref=ref)


def up_to_sign(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    if len(a) == 0:
        return 0.0
    return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max())


def within_one_ulp(a, b, signed=True):
    """Every component of float32 a equals b or its float neighbour; signed=False: unit vectors that may also match with the opposite
    sign, a component that cancels to zero in fp64 compared absolutely at 1e-15 (tests/test_gpu_mls.py)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    if signed:
        return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol).all())
    tol = np.maximum(tol, 1e-15)
    ok = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol
    ko = np.abs(a.astype(np.float64) + b.astype(np.float64)) <= tol
    return bool((ok.all(axis=1) | ko.all(axis=1)).all())


def align(ref, dev_xyz, dev_idx):
    """Row of the device output for every voxel of the reference (-1: absent), walking both in key order.  A decided voxel must be
    present exactly when the reference keeps it; an undecided one counts as present when the next device row has its nearest point and
    lies within 1e-6 m of its reference result (neighbouring voxels' results lie a voxel, 2e-3 m, apart).  Asserts that nothing is left over."""
    und = R.undecided(ref)
    at = np.full(len(ref["keys"]), -1, np.int64)
    d = 0
    for t in np.flatnonzero(ref["near_valid"] & (ref["keep"] | und)):
        here = d < len(dev_idx) and dev_idx[d] == ref["nearest"][t] and np.abs(dev_xyz[d].astype(np.float64) - ref["result"][t]).max() <= 1e-6
        if und[t] and not here:
            continue
        assert here, f"voxel {t} (key {ref['keys'][t]}): expected idx {ref['nearest'][t]} at output row {d}"
        at[t] = d
        d += 1
    assert d == len(dev_idx), f"{len(dev_idx) - d} output rows beyond the reference's voxels"
    return at, und


def check_exact(stats, ref, und):
    rs = ref["stats"]
    for k in ("n_in", "n_valid", "n_voxels", "n_invalid_nearest", "n_polynomial", "data_size"):
        assert stats[k] == rs[k], (k, stats[k], rs[k])
    assert abs(stats["n_out"] - rs["n_out"]) <= int(und.sum()) and stats["n_out"] + stats["n_rejected_farther"] + stats["n_invalid_nearest"] == stats["n_voxels"]
    assert und.sum() <= 0.01 * max(len(und), 1)


def diffs(ref, at, und, xyz, nrm, curv):
    sel = (at >= 0) & ~und
    rows = at[sel]
    dp = float(np.abs(xyz[rows].astype(np.float64) - ref["result"][sel].astype(np.float64)).max()) if sel.any() else 0.0
    dn = up_to_sign(nrm[rows], ref["normal"][sel])
    rc = ref["curvature_vox"][sel]
    dc = float(np.abs(curv[rows].astype(np.float64) - rc.astype(np.float64)).max()) if sel.any() else 0.0
    return sel, rows, dp, dn, dc


@pytest.mark.parametrize("it", [0, 1])
def test_base_cloud_against_the_reference(ope, ctx, base, it):
    ref = base["ref"][it]
    xyz, idx, nrm, curv = ctx.mls_upsample(ctx.upload(base["xyz"]), RADIUS, order=ORDER, voxel_size=VOXEL, dilation_iterations=it, compute_normals=True)
    stats = ctx.mls_upsample_stats()
    at, und = align(ref, xyz, idx)
    check_exact(stats, ref, und)
    sel, rows, dp, dn, dc = diffs(ref, at, und, xyz, nrm, curv)
    assert np.array_equal(idx[rows], ref["nearest"][sel])
    moved = np.linalg.norm(ref["result"][ref["near_valid"]].astype(np.float64) - ref["pos"][ref["near_valid"]], axis=1)
    ndisp = np.abs(ref["n_disp"][ref["applied"]])
    print(f"\n[mls_upsample] base cloud, {it} dilation(s): {stats}\n  max |d position| = {dp:.7e} m, max |d normal| = {dn:.7e}, max |d curvature| = {dc:.7e}; "
          f"undecided voxels {int(und.sum())} of {len(und)}; median |result - pos| = {np.median(moved):.4e} m, median |n_disp| = {np.median(ndisp):.4e} m")
    assert 4 * POS_MEASURED <= np.median(moved) / 100    # an identity (result = voxel position) cannot pass
    assert 4 * POS_MEASURED <= np.median(ndisp) / 100    # nor can a plane-only result
    assert dp <= 4 * POS_MEASURED
    assert dn <= 4 * NRM_MEASURED
    assert dc <= 4 * CURV_MEASURED


OPTIONS = [dict(order=0), dict(order=1), dict(order=2), dict(order=3), dict(order=4), dict(polynomial_fit=False), dict(dilation_iterations=1),
           dict(sqr_gauss_param=4e-4), dict(compute_normals=False)]


@pytest.mark.parametrize("kw", OPTIONS, ids=["order0", "order1", "order2", "order3", "order4", "plane", "dilate1", "gauss", "normals_off"])
def test_options(ope, ctx, kw):
    rng = np.random.default_rng(21)
    pts = np.r_[mls_ref.paraboloid_patch(rng, 900, side=0.13), mls_ref.sphere_points(rng, 500, max_polar=np.radians(40.0))]
    args = dict(order=2, polynomial_fit=True, compute_normals=True, sqr_gauss_param=None, voxel_size=0.004, dilation_iterations=0)
    args.update(kw)
    ref = R.mls_upsample(pts, RADIUS, **args)
    xyz, idx, nrm, curv = ctx.mls_upsample(ctx.upload(pts), RADIUS, **args)
    stats = ctx.mls_upsample_stats()
    at, und = align(ref, xyz, idx)
    check_exact(stats, ref, und)
    sel, rows, dp, dn, dc = diffs(ref, at, und, xyz, nrm, curv)
    print(f"\n[mls_upsample] {kw}: {stats}\n  max |d position| = {dp:.3e} m, max |d normal| = {dn:.3e}, max |d curvature| = {dc:.3e}, undecided {int(und.sum())}")
    assert stats["n_out"] > 100 and np.array_equal(idx[rows], ref["nearest"][sel])
    assert within_one_ulp(xyz[rows], ref["result"][sel]) and within_one_ulp(curv[rows], ref["curvature_vox"][sel])
    assert within_one_ulp(nrm[rows], ref["normal"][sel], signed=False)
    if kw.get("polynomial_fit", True) is False:
        assert stats["n_polynomial"] == 0
    elif args["order"] <= 2:
        assert stats["n_polynomial"] > 0


def test_host_form_equals_cloud_form_and_colours_travel(ope, ctx, base):
    pts = base["xyz"]
    rgb = (np.arange(len(pts), dtype=np.uint64) * 2654435761 & 0xffffffff).astype(np.uint32)
    cloud = ctx.upload(pts)
    cloud.set_rgb(rgb)
    kw = dict(order=ORDER, voxel_size=VOXEL, compute_normals=True)
    xyz, idx, nrm, curv = ctx.mls_upsample(cloud, RADIUS, **kw)
    out, idx2 = ctx.mls_upsample(cloud, RADIUS, as_cloud=True, **kw)
    assert out.n == len(idx) > 1000 and np.array_equal(idx, idx2)
    assert ctx.download(out).tobytes() == xyz.tobytes() and np.isfinite(xyz).all()
    assert out.has_rgb and np.array_equal(out.download_rgb(), rgb[idx])
    n_dev, c_dev = out.download_normals()
    assert n_dev.tobytes() == nrm.tobytes() and c_dev.tobytes() == curv.tobytes()
    # the output is a cloud like any other: an index builds over it and generateMesh's k = 20 normals are estimated on it
    ix = ctx.build_index(out)
    n2, _ = ctx.normals(out, k=20)
    assert np.isfinite(n2).all()
    ix.free()
    plain, _ = ctx.mls_upsample(ctx.upload(pts), RADIUS, as_cloud=True, order=ORDER, voxel_size=VOXEL)
    assert not plain.has_rgb and ctx.download(plain).tobytes() == xyz.tobytes()
    with pytest.raises(ope.OpeError):   # normals were not asked for: none attached
        plain.download_normals()
    # normals off, host form: the same points and the plane's normal of point idx
    xyz0, idx0, nrm0, curv0 = ctx.mls_upsample(ctx.upload(pts), RADIUS, order=ORDER, voxel_size=VOXEL)
    assert xyz0.tobytes() == xyz.tobytes() and np.array_equal(idx0, idx) and curv0.tobytes() == curv.tobytes()
    assert up_to_sign(nrm0, base["res"]["n"][idx].astype(np.float32)) == 0.0


def test_determinism_and_upload_order(ope, ctx, base):
    pts = base["xyz"]
    kw = dict(order=ORDER, voxel_size=VOXEL, compute_normals=True, dilation_iterations=1)
    a = ctx.mls_upsample(ctx.upload(pts), RADIUS, **kw)
    b = ctx.mls_upsample(ctx.upload(pts), RADIUS, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # the same cloud uploaded in another order, without the duplicated points (a tie goes to the lowest index, which a shuffle changes)
    fin = np.isfinite(pts).all(axis=1)
    _, first = np.unique(pts[fin], axis=0, return_index=True)
    keep = np.sort(np.r_[np.flatnonzero(fin)[first], np.flatnonzero(~fin)])
    assert len(keep) == len(pts) - 10
    sub = pts[keep]
    perm = np.random.default_rng(5).permutation(len(sub))
    c = ctx.mls_upsample(ctx.upload(sub), RADIUS, **kw)
    d = ctx.mls_upsample(ctx.upload(sub[perm]), RADIUS, **kw)
    assert np.array_equal(perm[d[1]], c[1])
    assert c[0].tobytes() == d[0].tobytes() and c[2].tobytes() == d[2].tobytes() and c[3].tobytes() == d[3].tobytes()


def test_a_duplicated_point_goes_to_the_lower_index(ope, ctx, base):
    pts = base["xyz"]
    xyz, idx, _, _ = ctx.mls_upsample(ctx.upload(pts), RADIUS, order=ORDER, voxel_size=VOXEL)
    fin = np.flatnonzero(np.isfinite(pts).all(axis=1))
    _, inv, cnt = np.unique(pts[fin], axis=0, return_inverse=True, return_counts=True)
    later = set()
    for g in np.flatnonzero(cnt > 1):
        later.update(fin[np.flatnonzero(inv == g)][1:].tolist())
    assert len(later) == 10 and not later.intersection(idx.tolist())
    assert np.array_equal(idx, base["ref"][0]["idx"]) or R.undecided(base["ref"][0]).any()


@pytest.mark.parametrize("pts", [np.zeros((0, 3), np.float32), np.full((9, 3), np.nan, np.float32), np.array([[0.5, 0.5, 1.0]], np.float32)],
                         ids=["empty", "non_finite", "single"])
def test_clouds_without_a_result(ope, ctx, pts):
    for it in (0, 1):
        xyz, idx, nrm, curv = ctx.mls_upsample(ctx.upload(pts), RADIUS, order=ORDER, voxel_size=VOXEL, dilation_iterations=it, compute_normals=True)
        st = ctx.mls_upsample_stats()
        assert len(xyz) == len(idx) == len(nrm) == len(curv) == 0 and st["n_out"] == 0 and st["n_in"] == len(pts) and st["n_valid"] == 0
        ref = R.mls_upsample(pts, RADIUS, ORDER, voxel_size=VOXEL, dilation_iterations=it)
        assert st["n_voxels"] == ref["stats"]["n_voxels"] and st["data_size"] == ref["stats"]["data_size"]
        coloured = ctx.upload(pts)
        coloured.set_rgb(np.arange(len(pts), dtype=np.uint32))
        out, _ = ctx.mls_upsample(coloured, RADIUS, order=ORDER, voxel_size=VOXEL, dilation_iterations=it, as_cloud=True)
        assert out.n == 0 and out.has_rgb


def test_capacity_too_small_says_what_it_needs(ope, ctx, base):
    L = ope.lib()
    cloud = ctx.upload(base["xyz"])
    p = ope.default_mls_upsample_params(radius=RADIUS, order=ORDER, voxel_size=VOXEL)
    need = base["ref"][0]["stats"]["n_out"]
    n = C.c_size_t(0)
    xyz = np.full((need, 3), 7.0, np.float32)
    fp = xyz.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ope_mls_upsample(ctx.h, cloud.h, C.byref(p), fp, None, None, None, need - 1, C.byref(n)) == ope.OPE_EINVAL
    assert n.value == need and (xyz == 7.0).all()                                  # nothing was copied
    assert L.ope_mls_upsample(ctx.h, cloud.h, C.byref(p), None, None, None, None, 0, C.byref(n)) == ope.OPE_OK and n.value == need   # counting only
    assert L.ope_mls_upsample(ctx.h, cloud.h, C.byref(p), fp, None, None, None, need, C.byref(n)) == ope.OPE_OK and n.value == need
    assert xyz.tobytes() == base["ref"][0]["xyz"].tobytes() or POS_MEASURED > 0 or R.undecided(base["ref"][0]).any()
    h = C.c_void_p()
    idx = np.empty(need, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.ope_mls_upsample_cloud(ctx.h, cloud.h, C.byref(p), C.byref(h), ip, need - 1, C.byref(n)) == ope.OPE_EINVAL and not h.value and n.value == need


def test_bad_arguments_launch_nothing(ope, ctx):
    cloud = ctx.upload(np.zeros((4, 3), np.float32))
    wide = ctx.upload(np.array([[0, 0, 0], [1, 1, 1]], np.float32))
    L = ope.lib()
    n = C.c_size_t(7)
    ctx.profile_kernels(True)
    P = lambda **kw: ope.default_mls_upsample_params(**dict(dict(radius=0.03, voxel_size=0.002), **kw))
    bad = [P(radius=0.0), P(radius=-1.0), P(radius=float("nan")), P(order=5), P(order=-1), P(voxel_size=0.0), P(voxel_size=-0.002),
           P(voxel_size=float("nan")), P(voxel_size=float("inf")), P(dilation_iterations=-1), P(dilation_iterations=9), P(sqr_gauss_param=-1.0)]
    for p in bad:
        assert L.ope_mls_upsample(ctx.h, cloud.h, C.byref(p), None, None, None, None, 0, C.byref(n)) == ope.OPE_EINVAL and n.value == 0
        h = C.c_void_p()
        assert L.ope_mls_upsample_cloud(ctx.h, cloud.h, C.byref(p), C.byref(h), None, 0, C.byref(n)) == ope.OPE_EINVAL and not h.value
    # a grid more than 2^21 voxels wide: 1.5 * 1 m / 1e-7 m
    assert L.ope_mls_upsample(ctx.h, wide.h, C.byref(P(voxel_size=1e-7)), None, None, None, None, 0, C.byref(n)) == ope.OPE_EINVAL
    assert L.ope_mls_upsample(ctx.h, cloud.h, None, None, None, None, None, 0, C.byref(n)) == ope.OPE_EINVAL
    assert L.ope_mls_upsample(ctx.h, cloud.h, C.byref(P()), None, None, None, None, 0, None) == ope.OPE_EINVAL
    # the smoothing entry keeps its own range of orders
    with pytest.raises(ope.OpeError):
        ctx.mls_smooth(cloud, 0.02, order=3)
    assert not any(k.startswith("mls_") for k in ctx.profile_kernels_read())
    ctx.profile_kernels(False)


def test_launches_do_not_depend_on_the_points(ope, ctx, base):
    pts = base["xyz"]
    fin = pts[np.isfinite(pts).all(axis=1)]
    for it in (0, 1, 2):
        seen = []
        for cloud in (pts, fin[:300]):
            ctx.mls_upsample(ctx.upload(cloud), RADIUS, order=ORDER, voxel_size=VOXEL, dilation_iterations=it)
            st = ctx.mls_upsample_stats()
            seen.append((st["launches"], st["host_syncs"]))
        assert seen[0] == seen[1] and seen[0][1] == 3 + it
