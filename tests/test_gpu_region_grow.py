"""Region growing on the device (ope_region_grow, ope_region_grow_cloud) against the host reference (tests/region_grow_ref.py: a
literal, sequential restatement of pcl::RegionGrowing over oracle k-NN lists and oracle normals).  Everything is compared exactly:
clusters, offsets, labels and the count.  The scenes meet the conditions test_region_grow_ref.py checks on the CPU (distinct
curvatures, no boundary tie in a k-NN list, no edge within 4 ulp of the cosine threshold), so that an exact answer exists.

One case differs from its description in the issue by arithmetic alone: against its links the 2 000-point chain gives 1 998
singletons and the pair {0, 1}, not 2 000 singletons — the closest pair of any point set is mutual (tests/region_grow_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import region_grow_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


def _params(ope, scene, **kw):
    args = dict(number_of_neighbours=scene.k, smoothness_threshold=scene.theta, min_size=1)
    args.update(kw)
    return ope.default_region_params(**args)


def _run(ctx, ope, scene, max_clusters=None, **kw):
    return ctx.region_grow(scene.pts, _params(ope, scene, **kw), scene.normals, scene.curvature, max_clusters=max_clusters)


def _same(got, want):
    assert [len(c) for c in got] == [len(c) for c in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _check(ctx, got, scene, want, cap=None):
    clusters, labels, stats = got
    kept = want if cap is None else want[:cap]
    print(scene.name, "regions", len(want), "sizes", [len(c) for c in want[:6]], "stats", stats)
    assert ctx.last_cluster_count == len(want)
    _same(clusters, kept)
    np.testing.assert_array_equal(labels, R.labels_of(kept, len(scene.pts)))
    assert stats["refused_curvature"] == 0


# ---------------------------------------------------------------------------------------------------- 1. one-way edge
@pytest.mark.parametrize("first", [False, True])
def test_one_way_edge(ctx, ope, first):
    scene = R.one_way(first)
    want = scene.reference(1)[0]
    assert [c.tolist() for c in want] == ([[0, 1, 2, 3]] if first else [[1, 2, 3], [0]])
    got = _run(ctx, ope, scene)
    _check(ctx, got, scene, want)
    assert got[2]["one_way_edges"] == 2 and got[2]["regions_before_size_filter"] == len(want)


# ---------------------------------------------------------------------------------------------------- 2. long chain
@pytest.mark.parametrize("with_links", [True, False])
def test_long_chain(ctx, ope, with_links):
    scene = R.chain(with_links)
    want = scene.reference(1)[0]
    assert len(want) == (1 if with_links else R.CHAIN_N - 1)
    got = _run(ctx, ope, scene)
    _check(ctx, got, scene, want)
    assert got[2]["one_way_edges"] == R.CHAIN_N - 2 and got[2]["sweeps"] >= 1


# ---------------------------------------------------------------------------------------------------- 3. crease
def test_crease_parts_at_10_degrees_and_joins_at_40(ctx, ope):
    scene = R.crease()
    want = scene.reference(1)[0]
    assert sorted(len(c) for c in want)[-2:] == [1560, 1640]
    _check(ctx, _run(ctx, ope, scene), scene, want)
    wide = scene.reference(1, theta=40 * R.DEG)[0]
    assert len(wide) == 1
    _check(ctx, _run(ctx, ope, scene, smoothness_threshold=40 * R.DEG), scene, wide)


# ---------------------------------------------------------------------------------------------------- 4. size filter and order
@pytest.mark.parametrize("mn,mx", [(1, 1000000), (50, 1000000), (500, 1000000), (50, 2500)])
def test_size_filter_keeps_the_seed_order(ctx, ope, mn, mx):
    scene = R.scene4()
    want = scene.reference(mn, mx)[0]
    if (mn, mx) == (50, 1000000):
        assert [len(c) for c in want] == [2282, 3000, 50]          # by seed, not by size
    got = _run(ctx, ope, scene, min_size=mn, max_size=mx)
    _check(ctx, got, scene, want)
    assert got[2]["regions_before_size_filter"] == scene.reference(1)[2]


def test_max_clusters_below_the_count_and_null_outputs(ctx, ope):
    scene = R.scene4()
    want = scene.reference(1)[0]
    assert len(want) > 3
    _check(ctx, _run(ctx, ope, scene, max_clusters=3), scene, want, cap=3)
    # the raw entry point: no label array; then nothing written at all (max_clusters 0: every output NULL)
    cloud = ctx.upload(scene.pts)
    p = _params(ope, scene)
    n = len(scene.pts)
    idx, off, k = np.empty(n, np.int32), np.zeros(3, np.int32), C.c_size_t(0)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    nrm, cur = scene.normals.ctypes.data_as(fp), scene.curvature.ctypes.data_as(fp)
    rc = ope.lib().ope_region_grow(ctx.h, cloud.h, C.byref(p), nrm, cur, 2, C.byref(k), idx.ctypes.data_as(ip), off.ctypes.data_as(ip), None)
    assert rc == ope.OPE_OK and k.value == len(want)
    np.testing.assert_array_equal(off, R.offsets_of(want[:2]))
    _same([idx[off[i]:off[i + 1]] for i in range(2)], want[:2])
    k = C.c_size_t(0)
    rc = ope.lib().ope_region_grow(ctx.h, cloud.h, C.byref(p), nrm, cur, 0, C.byref(k), None, None, None)
    assert rc == ope.OPE_OK and k.value == len(want)


# ---------------------------------------------------------------------------------------------------- 5. self-estimated normals
def test_self_estimated_normals(ctx, ope):
    scene = R.scene4()
    want = scene.reference(50)[0]
    cloud = ctx.upload(scene.pts)
    got = ctx.region_grow(cloud, _params(ope, scene, min_size=50, normals_k=30))
    _check(ctx, got, scene, want)
    nrm, cur = cloud.download_normals()
    fresh = ctx.upload(scene.pts)
    ctx.normals(fresh, 30)
    nrm2, cur2 = fresh.download_normals()
    assert nrm.tobytes() == nrm2.tobytes() and cur.tobytes() == cur2.tobytes()
    # passed normals leave the cloud's own alone
    other = ctx.upload(scene.pts)
    ctx.region_grow(other, _params(ope, scene), scene.normals, scene.curvature)
    with pytest.raises(ope.OpeError):
        other.download_normals()


# ---------------------------------------------------------------------------------------------------- 6. edges of the input
def test_non_finite_points_are_in_no_region(ctx, ope):
    base = R.scene4()
    rng = np.random.default_rng(3)
    pts = base.pts.copy()
    bad = rng.choice(len(pts), 150, replace=False)
    pts[bad[:50], 0] = np.nan
    pts[bad[50:100], 1] = np.inf
    pts[bad[100:], 2] = -np.inf
    nrm, cur = base.normals.copy(), base.curvature.copy()
    nrm[bad], cur[bad] = np.nan, np.nan
    scene = R.Scene("scene4_holes", pts, nrm, cur, 15)
    want = scene.reference(1)[0]
    got = _run(ctx, ope, scene)
    _check(ctx, got, scene, want)
    assert (got[1][bad] == -1).all()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_clouds(ctx, ope, n):
    pts = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.31]], np.float32)[:n]
    scene = R.Scene("tiny", pts, R._flat_normals(n), np.array([0.02, 0.01], np.float32)[:n], 15)      # more neighbours than points
    got = _run(ctx, ope, scene)
    want = scene.reference(1)[0]
    assert [c.tolist() for c in want] == [[], [[0]], [[0, 1]]][n]
    _check(ctx, got, scene, want)


def test_a_nan_normal_is_absorbed(ctx, ope):
    """validatePoint refuses `dot < c`; a NaN product is not less, so a point with a NaN normal joins and carries the region on.
    (The spacing grows: every point lists its predecessor, and the ranks descend along the line.)"""
    pts = np.zeros((6, 3), np.float32)
    pts[:, 0] = [0.0, 0.1, 0.21, 0.33, 0.46, 0.6]
    nrm = R._flat_normals(6)
    nrm[2] = np.nan
    nrm[4] = [1.0, 0.0, 0.0]                                   # perpendicular: refused from both sides
    cur = np.array([0.06, 0.05, 0.04, 0.03, 0.02, 0.01], np.float32)
    scene = R.Scene("nan_normal", pts, nrm, cur, 2)
    want = scene.reference(1)[0]
    assert [c.tolist() for c in want] == [[5], [4], [0, 1, 2, 3]]
    _check(ctx, _run(ctx, ope, scene), scene, want)


BAD = [dict(number_of_neighbours=0), dict(number_of_neighbours=33), dict(smoothness_threshold=float("nan")),
       dict(smoothness_threshold=float("inf")), dict(smoothness_threshold=-0.1), dict(curvature_threshold=float("nan")),
       dict(curvature_threshold=float("inf")), dict(min_size=0), dict(min_size=10, max_size=9)]


def _refused(ctx, ope, call):
    ctx.profile_kernels(True)
    with pytest.raises(ope.OpeError) as e:
        call()
    rec = ctx.profile_kernels_read()
    ctx.profile_kernels(False)
    assert e.value.code == ope.OPE_EINVAL
    assert rec == {} and ctx.region_stats()["launches"] == 0 and ctx.region_stats()["host_syncs"] == 0


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_launch_nothing(ctx, ope, kw):
    scene = R.crease()
    cloud = ctx.upload(scene.pts)
    _refused(ctx, ope, lambda: ctx.region_grow(cloud, _params(ope, scene, **kw), scene.normals, scene.curvature))


@pytest.mark.parametrize("normals_k", [2, 33])
def test_refusal_of_normals_k_only_when_it_is_needed(ctx, ope, normals_k):
    scene = R.crease()
    cloud = ctx.upload(scene.pts)
    _refused(ctx, ope, lambda: ctx.region_grow(cloud, _params(ope, scene, normals_k=normals_k)))
    _check(ctx, ctx.region_grow(cloud, _params(ope, scene, normals_k=normals_k), scene.normals, scene.curvature), scene, scene.reference(1)[0])


def test_refusal_of_one_array_without_the_other(ctx, ope):
    scene = R.crease()
    cloud = ctx.upload(scene.pts)
    _refused(ctx, ope, lambda: ctx.region_grow(cloud, _params(ope, scene), scene.normals, None))
    _refused(ctx, ope, lambda: ctx.region_grow(cloud, _params(ope, scene), None, scene.curvature))


def test_a_curvature_above_the_threshold_is_refused_with_outputs_untouched(ctx, ope):
    scene = R.crease()
    cloud = ctx.upload(scene.pts)
    n = len(scene.pts)
    p = _params(ope, scene, curvature_threshold=float(np.sort(scene.curvature)[-3]))      # two points lie above it
    idx, off, lab = np.full(n, -7, np.int32), np.full(n + 1, -7, np.int32), np.full(n, -7, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    k = C.c_size_t(99)
    rc = ope.lib().ope_region_grow(ctx.h, cloud.h, C.byref(p), scene.normals.ctypes.data_as(fp), scene.curvature.ctypes.data_as(fp), n, C.byref(k),
                                   idx.ctypes.data_as(ip), off.ctypes.data_as(ip), lab.ctypes.data_as(ip))
    assert rc == ope.OPE_EINVAL and k.value == 0
    assert (idx == -7).all() and (off == -7).all() and (lab == -7).all()
    assert ctx.region_stats()["refused_curvature"] == 2
    assert b"curvature" in ope.lib().ope_last_error(ctx.h)
    # the threshold is compared as PCL compares it, in float and strictly: at the largest curvature nothing is refused
    p = _params(ope, scene, curvature_threshold=float(scene.curvature.max()))
    _check(ctx, ctx.region_grow(cloud, p, scene.normals, scene.curvature), scene, scene.reference(1)[0])


def test_launches_do_not_depend_on_the_number_of_regions(ctx, ope):
    scene = R.scene4()
    cloud = ctx.upload(scene.pts)
    seen = []
    for mn in (1, 500):
        ctx.profile_kernels(True)
        clusters, _, stats = ctx.region_grow(cloud, _params(ope, scene, min_size=mn), scene.normals, scene.curvature)
        rec = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        seen.append((len(clusters), {name: r["launches"] for name, r in rec.items() if name != "rg_sweep_kernel"},
                     stats["launches"] - rec["rg_sweep_kernel"]["launches"] * 5 // 4, stats["host_syncs"] - rec["rg_sweep_kernel"]["launches"] // 4))
        assert rec["rg_sweep_kernel"]["launches"] % 4 == 0 and rec["rg_graph_kernel"]["launches"] == 1
    assert seen[0][0] > 100 and seen[1][0] == 2
    assert seen[0][1:] == seen[1][1:]


# ---------------------------------------------------------------------------------------------------- 7. the _cloud form
def test_cloud_form_equals_select(ctx, ope):
    scene = R.scene4()
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 1 << 24, len(scene.pts)).astype(np.uint32)
    want = scene.reference(50)[0]
    runs = []
    for _ in range(2):
        cloud = ctx.upload(scene.pts)
        cloud.set_rgb(rgb)
        clouds, indices, stats = ctx.region_grow(cloud, _params(ope, scene, min_size=50, normals_k=30), clouds=True)
        _same(indices, want)
        blob = b""
        for c, ind in zip(clouds, indices):
            sel = ctx.select(cloud, ind)
            assert c.n == len(ind) == sel.n
            pts, (nrm, cur), col = ctx.download(c), c.download_normals(), c.download_rgb()
            assert pts.tobytes() == ctx.download(sel).tobytes() == scene.pts[ind].tobytes()
            nrm_s, cur_s = sel.download_normals()
            assert nrm.tobytes() == nrm_s.tobytes() and cur.tobytes() == cur_s.tobytes()
            assert col.tobytes() == sel.download_rgb().tobytes() == rgb[ind].tobytes()
            blob += pts.tobytes() + nrm.tobytes() + cur.tobytes() + col.tobytes() + ind.tobytes()
        runs.append(blob)
    assert runs[0] == runs[1]
