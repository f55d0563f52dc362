"""ope_region_grow_rgb against the sequential restatement of pcl::RegionGrowingRGB (region_grow_rgb_ref.py), with lists from
oracle.KdTree.  Clusters, offsets, labels, the count and the stats segments, segment_pairs, homogeneous_regions and
regions_absorbed are compared exactly.  Every scene is asserted free of boundary ties, and what it is there to exercise is asserted
from the reference alone before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import region_grow_rgb_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

STATS = ("segments", "segment_pairs", "homogeneous_regions", "regions_absorbed", "regions_before_size_filter", "one_way_edges")


@pytest.fixture(scope="module")
def ope():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


_SCENES = {}


def scene_of(name, make):
    if name not in _SCENES:
        _SCENES[name] = make()
        assert _SCENES[name].free_of_boundary_ties(), name
    return _SCENES[name]


def _params(ope, scene, **over):
    kw = dict(scene.params)
    kw.update(over)
    return ope.default_region_rgb_params(region_neighbour_number=scene.k, **kw)


def _upload(ctx, scene, rgb=None):
    cloud = ctx.upload(scene.pts)
    cloud.set_rgb(scene.rgb if rgb is None else rgb)
    return cloud


def _check(ctx, got, scene, want, info):
    clusters, labels, stats = got
    print("[region_grow_rgb] %s: n %d k %d -> %s; device %s" % (scene.name, len(scene.pts), scene.k, {k: info[k] for k in STATS}, stats))
    assert ctx.last_cluster_count == len(want)
    assert len(clusters) == len(want)
    for a, b in zip(clusters, want):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert np.array_equal(labels, R.labels_of(want, len(scene.pts)))
    for k in STATS:
        assert stats[k] == info[k], k


def _run(ctx, ope, scene, **over):
    want, info = scene.reference(**over)
    _check(ctx, ctx.region_grow_rgb(_upload(ctx, scene), _params(ope, scene, **over)), scene, want, info)
    return want, info


# ---------------------------------------------------------------------------------------------------- the scenes, one per step
def test_two_colours(ctx, ope):
    scene = scene_of("two_colours", R.two_colours)
    want, info = scene.reference()
    assert info["segments"] == 2 and [len(c) for c in want] == [1000, 1000]
    _run(ctx, ope, scene)


def test_chain_is_one_segment(ctx, ope):
    scene = scene_of("chain", R.chain)
    want, info = scene.reference()
    ch = R.channels(scene.rgb)
    assert info["segments"] == 1 and len(want) == 1 and R.color_dist(ch[0], ch[59]) > 100       # the end stripes are far apart in colour
    _run(ctx, ope, scene)


def test_steps_of_12_are_absorbed_in_sequence(ctx, ope):
    scene = scene_of("steps_of_12", R.steps_of_12)
    want, info = scene.reference()
    assert info["segments"] == 6 and info["homogeneous_regions"] == 6 and info["regions_absorbed"] >= 2 and info["swaps"] >= 1
    assert all(np.count_nonzero(info["seg"] == s) < 700 for s in range(6))
    _run(ctx, ope, scene)


def test_merge_a_joins_similar_segments_within_the_distance_threshold(ctx, ope):
    scene = scene_of("merge_a", R.merge_a)
    want, info = scene.reference()
    assert info["segments"] == 2 and info["homogeneous_regions"] == 1 and len(want) == 1 and info["regions_absorbed"] == 0
    _run(ctx, ope, scene)


def test_distance_threshold_below_the_gap_keeps_them_apart(ctx, ope):
    scene = scene_of("distance_threshold", lambda: R.merge_a(0.01))
    want, info = scene.reference()
    assert info["segments"] == 2 and info["homogeneous_regions"] == 2 and [len(c) for c in want] == [900, 900]
    _run(ctx, ope, scene)


def test_salt_is_absorbed(ctx, ope):
    scene = scene_of("salt", R.salt)
    want, info = scene.reference()
    assert info["segments"] == 5 and info["regions_absorbed"] == 4 and [len(c) for c in want] == [2000]
    assert sorted(np.count_nonzero(info["seg"] == s) for s in range(5)) == [1, 1, 1, 1, 1996]
    _run(ctx, ope, scene)


def test_truncation_to_the_k_nearest_segments_with_equal_distances(ctx, ope):
    scene = scene_of("truncation", R.truncation)
    want, info = scene.reference()
    assert scene.k == 8 and info["truncated"] >= 1
    first = info["kept"][0]                       # the left stripe: A and B at the same distance, ordered by segment
    assert len(first) == 8 and first[0][0] == first[1][0] == 2.0 ** -20 and first[0][1] + 1 == first[1][1] == info["segments"] - 1
    _run(ctx, ope, scene)


def test_one_way_edges(ctx, ope):
    scene = scene_of("one_way_edges", R.one_way_edges)
    want, info = scene.reference()
    lone = len(scene.pts) - 1
    assert info["one_way_edges"] > 0 and not (scene.nbrs[:lone] == lone).any() and (scene.nbrs[lone] >= 0).all()
    _run(ctx, ope, scene)


# ---------------------------------------------------------------------------------------------------- the search at other K
@pytest.mark.parametrize("k", [1, 33, 100, 128])
def test_search_rows_at_every_list_length(ctx, ope, k):
    """Every later step reads the rows as sets with their distances: segment_pairs and the kept lists (through the merges) come out
    as the reference's only if every row holds the oracle's k nearest with bit-equal d2.  3 000 points, 5 of them non-finite."""
    scene = scene_of("search_k%d" % k, lambda: R.search_cloud(k))
    want, info = scene.reference()
    assert np.count_nonzero(~np.isfinite(scene.pts).all(1)) == 5
    if k == 1:
        assert info["segments"] == 2995 and info["segment_pairs"] == 0 and want == []
    else:
        # (the salt points link up where they come into each other's lists: fewer segments at a larger K)
        assert info["segments"] > 10 and info["segment_pairs"] > info["segments"] and info["regions_absorbed"] > 5 and len(want) == 4
    _run(ctx, ope, scene)
    labels = ctx.region_grow_rgb(_upload(ctx, scene), _params(ope, scene))[1]
    assert (labels[[7, 500, 1501, 2222, 2999]] == -1).all()         # non-finite points are in no region


@pytest.mark.parametrize("n", [0, 1, 2, 60])
def test_fewer_finite_points_than_k(ctx, ope, n):
    if n == 0:
        cloud = ctx.upload(np.zeros((0, 3), np.float32))
        cloud.set_rgb(np.zeros(0, np.uint32))
        clusters, labels, stats = ctx.region_grow_rgb(cloud)
        assert clusters == [] and labels.shape == (0,) and stats["launches"] == 0
        return
    scene = scene_of("small_%d" % n, lambda: R.small_cloud(n))
    want, info = scene.reference()
    assert scene.k == 100 and (scene.nbrs[:, n:] == -1).all() and len(want) == min(n, 2)
    _run(ctx, ope, scene)


def test_all_points_non_finite(ctx, ope):
    pts = np.full((5, 3), np.nan, np.float32)
    cloud = ctx.upload(pts)
    cloud.set_rgb(np.arange(5, dtype=np.uint32))
    clusters, labels, stats = ctx.region_grow_rgb(cloud, ope.default_region_rgb_params(min_size=1))
    assert clusters == [] and (labels == -1).all() and stats["segments"] == 0


def test_the_alpha_byte_is_ignored(ctx, ope):
    scene = scene_of("steps_of_12", R.steps_of_12)
    want, info = scene.reference()
    alpha = (np.arange(len(scene.rgb), dtype=np.uint32) * np.uint32(0x01010101)) & np.uint32(0xFF000000)
    _check(ctx, ctx.region_grow_rgb(_upload(ctx, scene, scene.rgb | alpha), _params(ope, scene)), scene, want, info)


@pytest.mark.parametrize("mn, mx", [(1, R.INT_MAX), (700, R.INT_MAX), (50, 2500)])
def test_size_filter(ctx, ope, mn, mx):
    scene = scene_of("search_k33", lambda: R.search_cloud(33))
    want, info = _run(ctx, ope, scene, min_size=mn, max_size=mx)
    if mn == 1:
        assert len(want) == info["segments"] and info["regions_absorbed"] == 0       # nothing is small: the merge moves nothing
    assert all(mn <= len(c) <= mx for c in want)


def test_max_clusters_below_the_count_and_null_outputs(ctx, ope):
    scene = scene_of("search_k33", lambda: R.search_cloud(33))
    want, info = scene.reference()
    n = len(scene.pts)
    assert len(want) == 4
    cloud = _upload(ctx, scene)
    clusters, labels, _ = ctx.region_grow_rgb(cloud, _params(ope, scene), max_clusters=2)
    assert ctx.last_cluster_count == 4 and len(clusters) == 2
    assert all(np.array_equal(a, b) for a, b in zip(clusters, want)) and np.array_equal(labels, R.labels_of(want, n, cap=2))
    # the raw call: offsets and the count; then with every optional output NULL
    ip = C.POINTER(C.c_int32)
    p = _params(ope, scene)
    idx, off, lab = np.full(n, -7, np.int32), np.full(n + 1, -7, np.int32), np.full(n, -7, np.int32)
    k = C.c_size_t(99)
    rc = ope.lib().ope_region_grow_rgb(ctx.h, cloud.h, C.byref(p), n, C.byref(k), idx.ctypes.data_as(ip), off.ctypes.data_as(ip), lab.ctypes.data_as(ip))
    assert rc == 0 and k.value == 4 and np.array_equal(off[:5], R.offsets_of(want)) and (off[5:] == -7).all()
    assert np.array_equal(idx[:off[4]], np.concatenate(want))
    k = C.c_size_t(99)
    assert ope.lib().ope_region_grow_rgb(ctx.h, cloud.h, C.byref(p), 0, C.byref(k), None, None, None) == 0 and k.value == 4
    k = C.c_size_t(99)
    assert ope.lib().ope_region_grow_rgb(ctx.h, cloud.h, C.byref(p), n, C.byref(k), idx.ctypes.data_as(ip), off.ctypes.data_as(ip), None) == 0 and k.value == 4
    assert ope.lib().ope_region_grow_rgb(ctx.h, cloud.h, C.byref(p), n, C.byref(k), None, off.ctypes.data_as(ip), None) == ope.OPE_EINVAL


# ---------------------------------------------------------------------------------------------------- refusals and the budget
BAD = [dict(region_neighbour_number=0), dict(region_neighbour_number=129), dict(distance_threshold=-0.1), dict(distance_threshold=float("nan")),
       dict(point_color_threshold=float("inf")), dict(point_color_threshold=-1.0), dict(region_color_threshold=float("nan")),
       dict(region_color_threshold=-2.0), dict(min_size=0), dict(min_size=10, max_size=9)]


def _refused(ctx, ope, call):
    ctx.profile_kernels(True)
    with pytest.raises(ope.OpeError) as e:
        call()
    rec = ctx.profile_kernels_read()
    ctx.profile_kernels(False)
    assert e.value.code == ope.OPE_EINVAL
    assert rec == {} and ctx.region_rgb_stats()["launches"] == 0 and ctx.region_rgb_stats()["host_syncs"] == 0


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_launch_nothing(ctx, ope, kw):
    scene = scene_of("small_60", lambda: R.small_cloud(60))
    cloud = _upload(ctx, scene)
    _refused(ctx, ope, lambda: ctx.region_grow_rgb(cloud, ope.default_region_rgb_params(**kw)))
    _refused(ctx, ope, lambda: ctx.region_grow_rgb(cloud, ope.default_region_rgb_params(**kw), clouds=True))


def test_a_cloud_without_colours_is_refused(ctx, ope):
    scene = scene_of("small_60", lambda: R.small_cloud(60))
    plain = ctx.upload(scene.pts)
    _refused(ctx, ope, lambda: ctx.region_grow_rgb(plain))
    _refused(ctx, ope, lambda: ctx.region_grow_rgb(plain, clouds=True))


def test_launches_do_not_depend_on_the_number_of_segments(ctx, ope):
    """two regions from two segments, and 2 995 segments: the same kernels, launches and synchronisations once the batches of
    sweeps are taken out"""
    seen = []
    for scene in (scene_of("two_colours", R.two_colours), scene_of("search_k1", lambda: R.search_cloud(1)), scene_of("search_k33", lambda: R.search_cloud(33))):
        cloud = _upload(ctx, scene)
        ctx.profile_kernels(True)
        clusters, _, stats = ctx.region_grow_rgb(cloud, _params(ope, scene))
        rec = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        batches = rec["rg_sweep_kernel"]["launches"] // 4
        assert rec["rg_sweep_kernel"]["launches"] % 4 == 0 and rec["rgb_search_kernel"]["launches"] == 1 and batches >= 1
        seen.append((stats["segments"], {name: r["launches"] for name, r in rec.items() if name != "rg_sweep_kernel"}, stats["launches"] - 5 * batches,
                     stats["host_syncs"] - batches))
    assert seen[0][0] == 2 and seen[1][0] > 100 and seen[2][0] > 30
    assert seen[0][1:] == seen[1][1:] == seen[2][1:]
    assert seen[0][2:] == (27, 4)                      # the counts the header states


# ---------------------------------------------------------------------------------------------------- the _cloud form
def test_cloud_form_equals_select(ctx, ope):
    scene = scene_of("search_k33", lambda: R.search_cloud(33))
    want, info = scene.reference()
    cloud = _upload(ctx, scene)
    nrm = np.random.default_rng(3).standard_normal((len(scene.pts), 3)).astype(np.float32)
    cloud.set_normals(nrm)
    clouds, indices, stats = ctx.region_grow_rgb(cloud, _params(ope, scene), clouds=True)
    assert len(indices) == len(want) == 4 and all(np.array_equal(a, b) for a, b in zip(indices, want))
    for c, ind in zip(clouds, indices):
        sel = ctx.select(cloud, ind)
        assert c.n == len(ind) == sel.n and c.has_rgb
        assert ctx.download(c).tobytes() == ctx.download(sel).tobytes() == scene.pts[ind].tobytes()
        assert c.download_rgb().tobytes() == sel.download_rgb().tobytes() == scene.rgb[ind].tobytes()
        assert c.download_normals()[0].tobytes() == sel.download_normals()[0].tobytes() == nrm[ind].tobytes()
    assert stats["launches"] - 5 * ((stats["sweeps"] + 3) // 4) == 27 + 5 and stats["host_syncs"] - (stats["sweeps"] + 3) // 4 == 4 + 1
