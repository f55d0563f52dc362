"""Euclidean cluster extraction on the device (ope_euclidean_clusters) against the host reference (tests/cluster_ref.py:
cKDTree candidate pairs, the exact float predicate, scipy's connected components, PCL's filter and order)."""
import numpy as np
import pytest

from cluster_ref import labels_of, r2_of, reference_clusters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(synth):
    return synth.tabletop_objects()


def _run(ctx, pts, tol, mn, mx, max_clusters=None):
    cl, lab = ctx.euclidean_clusters(pts, tolerance=tol, min_size=mn, max_size=mx, want_labels=True, max_clusters=max_clusters)
    return cl, lab


def _same(got, want):
    assert [len(c) for c in got] == [len(c) for c in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_tabletop_equals_the_reference_exactly(ctx, table):
    pts, oid = table
    want = reference_clusters(pts, 0.05, 300, 100000)
    got, lab = _run(ctx, pts, 0.05, 300, 100000)
    _same(got, want)
    np.testing.assert_array_equal(lab, labels_of(want, len(pts)))
    # against the generating objects: the blobs (ids 6-10) are dropped, box and cylinder (1, 2) merge
    objs = [np.nonzero(oid == i)[0] for i in (0, 3, 4, 5)] + [np.nonzero((oid == 1) | (oid == 2))[0]]
    objs.sort(key=lambda c: (-len(c), c[0]))
    _same(got, objs)


def boundary_pairs(tol):
    """Three point pairs whose float d2 ((dx*dx + dy*dy) + dz*dz, from the float coordinates) is r2, the float below r2 and the
    float above r2."""
    r2 = r2_of(tol)
    a = np.array([0.3, 0.2, 0.1], np.float32)
    r = np.sqrt(np.float64(r2))
    bx = (a[0] + np.float32(r * 0.8)).astype(np.float32) + np.arange(-3000, 3000, dtype=np.float32) * np.spacing(np.float32(0.34))
    by = (a[1] + np.float32(r * 0.6)).astype(np.float32) + np.arange(-400, 400, dtype=np.float32) * np.spacing(np.float32(0.23))
    dx = (bx.astype(np.float32) - a[0]).astype(np.float32)
    dy = (by.astype(np.float32) - a[1]).astype(np.float32)
    d2 = (dx[:, None] * dx[:, None] + dy[None, :] * dy[None, :]).astype(np.float32)   # + dz*dz with dz = 0
    out = {}
    for key, target in (("eq", r2), ("below", np.nextafter(r2, np.float32(0))), ("above", np.nextafter(r2, np.float32(1)))):
        i, j = np.argwhere(d2 == target)[0]
        out[key] = np.stack([a, np.array([bx[i], by[j], a[2]], np.float32)])
    return out


def test_boundary_pairs_join_at_r2_and_one_ulp_below_but_not_above(ctx):
    from cluster_ref import flann_d2
    tol = 0.05
    pairs = boundary_pairs(tol)
    r2 = r2_of(tol)
    assert flann_d2(*pairs["eq"]) == r2 and flann_d2(*pairs["above"]) > r2 > flann_d2(*pairs["below"])
    for key, joined in (("eq", True), ("below", True), ("above", False)):
        got, _ = _run(ctx, pairs[key], tol, 1, 10)
        assert [c.tolist() for c in got] == ([[0, 1]] if joined else [[0], [1]]), key
        # the same pair moved along a chain of copies: every link sits on the boundary, across cell borders
        step = pairs[key][1] - pairs[key][0]
        chain = (pairs[key][0] + np.arange(40, dtype=np.float32)[:, None] * step).astype(np.float32)
        _same(_run(ctx, chain, tol, 1, 100)[0], reference_clusters(chain, tol, 1, 100))


def test_size_limits_keep_whole_components(ctx):
    rng = np.random.default_rng(5)
    sizes = [299, 300, 400, 401]
    pts = np.concatenate([rng.normal(0, 0.004, (s, 3)) + np.array([k * 1.0, 0, 0]) for k, s in enumerate(sizes)]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    got, _ = _run(ctx, pts, 0.05, 300, 400)
    assert sorted(len(c) for c in got) == [300, 400]
    _same(got, reference_clusters(pts, 0.05, 300, 400))


@pytest.mark.parametrize("mn", [1, 300])
def test_non_finite_points_are_singletons(ctx, table, mn):
    pts = table[0].copy()
    rng = np.random.default_rng(9)
    bad = rng.choice(len(pts), 200, replace=False)
    pts[bad[:80], 0] = np.nan
    pts[bad[80:140], 1] = np.inf
    pts[bad[140:], 2] = -np.inf
    got, lab = _run(ctx, pts, 0.05, mn, 100000)
    want = reference_clusters(pts, 0.05, mn, 100000)
    _same(got, want)
    np.testing.assert_array_equal(lab, labels_of(want, len(pts)))


def test_degenerate_inputs(ctx, ope):
    assert ctx.euclidean_clusters(np.zeros((0, 3), np.float32), min_size=1) == []
    one = ctx.euclidean_clusters(np.array([[1, 2, 3]], np.float32), min_size=1)
    assert [c.tolist() for c in one] == [[0]]
    rng = np.random.default_rng(3)
    cell = (rng.uniform(0, 0.01, (500, 3)) + 7.0).astype(np.float32)   # every point in one cell
    got = ctx.euclidean_clusters(cell, tolerance=0.05, min_size=1)
    assert [c.tolist() for c in got] == [list(range(500))]
    assert ctx.cluster_stats()["cells"] == 1


def test_extent_beyond_2_to_the_32_cells(ctx):
    rng = np.random.default_rng(4)
    a = rng.normal(0, 0.0004, (400, 3))
    b = rng.normal(0, 0.0004, (500, 3)) + np.array([100.0, 30.0, -20.0])
    pts = np.concatenate([a, b]).astype(np.float32)
    got = ctx.euclidean_clusters(pts, tolerance=0.001, min_size=10)
    want = reference_clusters(pts, 0.001, 10, 100000)
    _same(got, want)
    assert len(want) >= 2


def test_many_equal_size_clusters_tie_order(ctx):
    rng = np.random.default_rng(6)
    k = 2100
    grid = np.stack(np.meshgrid(np.arange(15), np.arange(15), np.arange(10), indexing="ij"), -1).reshape(-1, 3)[:k] * 0.2
    pts = (grid[:, None, :] + rng.uniform(0, 0.01, (k, 4, 3))).reshape(-1, 3).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    got = ctx.euclidean_clusters(pts, tolerance=0.05, min_size=1)
    assert len(got) == k
    _same(got, reference_clusters(pts, 0.05, 1, 100000))
    firsts = [int(c[0]) for c in got]
    assert firsts == sorted(firsts)


def test_long_chains_flatten_to_their_roots(ctx):
    # helices of points 0.6 tolerances apart across thousands of cells: deep union-find trees when the flatten pass starts
    t = np.arange(30000, dtype=np.float64) * 0.006
    chains = [np.stack([0.4 * np.cos(t + k), 0.4 * np.sin(t + k), 0.0005 * t + 1.5 * k], 1) for k in range(4)]
    pts = np.concatenate(chains).astype(np.float32)
    pts = pts[np.random.default_rng(12).permutation(len(pts))]
    want = reference_clusters(pts, 0.01, 1, 1000000)
    runs = []
    for _ in range(3):
        got, lab = _run(ctx, pts, 0.01, 1, 1000000)
        _same(got, want)
        runs.append(lab.tobytes())
    assert runs[0] == runs[1] == runs[2]


def test_dense_clumps_just_over_the_tolerance_apart(ctx):
    # the worst case of the cell-pair comparison: dense neighbouring cells with no joining pair
    rng = np.random.default_rng(13)
    tol = 0.05
    centres = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.2 * tol
    pts = (centres[:, None, :] + rng.uniform(-0.04 * tol, 0.04 * tol, (len(centres), 600, 3))).reshape(-1, 3).astype(np.float32)
    got = ctx.euclidean_clusters(pts, tolerance=tol, min_size=300)
    want = reference_clusters(pts, tol, 300, 100000)
    assert len(want) == 27
    _same(got, want)


def test_truncation_reports_the_full_count(ctx, table):
    pts = table[0]
    want = reference_clusters(pts, 0.05, 1, 100000)
    got, lab = _run(ctx, pts, 0.05, 1, 100000, max_clusters=3)
    assert ctx.last_cluster_count == len(want)
    _same(got, want[:3])
    np.testing.assert_array_equal(lab, labels_of(want[:3], len(pts)))


def test_shuffled_input_gives_the_same_index_sets(ctx, table):
    pts = table[0]
    perm = np.random.default_rng(8).permutation(len(pts))
    a = ctx.euclidean_clusters(pts, min_size=1)
    b = ctx.euclidean_clusters(pts[perm], min_size=1)
    assert sorted(c.tolist() for c in a) == sorted(np.sort(perm[c]).tolist() for c in b)


def test_repeated_calls_are_byte_identical(ctx, table):
    cloud = ctx.upload(table[0])
    runs = []
    for _ in range(3):
        cl, lab = ctx.euclidean_clusters(cloud, want_labels=True)
        runs.append(b"".join(c.tobytes() for c in cl) + lab.tobytes())
    assert runs[0] == runs[1] == runs[2]


def test_launches_do_not_depend_on_the_number_of_clusters(ctx):
    rng = np.random.default_rng(2)
    recs, stats = [], []
    for k in (1, 8, 200):
        n = 4000
        centres = np.arange(k)[:, None] * np.array([[0.5, 0, 0]])
        pts = (centres[rng.integers(0, k, n)] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
        cloud = ctx.upload(pts)
        ctx.profile_kernels(True)
        got = ctx.euclidean_clusters(cloud, min_size=1)
        rec = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        assert len(got) == k
        recs.append({name: r["launches"] for name, r in rec.items() if name.startswith("cc_")})
        s = ctx.cluster_stats()
        stats.append((s["launches"], s["host_syncs"]))
    assert recs[0] == recs[1] == recs[2]
    assert stats[0] == stats[1] == stats[2]
    assert stats[0][1] == 1


@pytest.mark.parametrize("kw", [dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(min_size=0),
                                dict(min_size=10, max_size=9)])
def test_refusals_launch_nothing(ctx, ope, table, kw):
    cloud = ctx.upload(table[0][:1000])
    args = dict(tolerance=0.05, min_size=300, max_size=100000)
    args.update(kw)
    ctx.profile_kernels(True)
    with pytest.raises(ope.OpeError) as e:
        ctx.euclidean_clusters(cloud, **args)
    rec = ctx.profile_kernels_read()
    ctx.profile_kernels(False)
    assert e.value.code == ope.OPE_EINVAL
    assert not any(name.startswith("cc_") for name in rec)
    assert ctx.cluster_stats()["launches"] == 0


def test_c3_frame(ctx, synth):
    scene, _ = synth.config_clouds("C3")
    cloud = ctx.upload(scene)
    assert ctx.euclidean_clusters(cloud) == []          # tol 0.05: one component above max_size
    want = reference_clusters(scene, 0.001, 300, 100000)
    got, lab = _run(ctx, cloud, 0.001, 300, 100000)
    _same(got, want)
    np.testing.assert_array_equal(lab, labels_of(want, len(scene)))
