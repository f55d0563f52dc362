"""ope_vfh_batch / ope_vfh_match / ope_vfh_recognise on the device against tests/vfh_ref.py, the literal restatement of
pcl::VFHEstimation::computeFeature and flann::ChiSquareDistance: signatures byte for byte, counts, per-point bins, neighbour
indices and distances.  Every comparison is exact."""
import numpy as np
import pytest

import oracle
import vfh_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL = -1


@pytest.fixture(scope="module")
def ope():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


_clouds, _refs = {}, {}


def cloud(n):
    """The n-point test cluster (a sphere patch with its normals) and its reference, computed once."""
    if n not in _clouds:
        _clouds[n] = R.sphere_patch(n, 1000 + n)
        _refs[n] = R.vfh(*_clouds[n])
    return _clouds[n], _refs[n]


def check(sig, counts, bins, ref, what=""):
    bad = np.flatnonzero((bins != ref["bins"]).any(1))
    assert len(bad) == 0, f"{what}: point {bad[0]} bins {bins[bad[0]]} reference {ref['bins'][bad[0]]}"
    assert (counts == ref["counts"]).all(), what
    assert sig.tobytes() == ref["sig"].tobytes(), what


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_cluster_sizes(ctx, n):
    (xyz, nrm), ref = cloud(n)
    sig, counts, bins = ctx.vfh([ctx.upload(xyz, nrm)], want_counts=True, want_bins=True)
    check(sig[0], counts[0], bins, ref, f"n = {n}")
    st = ctx.vfh_stats()
    assert (st["points"], st["rejected_pairs"], st["normals_estimated"], st["empty_clouds"], st["host_syncs"]) == (n, ref["rejected"], 0, 0, 1)
    if n == 1:
        assert ref["rejected"] == 1 and sig[0].sum() == 100.0   # its only pair is with itself; the viewpoint block holds it


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_batching(ctx, order):
    sizes = [1, 2, 63, 64, 65, 1000, 5000]
    if order == "reversed":
        sizes = sizes[::-1]
    clouds = [ctx.upload(*cloud(n)[0]) for n in sizes]
    sig, counts, bins = ctx.vfh(clouds, want_counts=True, want_bins=True)
    assert ctx.vfh_stats()["points"] == sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for i, n in enumerate(sizes):
        check(sig[i], counts[i], bins[off[i]:off[i + 1]], cloud(n)[1], f"{order} cluster {i} (n = {n})")
        single = ctx.vfh([clouds[i]])
        assert single[0].tobytes() == sig[i].tobytes()


def test_empty_cluster_gives_a_zero_row(ctx):
    (xyz, nrm), ref = cloud(64)
    sig, counts, _ = ctx.vfh([ctx.upload(np.zeros((0, 3), F)), ctx.upload(xyz, nrm), ctx.upload(np.zeros((0, 3), F))], want_counts=True)
    assert not sig[0].any() and not sig[2].any() and not counts[0].any() and not counts[2].any()
    assert sig[1].tobytes() == ref["sig"].tobytes()
    assert ctx.vfh_stats()["empty_clouds"] == 2


def test_flat_cluster(ctx):
    """All 5 000 normals equal: one viewpoint bin takes all 5 000 additions, the longest replay of the suite."""
    rng = np.random.default_rng(5)
    xyz = np.column_stack([rng.uniform(-0.1, 0.1, 5000), rng.uniform(-0.1, 0.1, 5000), np.full(5000, 0.75)]).astype(F)
    nrm = np.tile(np.array([0, 0, -1], F), (5000, 1))
    ref = R.vfh(xyz, nrm)
    assert ref["counts"][180:].max() == 5000
    sig, counts, bins = ctx.vfh([ctx.upload(xyz, nrm)], want_counts=True, want_bins=True)
    check(sig[0], counts[0], bins, ref, "flat")
    assert sig[0][180:].max() != F(5000) * F(100.0 / 5000)   # the replayed sum is not the product


def test_rejected_pair(ctx):
    """Three collinear points, the middle one on the (exact) centroid."""
    xyz = np.array([[-1, 0, 2], [0, 0, 2], [1, 0, 2]], F)
    nrm = np.tile(np.array([0, 0, -1], F), (3, 1))
    ref = R.vfh(xyz, nrm)
    assert (ref["centroid"] == [0, 0, 2]).all() and ref["rejected"] == 1
    sig, counts, bins = ctx.vfh([ctx.upload(xyz, nrm)], want_counts=True, want_bins=True)
    check(sig[0], counts[0], bins, ref, "collinear")
    assert list(bins[1, :3]) == [255, 255, 255] and (bins[[0, 2], :3] != 255).all()
    for blk in range(3):
        assert counts[0][45 * blk:45 * blk + 45].sum() == 2
    assert counts[0][180:].sum() == 3 and ctx.vfh_stats()["rejected_pairs"] == 1


def test_clamping(ctx, ope):
    """Given centroid (0, 0, 0) and normal (0, 0, 1).  A point exactly at (0, 0, 1) is parallel to the normal, its cross product
    is zero and computePairFeatures rejects it; one at (1e-5, 0, 1) still has |d| == 1.0f, so f3 == 1.0 and floor(45 * 1.0) = 45 is
    clamped to bin 44.  Its neighbour's normal is opposite to v: f2 == -1, bin 0.  The viewpoint is moved off the given centroid
    (PCL normalises a zero vector otherwise)."""
    xyz = np.array([[1e-5, 0, 1], [-1e-5, 0, 1], [0, 0, 1]], F)
    nrm = np.array([[1, 0, 0], [0, -1, 0], [1, 0, 0]], F)
    kw = dict(viewpoint=(0, 0, -1), given_centroid=(0, 0, 0), given_normal=(0, 0, 1))
    ref = R.vfh(xyz, nrm, **kw)
    ok, f = oracle.pair_features(np.zeros(3, F), np.array([0, 0, 1], F), xyz[0], nrm[0])
    assert ok and f[2] == 1.0
    ok, f = oracle.pair_features(np.zeros(3, F), np.array([0, 0, 1], F), xyz[1], nrm[1])
    assert ok and f[1] == -1.0
    assert ref["clamped"][0, 2] and ref["bins"][0, 2] == 44      # the reference took the clamp branch
    assert ref["bins"][1, 1] == 0 and list(ref["bins"][2, :3]) == [255] * 3
    p = ope.default_vfh_params(viewpoint=(0, 0, -1), use_given_centroid=1, centroid=(0, 0, 0), use_given_normal=1, normal=(0, 0, 1))
    sig, counts, bins = ctx.vfh([ctx.upload(xyz, nrm)], params=p, want_counts=True, want_bins=True)
    check(sig[0], counts[0], bins, ref, "clamp")


def test_normals_estimated_in_the_call(ctx):
    xyz, _ = R.sphere_patch(2000, 77)
    nrm, _ = oracle.normals_knn(xyz, k=30)
    ref = R.vfh(xyz, nrm)
    c = ctx.upload(xyz)
    sig, counts, bins = ctx.vfh([c], want_counts=True, want_bins=True)
    check(sig[0], counts[0], bins, ref, "estimated normals")
    st = ctx.vfh_stats()
    assert st["normals_estimated"] == 1
    left, _ = c.download_normals()
    assert left.tobytes() == nrm.tobytes()
    ctx.vfh([c])
    assert ctx.vfh_stats()["normals_estimated"] == 0   # they stayed on the cloud


def _table(m, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(0, 20, (m, 308)).astype(F)
    rows[rng.uniform(size=rows.shape) < 0.33] = 0
    if m >= 15:
        rows[11] = rows[3]          # two duplicated rows: the tie goes to the lower index
        rows[m - 1] = rows[5]
    q = rng.uniform(0, 20, (3, 308)).astype(F)
    q[rng.uniform(size=q.shape) < 0.33] = 0
    q[1] = rows[m // 2]             # a query equal to a row
    if m >= 15:
        q[2] = rows[3]
    return rows, q


@pytest.mark.parametrize("m", [1, 15, 16, 300, 1025])
def test_chi_square_search(ctx, m):
    rows, q = _table(m, 40 + m)
    db = ctx.vfh_db(rows)
    assert db.m == m
    for k in (15, 16):
        want_i, want_d = R.knn(rows, q, k)
        idx, dist = ctx.vfh_match(db, q, k)
        assert (idx == want_i).all(), (m, k)
        assert dist.tobytes() == want_d.tobytes(), (m, k)
        if m < k:
            assert (idx[:, m:] == -1).all() and np.isposinf(dist[:, m:]).all()
        assert dist[1, 0] == 0
    if m >= 15:
        assert list(want_i[2, :2]) == [3, 11]
    db.free()


def test_recognition(ctx):
    s = R.recognition_set()
    db = ctx.vfh_db(s["rows"])
    want_i, want_d = R.knn(s["rows"], s["query_sigs"], 15)
    idx, dist, sig = ctx.vfh_recognise(db, [ctx.upload(x, n) for x, n in s["queries"]], k=15, want_signatures=True)
    assert sig.tobytes() == s["query_sigs"].tobytes()
    assert (idx == want_i).all() and dist.tobytes() == want_d.tobytes()
    assert [R.object_name(s["names"], idx[i], dist[i]) for i in range(3)] == s["expected"]
    # the training rows themselves come out of the device too
    v0 = R.shape_view("box", 0.0, 0.45, R.RECOGNITION_SEED)
    assert ctx.vfh([ctx.upload(*v0)])[0].tobytes() == s["rows"][0].tobytes()
    db.free()


def _launches(ctx):
    return {k: v["launches"] for k, v in ctx.profile_kernels_read().items()}


def test_launch_counts_do_not_depend_on_the_clusters(ctx):
    one = [ctx.upload(*cloud(257)[0])]
    eight = [ctx.upload(*cloud(n)[0]) for n in (1, 2, 63, 64, 65, 255, 256, 1000)]
    db = ctx.vfh_db(R.recognition_set()["rows"])
    ctx.profile_kernels(True)
    try:
        ctx.vfh_recognise(db, one)
        a = _launches(ctx)
        sa = ctx.vfh_stats()
        ctx.profile_kernels(True)
        ctx.vfh_recognise(db, eight)
        b = _launches(ctx)
        sb = ctx.vfh_stats()
    finally:
        ctx.profile_kernels(False)
    assert a == b and set(a) == {"vfh_scatter_kernel", "vfh_centroid_kernel", "vfh_bins_kernel", "vfh_signature_kernel", "vfh_chi2_kernel"}
    assert all(v == 1 for v in a.values())
    assert (sa["launches"], sa["host_syncs"]) == (sb["launches"], sb["host_syncs"]) == (7, 1)
    db.free()


def test_refusals(ctx, ope):
    (xyz, nrm), _ = cloud(64)
    good = ctx.upload(xyz, nrm)
    rows, q = _table(16, 1)
    db = ctx.vfh_db(rows)
    bad_pt = xyz.copy()
    bad_pt[5, 1] = np.nan
    bad_n = nrm.copy()
    bad_n[7, 2] = np.nan
    cases = {
        "NaN point": lambda: ctx.vfh([good, ctx.upload(bad_pt, nrm)]),
        "NaN normal": lambda: ctx.vfh([ctx.upload(xyz, bad_n)]),
        "NaN normal, recognise": lambda: ctx.vfh_recognise(db, [ctx.upload(xyz, bad_n)]),
        "k = 17": lambda: ctx.vfh_match(db, q, 17),
        "k = 0": lambda: ctx.vfh_match(db, q, 0),
        "k = 17, recognise": lambda: ctx.vfh_recognise(db, [good], k=17),
        "null table": lambda: ctx.vfh_match(None, q, 15),
        "null table, recognise": lambda: ctx.vfh_recognise(None, [good]),
        "m = 0": lambda: ctx.vfh_db(np.zeros((0, 308), F)),
        "no clusters": lambda: ctx.vfh([]),
        "centroid on the viewpoint": lambda: ctx.vfh([good], params=ope.default_vfh_params(use_given_centroid=1)),
    }
    ctx.profile_kernels(True)
    try:
        for what, call in cases.items():
            with pytest.raises(ope.OpeError) as e:
                call()
            assert e.value.code == EINVAL, what
            assert sum(_launches(ctx).values()) == 0, what
            assert ctx.vfh_stats()["launches"] == 0, what
        ctx.vfh([good])   # the context is still usable
        assert sum(_launches(ctx).values()) == 4
    finally:
        ctx.profile_kernels(False)
    db.free()
