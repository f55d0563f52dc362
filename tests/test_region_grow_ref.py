"""CPU-side checks of the region-growing reference (tests/region_grow_ref.py, a literal restatement of pcl::RegionGrowing) and of
the statement the device code is built on: with no curvature above the threshold, the sequential flood equals
label(v) = min over all u that reach v in the directed graph (v included) of rank(u).  Also the conditions the GPU scenes must
meet for an exact comparison to be meaningful: distinct curvatures, no k-NN boundary tie, every edge at least 4 ulp from the
cosine threshold."""
import numpy as np
import pytest

import region_grow_ref as R


def min_ancestor_clusters(n, nbrs, passes, curvature, finite, min_size, max_size):
    """The formula, computed by plain propagation to a fixed point: L = rank; L[v] = min(L[v], L[u]) over the edges u -> v."""
    order = R.seed_order(curvature, finite)
    L = np.full(n, -1, np.int64)
    L[order] = np.arange(len(order))
    u, j = np.nonzero((nbrs >= 0) & passes)
    v = nbrs[u, j]
    while True:
        new = L.copy()
        np.minimum.at(new, v, L[u])
        if (new == L).all():
            break
        L = new
    return R.clusters_of_labels(L, min_size, max_size)


def _passes(scene_normals, nbrs, theta):
    with np.errstate(invalid="ignore"):
        return ~(R.abs_dots(scene_normals, nbrs) < R.cos_threshold(theta))


def _same(got, want):
    assert [len(c) for c in got] == [len(c) for c in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("seed", range(8))
def test_formula_equals_the_flood_on_random_directed_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 501))
    k = int(rng.integers(2, 6))
    nbrs = rng.integers(0, n, (n, k)).astype(np.int32)
    nbrs[:, 0] = np.arange(n)
    nbrs[rng.random((n, k)) < 0.2] = -1                       # short lists
    # two normal directions 20 degrees apart: edges between the groups fail at 10 degrees
    grp = rng.random(n) < 0.5
    nrm = np.where(grp[:, None], [0.0, 0.0, 1.0], [np.sin(np.radians(20.0)), 0.0, np.cos(np.radians(20.0))]).astype(np.float32)
    cur = rng.permutation(n).astype(np.float32) / np.float32(4 * n)
    if seed % 2:
        cur[rng.integers(0, n, n // 5)] = cur[0]              # equal curvatures: the index decides
    pts = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    for mn, mx in ((1, n), (3, n // 2)):
        want, _, _ = R.region_grow_pcl(pts, nrm, cur, nbrs, 10 * R.DEG, 1.0, mn, mx)
        got = min_ancestor_clusters(n, nbrs, _passes(nrm, nbrs, 10 * R.DEG), cur, np.ones(n, bool), mn, mx)
        _same(got, want)


@pytest.mark.parametrize("scene", R.gpu_scenes(), ids=lambda s: s.name)
def test_formula_equals_the_flood_on_every_gpu_scene(scene):
    n = len(scene.pts)
    for theta in (scene.theta, 40 * R.DEG):
        want, _, _ = scene.reference(1, theta=theta)
        got = min_ancestor_clusters(n, scene.nbrs, _passes(scene.normals, scene.nbrs, theta), scene.curvature, np.isfinite(scene.pts).all(axis=1),
                                    1, 1000000)
        _same(got, want)


def test_an_active_curvature_test_breaks_the_formula():
    """Four points a, h, b, c with the lists a: {a, h}, h: {h, b}, b: {b, c}, c: {c}, all normals parallel, ranks a < h < b < c and
    h's curvature above the threshold.  PCL: a takes h, h is labelled but not expanded, b starts a region of its own and takes c.
    The formula lets a's label run through h to b and c.  Were h ranked first it would be a seed itself and expand: whether it
    does depends on who ends up a seed, which no monotone fixed point expresses."""
    nbrs = np.array([[0, 1], [1, 2], [2, 3], [3, -1]], np.int32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    pts = np.zeros((4, 3), np.float32)
    cur = np.array([0.01, 0.5, 0.02, 0.03], np.float32)
    seq, _, _ = R.region_grow_pcl(pts, nrm, cur, nbrs, 10 * R.DEG, 0.1, 1, 10)
    assert [c.tolist() for c in seq] == [[0, 1], [2, 3]]
    # (the formula's ranks: curvature order a, b, c, h; h reaches b and c, a reaches h)
    mono = min_ancestor_clusters(4, nbrs, np.ones((4, 2), bool), cur, np.ones(4, bool), 1, 10)
    assert [c.tolist() for c in mono] == [[0, 1, 2, 3]]
    # with the threshold off the two agree again
    off, _, _ = R.region_grow_pcl(pts, nrm, cur, nbrs, 10 * R.DEG, 1.0, 1, 10)
    assert [c.tolist() for c in off] == [[0, 1, 2, 3]]
    # h as the initial seed expands although its curvature is above the threshold
    cur2 = np.array([0.6, 0.5, 0.7, 0.8], np.float32)
    first, _, _ = R.region_grow_pcl(pts, nrm, cur2, nbrs, 10 * R.DEG, 0.1, 1, 10)
    assert [c.tolist() for c in first] == [[1, 2], [0], [3]]


def test_one_way_edges_are_not_undirected():
    last, first = R.one_way(False), R.one_way(True)
    assert last.nbrs.tolist() == [[0, 1], [1, 2], [2, 3], [3, 2]]          # nothing lists x = 0 but itself
    # x = 0 ranked last: the other three are one region and take nothing from it (an undirected union-find would join all four)
    assert [c.tolist() for c in last.reference(1)[0]] == [[1, 2, 3], [0]]
    # ranked first, it takes all four
    assert [c.tolist() for c in first.reference(1)[0]] == [[0, 1, 2, 3]]


def test_chain_answers():
    assert [len(c) for c in R.chain(True).reference(1)[0]] == [R.CHAIN_N]
    against = R.chain(False).reference(1)[0]
    # against the links nothing flows; the closest pair of any point set is mutual, so 0 and 1 stay together
    assert len(against) == R.CHAIN_N - 1 and against[0].tolist() == [0, 1] and all(len(c) == 1 for c in against[1:])
    nb = R.chain(True).nbrs
    assert (nb[2:, 1] == np.arange(1, R.CHAIN_N - 1)).all() and nb[0, 1] == 1 and nb[1, 1] == 0


def test_crease_and_scene4_answers():
    cr = R.crease()
    assert sorted(len(c) for c in cr.reference(1)[0])[-2:] == [1560, 1640] and len(cr.reference(1, theta=40 * R.DEG)[0]) == 1
    s4 = R.scene4()
    sizes = [len(c) for c in s4.reference(50)[0]]
    assert sizes == [2282, 3000, 50]                                     # seed order, not size order
    assert [len(c) for c in s4.reference(500)[0]] == [2282, 3000]
    assert [len(c) for c in s4.reference(50, 2500)[0]] == [2282, 50]
    assert len(s4.reference(1)[0]) == s4.reference(1)[2] > 100


@pytest.mark.parametrize("scene", R.gpu_scenes(), ids=lambda s: s.name)
def test_gpu_scenes_meet_the_input_conditions(scene):
    fin = np.isfinite(scene.pts).all(axis=1)
    cur = scene.curvature[fin]
    assert len(np.unique(cur)) == len(cur) and not np.isnan(cur).any() and cur.max() <= 1.0
    ks = [scene.k] + ([scene.normals_k] if scene.normals_k and scene.normals_k != scene.k else [])
    for k in ks:
        _, d2 = R.knn_lists(scene.pts, k, with_next=True)
        assert (d2[fin, k - 1] != d2[fin, k]).all(), k                   # no tie on the list's boundary
    for theta in (scene.theta, 40 * R.DEG) if scene.name == "crease" else (scene.theta,):
        margin = scene.reference(1, theta=theta)[1]
        assert margin >= 4 * float(np.spacing(R.cos_threshold(theta))), (theta, margin)
