"""The restatement of pcl::RegionGrowingRGB that ope_region_grow_rgb computes (region_grow_rgb_ref.py), checked on
the CPU: the parallel forms the device uses against the literal sequential ones on random graphs, PCL's two-pointer pass on hand
cases, and the order of segment neighbours with equal distances."""
import numpy as np
import pytest

import region_grow_rgb_ref as ref


def random_kept(rng, S, k):
    """a directed segment graph: per segment up to k neighbours (dist, t), ascending by (dist, t), distances from a small set so
    that equal ones occur"""
    kept = []
    for s in range(S):
        others = [t for t in range(S) if t != s]
        m = int(rng.integers(0, min(k, len(others)) + 1))
        ts = rng.choice(others, m, replace=False) if m else []
        kept.append(sorted((float(rng.choice([0.5, 1.0, 1.5, 2.0, 3.0])), int(t)) for t in ts))
    return kept


def test_parent_formula_equals_the_sequential_first_merge_pass():
    rng = np.random.default_rng(2024)
    joined = 0
    for trial in range(3000):
        S = int(rng.integers(1, 41))
        kept = random_kept(rng, S, int(rng.integers(1, 7)))
        means = [[int(v) for v in rng.integers(0, 4, 3) * 5] for _ in range(S)]
        d2_thr, r2_thr = float(rng.choice([0.75, 1.0, 1.75, 10.0])), float(rng.choice([1.0, 26.0, 51.0, 1000.0]))
        a = ref.merge_a_sequential(kept, means, d2_thr, r2_thr)
        b = ref.merge_a_parent(kept, means, d2_thr, r2_thr)
        assert a == b, (trial, kept, means)
        joined += a[1] < S
    assert joined > 500            # the trials do merge


def test_min_index_reachability_equals_the_queue_flood():
    """symmetric edge tests over asymmetric lists: u -> v iff v is in u's list and the two colours are close"""
    rng = np.random.default_rng(7)
    several = 0
    for trial in range(400):
        n = int(rng.integers(1, 60))
        finite = rng.random(n) > 0.1
        col = rng.integers(0, 6, n)
        edges = [[] for _ in range(n)]
        for u in np.flatnonzero(finite):
            cand = [int(v) for v in np.flatnonzero(finite) if v != u]
            lst = rng.choice(cand, min(len(cand), int(rng.integers(0, 4))), replace=False) if cand else []
            edges[u] = [int(v) for v in lst if abs(int(col[u]) - int(col[v])) <= 1]
        a_seg, a_count = ref.flood_segments(n, finite, edges)
        b_seg, b_count = ref.min_reach_segments(n, finite, edges)
        assert a_count == b_count and np.array_equal(a_seg, b_seg), trial
        assert (a_seg[~finite] == -1).all()
        several += a_count > 1
    assert several > 100


@pytest.mark.parametrize("sizes, want, swaps", [
    ([0, 0, 0], [0, 1, 2], 0),                      # all empty: nothing to bring forward
    ([4, 5, 6], [0, 1, 2], 0),                      # none empty
    ([0, 0, 7, 8], [3, 2, 1, 0], 2),                # the empty regions at the front: the pass REORDERS (8 before 7)
    ([7, 0, 0, 8, 9], [0, 4, 3, 2, 1], 2),          # in the middle
    ([7, 8, 0, 0], [0, 1, 2, 3], 0),                # at the end
    ([0, 5], [1, 0], 1),
    ([], [], 0),
    ([3], [0], 0),
])
def test_two_pointer_pass(sizes, want, swaps):
    order, n = ref.two_pointer_order(sizes)
    assert order == want and n == swaps
    # the non-empty regions come first, and nothing is lost
    filled = [sizes[r] > 0 for r in order]
    assert filled == sorted(filled, reverse=True) and sorted(order) == list(range(len(sizes)))


def test_kept_neighbours_order_equal_distances_by_segment():
    pairs = {9: 2.0, 4: 1.0, 7: 1.0, 2: 2.0, 5: 0.5, 8: 2.0}
    assert ref.kept_neighbours(pairs, 100) == [(0.5, 5), (1.0, 4), (1.0, 7), (2.0, 2), (2.0, 8), (2.0, 9)]
    assert ref.kept_neighbours(pairs, 4) == [(0.5, 5), (1.0, 4), (1.0, 7), (2.0, 2)]      # the cut falls inside a run of equals
    assert ref.kept_neighbours(pairs, 2) == [(0.5, 5), (1.0, 4)]
    assert ref.kept_neighbours({}, 3) == []


def test_tiny_scene_by_hand():
    """four collinear points, k = 2, colours 0 / 0 / 200 / 200: x = 0 lists x = 1 but nothing lists x = 0; two segments, whose
    means differ too much to merge by colour; both below min_size 3, so merge B moves the first into the second"""
    pts = ref.one_way_points()
    rgb = np.array([ref.word(0, 0, 0), ref.word(0, 0, 0), ref.word(200, 0, 0), ref.word(200, 0, 0)], np.uint32)
    nbrs = ref.knn_lists(pts, 2)
    clusters, info = ref.region_grow_rgb_pcl(pts, rgb, nbrs, distance_threshold=10.0, min_size=1, k=2)
    assert [c.tolist() for c in clusters] == [[0, 1], [2, 3]] and info["one_way_edges"] == 1 and info["segment_pairs"] == 1
    clusters, info = ref.region_grow_rgb_pcl(pts, rgb, nbrs, distance_threshold=10.0, min_size=3, k=2)
    assert [c.tolist() for c in clusters] == [[0, 1, 2, 3]] and info["regions_absorbed"] == 1 and info["swaps"] == 1
    # the alpha byte plays no part
    clusters2, _ = ref.region_grow_rgb_pcl(pts, rgb | np.uint32(0xAB000000), nbrs, distance_threshold=10.0, min_size=3, k=2)
    assert [c.tolist() for c in clusters2] == [[0, 1, 2, 3]]
