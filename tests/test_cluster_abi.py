"""CPU-side checks of Euclidean cluster extraction (ope_euclidean_clusters, ope_euclidean_clusters_cloud): declared, exported
and bound; the ctypes structs lay out exactly as the C compiler lays out ope_cluster_params / ope_cluster_stats; the defaults
are the reference's literals (objectsegmentationplane.cpp:85-87); and the host reference the GPU tests compare with agrees
with a literal port of PCL's seed-queue search, order included."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_probe import c_layout, ctypes_layout
from conftest import ROOT, load_pkg
from cluster_ref import pcl_bfs, reference_clusters

HEADER = os.path.join(ROOT, "include", "ope.h")
ENTRIES = ("ope_cluster_default_params", "ope_euclidean_clusters", "ope_euclidean_clusters_cloud", "ope_cluster_last_stats")


@pytest.fixture(scope="module")
def ope():
    pkg = load_pkg()
    pkg.build_library()
    return pkg


@pytest.mark.parametrize("name", ENTRIES)
def test_cluster_entry_is_declared_exported_and_bound(ope, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(ope.LIB_PATH), name)
    assert name in {n for n, _, _ in ope.ABI}


def test_cluster_layouts_match_the_c_compiler(ope):
    structs = {ope.ClusterParams: "ope_cluster_params", ope.ClusterStats: "ope_cluster_stats"}
    got = ctypes_layout(structs)
    got["abi"] = 5   # the change only adds to the ABI
    assert got == c_layout(structs, extra={"abi": "OPE_ABI_VERSION"})


def test_cluster_defaults_are_the_reference_literals(ope):
    p = ope.default_cluster_params()
    assert p.tolerance == 0.05     # setClusterTolerance (0.05) (objectsegmentationplane.cpp:85)
    assert p.min_size == 300       # setMinClusterSize (300) (:86)
    assert p.max_size == 100000    # setMaxClusterSize (1e5) (:87)


def _random_cloud(seed, n=240, nan_share=0.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (12, 3))
    pts = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.03, (n, 3))
    pts = pts.astype(np.float32)
    bad = rng.random(n) < nan_share
    pts[bad, rng.integers(0, 3, int(bad.sum()))] = np.where(rng.random(int(bad.sum())) < 0.5, np.nan, np.inf)
    return pts


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("min_size,max_size", [(1, 1000), (3, 60), (10, 100000)])
def test_host_reference_equals_pcls_seed_queue_search(seed, min_size, max_size):
    pts = _random_cloud(seed, nan_share=0.03 if seed % 2 else 0.0)
    tol = 0.045
    want = pcl_bfs(pts, tol, min_size, max_size)
    got = reference_clusters(pts, tol, min_size, max_size)
    if len(want) <= 16:        # PCL's order is defined (a stable sort) only up to 16 clusters
        assert [c.tolist() for c in got] == [c.tolist() for c in want]
    else:
        assert sorted(c.tolist() for c in got) == sorted(c.tolist() for c in want)
        assert [len(c) for c in got] == [len(c) for c in want]


def test_pcl_order_among_equal_sizes_is_the_smallest_index():
    # three separated pairs and one triple, discovered in index order: sizes 3, 2, 2, 2 with the pairs by first index
    pts = np.array([[0, 0, 0], [5, 0, 0], [0, 0.01, 0], [10, 0, 0], [5, 0.01, 0], [20, 0, 0], [10, 0.01, 0], [20, 0.01, 0],
                    [20, 0.02, 0]], np.float32)
    want = [[5, 7, 8], [0, 2], [1, 4], [3, 6]]
    assert [c.tolist() for c in pcl_bfs(pts, 0.015, 1, 10)] == want
    assert [c.tolist() for c in reference_clusters(pts, 0.015, 1, 10)] == want


def test_boundary_predicate_is_float_flann_order():
    tol = 0.05
    r2 = np.float32(float(np.float32(tol)) ** 2)
    a = np.zeros(3, np.float32)
    b = np.array([np.sqrt(np.float64(r2)), 0, 0], np.float32)
    from cluster_ref import flann_d2
    # the largest x with x*x <= r2 in float
    while flann_d2(a, b) > r2:
        b[0] = np.nextafter(b[0], np.float32(0))
    while flann_d2(a, np.array([np.nextafter(b[0], np.float32(1)), 0, 0], np.float32)) <= r2:
        b[0] = np.nextafter(b[0], np.float32(1))
    joined = reference_clusters(np.stack([a, b]), tol, 1, 10)
    apart = reference_clusters(np.stack([a, np.array([np.nextafter(b[0], np.float32(1)), 0, 0], np.float32)]), tol, 1, 10)
    assert [c.tolist() for c in joined] == [[0, 1]]
    assert [c.tolist() for c in apart] == [[0], [1]]
