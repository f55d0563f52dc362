"""tests/peel_ref.py pinned on the CPU: every round of the peel is RandomSampleConsensus::computeModel run literally (one hypothesis at
a time) plus the refinement on that round's remainder; labels, remainder and inliers partition the cloud; the `while` test is
`>` in double, made before each fit; the degenerate clouds end as the reference's loop ends on them."""
import numpy as np
import pytest

import peel_ref as pf
import plane_ref as pr
from peel_scenes import SCENES, noise_with_nans, room_scene

SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def peeled():
    out = {}
    for name, sizes in SCENES.items():
        pts = room_scene(sizes)
        out[name] = (pts, {seed: pf.except_plane(pts, seed=seed) for seed in SEEDS})
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_every_round_is_the_literal_loop_on_its_remainder(peeled, seed):
    pts, runs = peeled["three"]
    _, p = runs[seed]
    assert len(p["coeffs"]) == 3
    for r in range(3):
        sub = pts[p["remainders"][r]]
        model, it, _ = pr.literal_loop(sub, 0.01, 50, 0.99, seed)
        inl = np.flatnonzero(pr.within(model, sub, 0.01))
        coeff = pr.optimize_coefficients(sub, inl, model)
        assert coeff.tobytes() == p["coeffs"][r].tobytes() and it == p["iterations"][r]
        assert np.array_equal(p["remainders"][r][pr.within(coeff, sub, 0.01)], p["inliers"][r])
        if r:
            assert np.array_equal(p["remainders"][r], np.setdiff1d(p["remainders"][r - 1], p["inliers"][r - 1]))


@pytest.mark.parametrize("seed", SEEDS)
def test_three_planes_are_peeled_and_three_blobs_are_left(peeled, seed):
    clusters, p = peeled["three"][1][seed]
    assert sorted(p["counts"].tolist()) == [3000, 5000, 8000] and p["counts"][0] == 8000
    assert p["stop"] == pf.FRACTION and len(p["rest_idx"]) == 4000
    sizes = [len(c) for c in clusters]
    assert len(sizes) == 3 and all(abs(s - w) <= 10 for s, w in zip(sizes, (1500, 1200, 900)))   # the 250-blob is dropped


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("seed", SEEDS)
def test_labels_remainder_and_inliers_partition_the_cloud(peeled, name, seed):
    pts, runs = peeled[name]
    clusters, p = runs[seed]
    n = len(pts)
    everything = np.concatenate(p["inliers"] + [p["rest_idx"]])
    assert np.array_equal(np.sort(everything), np.arange(n))
    for r, inl in enumerate(p["inliers"]):
        assert np.array_equal(np.flatnonzero(p["labels"] == r), inl)
    assert np.array_equal(np.flatnonzero(p["labels"] == -1), p["rest_idx"])
    assert all(np.isin(c, p["rest_idx"]).all() and (np.diff(c) > 0).all() for c in clusters)


@pytest.mark.parametrize("seed", SEEDS)
def test_a_remainder_of_exactly_the_fraction_stops_the_loop(peeled, seed):
    clusters, p = peeled["exact"][1][seed]
    assert p["counts"].tolist() == [8000, 6000] and len(p["rest_idx"]) == 6000 and p["stop"] == pf.FRACTION   # 6000 > 0.3 * 20000 is false
    assert len(clusters[0]) == 2000   # the untouched side wall


@pytest.mark.parametrize("seed", SEEDS)
def test_one_point_over_the_fraction_runs_a_third_round(peeled, seed):
    _, p = peeled["over"][1][seed]
    assert p["counts"][:2].tolist() == [8000, 5999] and len(p["counts"]) == 3 and p["stop"] == pf.FRACTION


def test_the_cap_stops_after_that_many_planes():
    pts = room_scene(SCENES["exact"])
    clusters, p = pf.except_plane(pts, max_planes=1, seed=1)
    assert p["stop"] == pf.MAX_PLANES and p["counts"].tolist() == [8000] and len(p["rest_idx"]) == 12000 and len(clusters) == 5
    _, p2 = pf.except_plane(pts, max_planes=2, seed=1)
    assert p2["stop"] == pf.FRACTION and len(p2["counts"]) == 2   # the fraction test comes first


def test_degenerate_clouds():
    p = pf.peel(np.zeros((0, 3), np.float32))
    assert len(p["coeffs"]) == 0 and p["stop"] == pf.FRACTION and len(p["rest_idx"]) == 0
    p = pf.peel(np.array([[0, 0, 1], [1, 0, 1.5], [0, 1, 2]], np.float32))
    assert p["counts"].tolist() == [3] and len(p["rest_idx"]) == 0 and p["stop"] == pf.FRACTION
    p = pf.peel(np.tile(np.array([[0.25, -1.0, 2.0]], np.float32), (500, 1)))
    assert len(p["coeffs"]) == 0 and p["stop"] == pf.NO_INLIERS and len(p["rest_idx"]) == 500


@pytest.mark.parametrize("seed", SEEDS)
def test_structureless_noise_is_peeled_slab_by_slab(seed):
    pts, bad = noise_with_nans()
    p = pf.peel(pts, seed=seed)
    assert len(p["coeffs"]) in (19, 20) and p["stop"] == pf.FRACTION
    assert np.isin(bad, p["rest_idx"]).all() and len(p["rest_idx"]) <= 900
