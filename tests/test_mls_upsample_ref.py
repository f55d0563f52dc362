"""CPU checks of tests/mls_upsample_ref.py, the numpy restatement of pcl::MovingLeastSquares with upsampling VOXEL_GRID_DILATION that
the device is compared against (tests/test_gpu_mls_upsample.py): the fits of orders 3 and 4 against an independent least-squares
solver, the voxel grid against an independent np.unique restatement, the tie rule, the 5 nr_coeff rule, the zero axes below nr_coeff
neighbours, what the operator does to a noisy sphere, and the population facts of the GPU test's cloud.

MEASURED here (numpy float64): normal equations + Cholesky against numpy.linalg.lstsq (QR / SVD) on sqrt(w)-scaled rows, largest
|c - c_lstsq| / max |c_lstsq| over 200 surface points of the GPU test's cloud: order 3 8.2e-13, order 4 2.3e-11 (FIT_REL_MEASURED; the
normal matrices' condition numbers reach ~1e6, so this is what fp64 leaves); the test asserts 4 x those.  Noisy sphere cap (sigma 0.5 mm, R 0.1 m,
radius 0.03, order 4, voxel 0.002): RMS radial error of the upsampled points over that of the input: 0.816584 (must be < 1).
"""
import numpy as np
import pytest

import mls_ref
import mls_upsample_ref as R
from mls_upsample_ref import ORDER, RADIUS, VOXEL

FIT_REL_MEASURED = {3: 8.197e-13, 4: 2.279e-11}
SPHERE_RATIO_MEASURED = 0.816584


@pytest.fixture(scope="module")
def base():
    xyz, n_surface = R.upsample_cloud()
    nbh = mls_ref.neighbourhoods(xyz, RADIUS)
    res = R.mls_results(xyz, RADIUS, ORDER, nbh=nbh)
    ref = [R.mls_upsample(xyz, RADIUS, ORDER, compute_normals=True, voxel_size=VOXEL, dilation_iterations=it, results=res) for it in (0, 1)]
    return dict(xyz=xyz, n_surface=n_surface, nbh=nbh, res=res, ref=ref)


def test_the_cloud_covers_what_it_should(base):
    """The population facts that tests/test_gpu_mls_upsample.py states, so that the cloud cannot silently stop covering them."""
    counts = np.diff(base["nbh"][1])
    fin = base["nbh"][0]
    surf = counts[fin < base["n_surface"]]   # (the non-finite rows were inserted later: close enough for a population check)
    assert surf.min() >= 20 and surf.max() >= 100 and 70 <= np.median(surf) <= 95
    assert 0.5 <= np.mean(surf >= 75) <= 0.85 and np.count_nonzero(surf < 75) >= 500        # both sides of the 5 nr_coeff rule
    assert np.count_nonzero(counts < 3) >= 9 and np.count_nonzero((counts >= 3) & (counts < 15)) >= 10
    assert mls_ref.pairs_near_radius(base["xyz"], RADIUS, ulps=4) == 0
    assert not base["res"]["fit_failed"].any()
    for ref, nvox in zip(base["ref"], (2899, 52685)):
        st = ref["stats"]
        assert st["n_voxels"] == nvox and st["data_size"] == 826 and st["n_valid"] == 3029
        assert 0.1 * nvox <= st["n_rejected_farther"] <= 0.4 * nvox and st["n_invalid_nearest"] >= 9 and st["n_polynomial"] >= 0.5 * nvox
        moved = np.linalg.norm(ref["result"][ref["near_valid"]].astype(np.float64) - ref["pos"][ref["near_valid"]], axis=1)
        assert np.median(moved) > 5e-4 and np.median(np.abs(ref["n_disp"][ref["applied"]])) > 5e-4
    assert R.undecided(base["ref"][0]).sum() == 0 and R.undecided(base["ref"][1]).sum() == 2


@pytest.mark.parametrize("order", [3, 4])
def test_fit_against_an_independent_least_squares_solver(base, order):
    xyz = base["xyz"]
    fin, offs, nidx, _ = base["nbh"]
    worst, done = 0.0, 0
    for k in range(0, 3000, 15):
        nb = xyz[nidx[offs[k]:offs[k + 1]]]
        if len(nb) < R.nr_coeff(order):
            continue
        one = R.mls_result(xyz[fin[k]], nb, order, True, RADIUS * RADIUS)
        # the same problem, by rows: minimise sum w (P^T c - f)^2
        u, v, n, mean = one["u"], one["v"], one["n"], one["mean"]
        de = nb.astype(np.float64) - mean
        w = np.exp(-((de * de).sum(axis=1).astype(np.float32)).astype(np.float64) / (RADIUS * RADIUS))   # PCL's weight: the squared distance is a float
        uc, vc, f = de @ u, de @ v, de @ n
        cols = [uc ** a * vc ** b for a in range(order + 1) for b in range(order - a + 1)]
        c_ls = np.linalg.lstsq(np.stack(cols, axis=1) * np.sqrt(w)[:, None], f * np.sqrt(w), rcond=None)[0]
        worst = max(worst, float(np.abs(one["c"] - c_ls).max() / np.abs(c_ls).max()))
        done += 1
    print(f"\n[mls_upsample_ref] order {order}: {done} fits, largest |c - c_lstsq| / max |c_lstsq| = {worst:.3e}")
    assert done >= 190 and worst <= 4 * FIT_REL_MEASURED[order]


def grid_by_unique(xyz, voxel_size, iterations):
    """An independent restatement of MLSVoxelGrid and its dilation: arrays and np.unique instead of a set of keys."""
    p = xyz[np.isfinite(xyz).all(axis=1)]
    vs = np.float32(voxel_size)
    bmin, bmax = p.min(axis=0), p.max(axis=0)
    ds = int(1.5 * float(np.max(bmax - bmin)) / float(vs))
    cells = np.unique(np.trunc((p - bmin) / vs).astype(np.int64), axis=0)
    dropped = 0
    off = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int64)
    for _ in range(iterations):
        c = (cells[:, None, :] + off[None, :, :]).reshape(-1, 3)
        inside = ((c >= 0) & (c < ds)).all(axis=1)
        dropped += int(np.count_nonzero(~inside))
        cells = np.unique(c[inside], axis=0)
    keys = (cells[:, 0] * ds + cells[:, 1]) * ds + cells[:, 2]
    order = np.argsort(keys, kind="stable")
    pos = cells[order].astype(np.float32) * vs + bmin
    return keys[order], ds, pos, dropped


@pytest.mark.parametrize("iterations", [0, 1])
def test_voxel_grid_against_an_independent_restatement(base, iterations):
    xyz = base["xyz"]
    keys, ds, bmin = R.voxel_keys(xyz, VOXEL, iterations)
    k2, ds2, pos2, dropped = grid_by_unique(xyz, VOXEL, iterations)
    assert ds == ds2 and np.array_equal(keys, k2) and np.all(np.diff(keys) > 0)
    assert R.voxel_positions(keys, ds, bmin, VOXEL).tobytes() == pos2.tobytes()
    assert np.array_equal(keys, base["ref"][iterations]["keys"])
    if iterations:
        assert dropped > 0   # the voxels of the lowest points have neighbours below cell 0: dropped, not wrapped


def test_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(8)
    pts = rng.uniform(0, 0.05, (200, 3)).astype(np.float32)
    pts[150] = pts[20]                      # an exact duplicate
    pts[7] = [np.nan, 0, 0]
    # two points mirrored about a voxel position: an exact fp32 tie that is not a duplicate
    q = np.array([0.025, 0.025, 0.08], np.float32)
    pts[180] = q + np.float32([0.001, 0, 0]); pts[60] = q - np.float32([0.001, 0, 0])
    pos = np.r_[pts[[20, 150, 33]], q[None, :], rng.uniform(0, 0.05, (50, 3)).astype(np.float32)]
    got = R.nearest_lowest_index(pos, pts)
    want = []
    for p in pos:   # brute force, one point after the other
        best, arg = np.inf, -1
        for i, t in enumerate(pts):
            if not np.isfinite(t).all():
                continue
            d = p - t
            d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if d2 < best:
                best, arg = d2, i
        want.append(arg)
    assert np.array_equal(got, want) and got[0] == 20 and got[1] == 20 and got[3] == 60


def test_the_polynomial_needs_five_times_nr_coeff_neighbours():
    rng = np.random.default_rng(11)
    a = mls_ref.paraboloid_patch(rng, 75, side=0.018, centre=(0.0, 0.0, 1.0))
    b = mls_ref.paraboloid_patch(rng, 74, side=0.018, centre=(0.3, 0.0, 1.0))
    pts = np.r_[a, b]
    ref = R.mls_upsample(pts, RADIUS, ORDER, voxel_size=VOXEL)
    res_m = np.r_[np.full(75, 75), np.full(74, 74)]
    ok = ref["near_valid"]
    assert ok.all() and np.array_equal(ref["applied"], res_m[ref["nearest"]] == 75)
    assert ref["applied"].any() and (~ref["applied"]).any() and np.all(ref["n_disp"][~ref["applied"]] == 0.0)
    assert np.abs(ref["n_disp"][ref["applied"]]).max() > 0
    assert ref["stats"]["n_polynomial"] == int(ref["applied"].sum())


def test_zero_axes_below_nr_coeff_neighbours(base):
    """A point with 3 <= m < nr_coeff neighbours has u = v = 0 (as 1.7 leaves them): every voxel it serves lands on its `mean`."""
    res, ref = base["res"], base["ref"][1]
    few = res["valid"] & (res["m"] < R.nr_coeff(ORDER))
    assert few.sum() >= 10 and not res["u"][few].any() and not res["v"][few].any()
    served = ref["near_valid"] & few[ref["nearest"]]
    assert served.sum() >= 10
    assert ref["result"][served].tobytes() == res["mean"][ref["nearest"][served]].astype(np.float32).tobytes()
    assert not ref["applied"][served].any()


def test_upsampling_a_noisy_sphere_lands_nearer_the_sphere():
    pts = mls_ref.sphere_points(np.random.default_rng(R.SEED), 1500, max_polar=np.radians(75.0))
    ref = R.mls_upsample(pts, RADIUS, ORDER, voxel_size=VOXEL)
    before, after = mls_ref.radial_rms(pts), mls_ref.radial_rms(ref["xyz"])
    print(f"\n[mls_upsample_ref] noisy sphere: {len(ref['xyz'])} points out, RMS radial error {before:.4e} m before, {after:.4e} m after, ratio {after / before:.6f}")
    assert len(ref["xyz"]) > 800 and ref["stats"]["n_polynomial"] > 500
    assert after / before < 1.0
    assert abs(after / before - SPHERE_RATIO_MEASURED) < 5e-6
