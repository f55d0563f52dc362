"""Pins tests/mls_ref.py (the moving-least-squares reference the GPU tests compare the device with) without a GPU: exactness on a
plane, an independent second implementation, the drop and plane-only rules, unitOrthogonal's branches, the orders, the Gaussian
parameter, and that the operator does denoise."""
import numpy as np
import pytest

import mls_ref
from mls_ref import RADIUS


def independent_mls(xyz, radius, order=2, sqr_gauss_param=None):
    """Written from the algorithm's text, not from mls_ref: brute-force neighbourhoods, numpy.linalg.eigh for the plane,
    numpy.linalg.lstsq on sqrt(w)-scaled rows for the fit.  Returns {index: (point, unit normal of the fitted surface)}."""
    X = np.asarray(xyz, np.float32).astype(np.float64)
    h2 = radius * radius if sqr_gauss_param is None else sqr_gauss_param
    out = {}
    for i, q in enumerate(X):
        nb = X[((X - q) ** 2).sum(axis=1) <= radius * radius]
        if len(nb) < 3:
            continue
        mu = nb.mean(axis=0)
        _, vec = np.linalg.eigh((nb - mu).T @ (nb - mu))
        n = vec[:, 0]
        foot = q - ((q - mu) @ n) * n
        normal = n
        if len(nb) >= (order + 1) * (order + 2) // 2:
            b1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
            b1 /= np.linalg.norm(b1)
            b2 = np.cross(n, b1)
            rel = nb - foot
            s, t, height = rel @ b1, rel @ b2, rel @ n
            cols = [s ** a * t ** b for a in range(order + 1) for b in range(order + 1 - a)]
            sw = np.sqrt(np.exp(-(rel ** 2).sum(axis=1) / h2))
            coef = np.linalg.lstsq(np.stack(cols, axis=1) * sw[:, None], height * sw, rcond=None)[0]
            foot = foot + coef[0] * n
            if order >= 1:
                normal = n - coef[order + 1] * b1 - coef[1] * b2   # gradient terms: d/ds is term (1, 0), d/dt is term (0, 1)
        out[i] = (foot, normal / np.linalg.norm(normal))
    return out


def test_points_on_a_tilted_plane_come_back_unchanged():
    # coordinates on a 2^-9 grid and a plane with dyadic coefficients: every point is on the plane exactly, in float already
    g = np.arange(-12, 13) / 512.0
    x, y = np.meshgrid(g, g)
    pts = np.c_[x.ravel(), y.ravel(), 0.5 * x.ravel() - 0.25 * y.ravel() + 1.0].astype(np.float32)
    r = mls_ref.mls_smooth(pts, RADIUS, compute_normals=True)
    assert r["stats"]["n_out"] == len(pts) and r["stats"]["n_plane_only"] == 0
    assert np.abs(r["xyz64"] - pts.astype(np.float64)).max() < 1e-12
    n = np.array([0.5, -0.25, -1.0]) / np.linalg.norm([0.5, -0.25, -1.0])
    assert np.abs(np.abs(r["normals"].astype(np.float64) @ n) - 1.0).max() < 1e-6


@pytest.mark.parametrize("surface", ["paraboloid", "sphere"])
def test_reference_agrees_with_an_independent_implementation(surface):
    """Tolerance 1e-9 m on positions.  Both sides work in fp64 on the same float inputs; what separates them is the conditioning
    of the 6 x 6 fit: the monomials of coordinates up to 0.02 m span 1 .. 1.6e-7, the normal equations the reference solves square
    that (condition ~1e10 at worst against ~1e5 for lstsq), so of fp64's 1.1e-16 about 1e-6 relative survives in c[0], which is
    itself below 1e-3 m: 1e-9 m.  Measured: 5e-12 m on both surfaces."""
    rng = np.random.default_rng(11)
    pts = mls_ref.paraboloid_patch(rng, 2000, side=0.26) if surface == "paraboloid" else mls_ref.sphere_points(rng, 2000)
    ref = mls_ref.mls_smooth(pts, RADIUS, compute_normals=True)
    ind = independent_mls(pts, RADIUS)
    assert sorted(ind) == ref["idx"].tolist()
    dp, dn = 0.0, 0.0
    for k, i in enumerate(ref["idx"]):
        p, n = ind[int(i)]
        dp = max(dp, np.abs(ref["xyz64"][k] - p).max())
        rn = ref["normals"][k].astype(np.float64)
        dn = max(dn, 1.0 - abs(float(rn @ n)) / np.linalg.norm(rn))
    print(f"{surface}: max |dp| = {dp:.3e} m, max 1 - |cos| of the normals = {dn:.3e}")
    assert dp < 1e-9
    assert dn < 1e-9   # (float normals: the rounding's 6e-8 per component enters the cosine squared)


def test_drop_rule_and_plane_only_rule():
    far = np.array([[5.0, 0, 0], [5.001, 0, 0]], np.float32)                                       # a pair: dropped
    lone = np.array([[9.0, 0, 0]], np.float32)                                                       # alone: dropped
    five = np.array([[0, 0, 0], [0.004, 0, 0.001], [0, 0.004, 0], [0.004, 0.004, 0], [0.002, 0.001, 0.002]], np.float32)   # 3 <= 5 < 6
    bad = np.array([[np.nan, 0, 0], [0.001, 0.001, np.inf]], np.float32)                             # never a neighbour
    pts = np.concatenate([far, five, bad, lone])
    r = mls_ref.mls_smooth(pts, RADIUS, compute_normals=True)
    assert r["idx"].tolist() == [2, 3, 4, 5, 6]
    assert r["stats"] == dict(n_in=10, n_out=5, n_plane_only=5, n_dropped=5, neighbours_total=2 * 2 + 5 * 5 + 1)
    # plane only: each point is its projection on the least-squares plane of the five, the normal is the plane's unit normal
    mu = pts[2:7].astype(np.float64).mean(axis=0)
    n = np.linalg.eigh((pts[2:7] - mu).T.astype(np.float64) @ (pts[2:7] - mu).astype(np.float64))[1][:, 0]
    want = pts[2:7] - ((pts[2:7] - mu) @ n)[:, None] * n
    assert np.abs(r["xyz64"] - want).max() < 1e-12
    assert np.abs(np.abs(r["normals"] @ n) - 1.0).max() < 1e-6
    # with order 1 (3 coefficients) the same five points are fitted
    assert mls_ref.mls_smooth(pts, RADIUS, order=1)["stats"]["n_plane_only"] == 0


def test_unit_orthogonal_takes_both_branches():
    for n in ([0.6, 0.0, 0.8], [0.0, 1e-3, 1.0], [1e-13, 1e-13, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]):
        n = np.array(n) / np.linalg.norm(n)
        v = mls_ref.unit_orthogonal(n)
        assert abs(v @ n) < 1e-15 and abs(np.linalg.norm(v) - 1.0) < 1e-15
        first = abs(n[0]) > abs(n[2]) * 1e-12 or abs(n[1]) > abs(n[2]) * 1e-12
        assert (v[2] == 0.0) if first else (v[0] == 0.0)
    assert mls_ref.unit_orthogonal([1e-13, 1e-13, 1.0])[0] == 0.0 and mls_ref.unit_orthogonal([0.0, 1e-3, 1.0])[2] == 0.0


@pytest.mark.parametrize("order", [0, 1])
def test_lower_orders_agree_with_the_independent_implementation(order):
    rng = np.random.default_rng(5)
    pts = mls_ref.paraboloid_patch(rng, 600, side=0.12)
    ref = mls_ref.mls_smooth(pts, RADIUS, order=order, compute_normals=True)
    ind = independent_mls(pts, RADIUS, order=order)
    assert ref["stats"]["n_plane_only"] == 0
    for k, i in enumerate(ref["idx"]):
        p, n = ind[int(i)]
        assert np.abs(ref["xyz64"][k] - p).max() < 1e-9
        rn = ref["normals"][k].astype(np.float64)
        assert 1.0 - abs(float(rn @ n)) / np.linalg.norm(rn) < 1e-9


def test_explicit_gauss_parameter():
    rng = np.random.default_rng(6)
    pts = mls_ref.paraboloid_patch(rng, 600, side=0.12)
    dflt = mls_ref.mls_smooth(pts, RADIUS)
    same = mls_ref.mls_smooth(pts, RADIUS, sqr_gauss_param=RADIUS * RADIUS)
    tight = mls_ref.mls_smooth(pts, RADIUS, sqr_gauss_param=1e-4)
    assert np.array_equal(dflt["xyz64"], same["xyz64"])
    assert np.abs(dflt["xyz64"] - tight["xyz64"]).max() > 1e-6
    ind = independent_mls(pts, RADIUS, sqr_gauss_param=1e-4)
    assert max(np.abs(tight["xyz64"][k] - ind[int(i)][0]).max() for k, i in enumerate(tight["idx"])) < 1e-9


def test_smoothing_reduces_the_radial_error_of_a_noisy_sphere():
    pts = mls_ref.sphere_points(np.random.default_rng(mls_ref.BASE_SEED), 2000)
    r = mls_ref.mls_smooth(pts, RADIUS)
    before, after = mls_ref.radial_rms(pts[r["idx"]]), mls_ref.radial_rms(r["xyz"])
    print(f"noisy sphere: RMS radial error {before:.4e} -> {after:.4e} m, ratio {after / before:.6f}")
    assert after < before
