"""Cases for the ending tests whose reference is oracle.icp: the estimators and searches tests/icp_end_ref.py does not restate.

icp_end_ref.py restates only the 1-NN + SVD loop; for point-to-plane (LLS and LM), normal shooting and reciprocal search the
reference is the C oracle.  The rule under test is the same, so the inputs follow the same discipline: no distance limit and
no rejector that is a close call (the pair count is then the cloud's size, or decided by exact index comparisons), the
REL_MSE threshold is the geometric mean of two consecutive values of the oracle's own |dMSE| / prev that lie a factor >= 16
apart, and every stop lies where the oracle itself is resolved: its float and double instantiations of LM within 1e-4 / 4 of
each other on the final and on the last incremental transform, within 1e-3 / 4 on last_mse.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from icp_end_ref import MIN_FACTOR, NOT_CONVERGED, OFF, REL_MSE, _gm, rigid

def _posed_pair(synth, n, noise_seed):
    """Two samplings of the model surface, the second posed: a real MSE floor (the samplings differ)."""
    P, nP = synth.model_surface(n, 5, return_normals=True)
    Q0, nQ0 = synth.model_surface(n, 6, return_normals=True)
    off = np.array([0, 0, 0.6])
    T = rigid(2.0, -1.5, 3.0, [0.004, -0.003, 0.002])
    Q = (Q0.astype(np.float64) + off) @ T[:3, :3].T + T[:3, 3]
    nQ = nQ0.astype(np.float64) @ T[:3, :3].T
    return (P + off.astype(np.float32)).astype(np.float32), nP.astype(np.float32), Q.astype(np.float32), nQ.astype(np.float32)


def _noisy_copy(P, nP, T, sigma, seed):
    Q = (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + np.random.default_rng(seed).normal(0, sigma, P.shape)).astype(np.float32)
    return Q, (nP.astype(np.float64) @ T[:3, :3].T).astype(np.float32)


def estimator_inputs(synth) -> dict:
    """name -> (src, src_nrm, tgt, tgt_nrm, kw): kw holds the search / estimator fields common to ope and the oracle."""
    P, nP, Q, nQ = _posed_pair(synth, 2000, 2)
    # normal shooting and reciprocal search converge slowly from afar: a small pose, the same cloud plus noise
    Ts = rigid(1, -1, 0.5, [0.002, -0.001, 0.001])
    S, nS = _noisy_copy(P, nP, Ts, 0.3e-3, 2)
    # LM: PCL's minimiser stops on a float-sized tolerance, so its float and double instantiations part by more than the
    # device's tolerances while the steps are large; on this copy they agree from iteration 4 on (T, Tk and MSE), while the
    # MSE still moves by several percent at iteration 5
    L, nL = _noisy_copy(P, nP, rigid(2, -3, 1, [0.004, -0.002, 0.003]), 0.3e-3, 3)
    torus = synth.bumpy_torus(3000)
    half = (torus.astype(np.float64) @ Ts[:3, :3].T + Ts[:3, 3] + np.random.default_rng(4).normal(0, 0.3e-3, (3000, 3)))[::2]
    return {
        "lls": (P, nP, Q, nQ, dict(estimator=1)),
        # (float LM returns an exactly zero step once it has settled, and an identity increment passes the transform test even
        # at epsilon 0: a negative epsilon takes that test out, so that the ending does not hang on LM's precision)
        "lm": (P, nP, L, nL, dict(estimator=2, transformation_epsilon=-1.0)),
        "normal_shooting": (P, nP, S, nS, dict(corr_mode=1, k_normal_shooting=20, use_surface_normal_rej=1, surface_normal_thr=0.7)),
        "reciprocal": (torus, None, half.astype(np.float32), None, dict(use_reciprocal=1)),
    }


def oracle_run(oracle, inp, **kw):
    src, sn, tgt, tn, base = inp
    p = oracle.default_icp_params()
    for k, v in {**dict(acc_mode=1, transform_mode=1, lm_precision=1), **OFF, **base, **kw}.items():
        setattr(p, k, v)
    assert not p.failure_after_max_iter, "oracle.icp never ends with the flag set (module docstring)"
    return oracle.icp(src, tgt, p, src_nrm=sn, tgt_nrm=tn)


def oracle_mse_trace(oracle, inp, n=14) -> list:
    """mse[i] of iteration i + 1: a run that ends on ITERATIONS at K reports the MSE of iteration K - 1."""
    return [oracle_run(oracle, inp, max_iterations=k).last_mse for k in range(2, n + 2)]


RESOLVED = 1e-4 / MIN_FACTOR      # the oracle's own float / double gap has to stay this far under the 1e-4 the device is held to


def last_increment(hist) -> np.ndarray:
    """T_n T_(n-1)^-1 from the oracle's per-iteration final transforms (its first transform for a one-iteration run)."""
    H = np.asarray(hist, np.float64)
    return H[-1] @ np.linalg.inv(H[-2]) if len(H) > 1 else H[-1]


def lm_gap(oracle, inp, **kw):
    """(|dT|_F, |dTk|_F, relative last_mse gap) between the oracle's float and double instantiations of an LM run; zeros for
    the other estimators, which have one instantiation.  PCL's LM stops on a float-sized tolerance, so before ICP has settled
    the two take a different number of LM steps and differ by more than the device is held to."""
    if inp[4].get("estimator") != 2:
        return 0.0, 0.0, 0.0
    a, b = (oracle_run(oracle, inp, lm_precision=prec, **kw) for prec in (0, 1))
    return (float(np.linalg.norm(a.T.astype(np.float64) - b.T.astype(np.float64))),
            float(np.linalg.norm(last_increment(a.T_hist) - last_increment(b.T_hist))),
            abs(a.last_mse - b.last_mse) / b.last_mse)


def resolved(gap) -> bool:
    """The oracle's own gap stays a factor 4 under what the device is held to: 1e-4 on T and Tk, rel 1e-3 on last_mse."""
    return gap[0] <= RESOLVED and gap[1] <= RESOLVED and gap[2] <= 1e-3 / MIN_FACTOR


@dataclass
class EstimatorCase:
    name: str
    inp: tuple
    eps: float              # the REL_MSE threshold
    rel_margin: float
    mse: list
    k_iter: int             # the ITERATIONS case's cap
    endings: dict           # "iterations" / "failure" / "rel_mse" -> (kw, oracle.IcpOut with converged / state as the library ends the run)


_EST_CASES: dict = {}


def clear_drops(rel, lo=2):
    """Every k >= lo with rel[k-1] / rel[k] >= 16: a threshold at their geometric mean is missed and passed by a factor >= 4."""
    return [k for k in range(lo, len(rel)) if rel[k] > 0.0 and rel[k - 1] / rel[k] >= MIN_FACTOR ** 2]


def estimator_cases(synth, oracle) -> dict:
    """The reference is oracle.icp with sums in double and, for LM, the double instantiation (the device's 6 x 6 algebra is
    double); the float instantiation must agree on every ending (test_icp_end_ref.py).

    ITERATIONS cap: the smallest K >= 3 at which the oracle is resolved and the MSE still moves by more than 1 % (so that
    rel 1e-3 on last_mse tells the stale value from the fresh one).  REL_MSE stop: the first clear drop of |dMSE| / prev at
    which the oracle is resolved."""
    if _EST_CASES:
        return _EST_CASES
    for name, inp in estimator_inputs(synth).items():
        mse = oracle_mse_trace(oracle, inp)
        rel = [1.0] + [abs(mse[i] - mse[i - 1]) / mse[i - 1] for i in range(1, len(mse))]
        K = next(K for K in range(3, 12) if rel[K - 1] > 0.01 and resolved(lm_gap(oracle, inp, max_iterations=K)))
        itk = oracle_run(oracle, inp, max_iterations=K)
        fail = oracle_run(oracle, inp, max_iterations=K)
        fail.converged, fail.state = False, NOT_CONVERGED
        for k in clear_drops(rel):
            eps = _gm(rel[k - 1], rel[k])
            stop_kw = dict(max_iterations=50, euclidean_fitness_epsilon=eps)
            if resolved(lm_gap(oracle, inp, **stop_kw)):
                break
        else:
            raise AssertionError((name, "no REL_MSE stop at which the oracle is resolved", rel))
        # every comparison up to the stop: misses by rel[i] / eps, the stop passes by eps / rel[k]
        margin = min([r / eps for r in rel[:k]] + [eps / rel[k]])
        assert margin >= MIN_FACTOR, (name, rel, eps)
        stop = oracle_run(oracle, inp, **stop_kw)
        assert (stop.iterations, stop.converged, stop.state) == (k + 1, True, REL_MSE), (name, stop.iterations, stop.state, k)
        _EST_CASES[name] = EstimatorCase(name, inp, eps, margin, mse, K, {
            "iterations": (dict(max_iterations=K), itk),
            "failure": (dict(max_iterations=K, failure_after_max_iter=1), fail),
            "rel_mse": (stop_kw, stop)})
    return _EST_CASES


def singular_lls_case():
    """A target lattice in the plane z = 0 whose normals are all (0, 0, 1): every row of the point-to-plane system is
    (y, -x, 0, 0, 0, 1) . n_z, so columns 3-5 of A^T A are exactly zero.  PCL would propagate NaNs; the library ends the
    run in state 5 with the guess untouched (ope.h)."""
    g = 0.01 * np.arange(-10, 11)
    X, Y = np.meshgrid(g, g, indexing="ij")
    tgt = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1.0]], np.float32), (len(tgt), 1))
    src = (tgt + np.array([0.002, -0.001, 0.003], np.float32)).astype(np.float32)
    return src, tgt, nrm, rigid(0, 0, 1, [0.001, 0.0, 0.0])
