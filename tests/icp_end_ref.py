"""How an ICP run ends: a plain fp64 numpy/scipy restatement of the 1-NN + SVD loop with PCL's ending rule.

The library decides the end of every registration in one device function (icp_update_lane, csrc/icp_update.hpp); this
module states the same rule on the host, independently of the library and of the C oracle:

  search    scipy's cKDTree, pairs beyond max_corr_dist dropped (squared distance > max_corr_dist^2);
  guard     fewer than min_correspondences pairs end the run BEFORE the estimate (icp_mod.hpp:232-240): `iterations`
            is not incremented, converged = 0, state 5, the final transform stays what it was;
  estimate  Umeyama without scale in fp64, rounded to float (transformation_ is a Matrix4f), F = Tk @ F;
  rule      DefaultConvergenceCriteria::hasConverged as icp_mod.hpp:164-168 wires it: rotation threshold
            1 - transformation_epsilon, SQUARED translation against transformation_epsilon, prev_mse from DBL_MAX,
            cur_mse computed only when neither the iteration test nor the transform test fired, so a run that ends on
            one of those reports the MSE of the iteration before (DBL_MAX if there was none).

failure_after_max_iter: PCL's hasConverged returns false at the iteration cap and the reference's `do ... while
(!converged_)` would go round for ever; the library (and this restatement) ends the run there with converged = 0 and
state 0 (NOT_CONVERGED).  oracle.icp follows PCL to the letter, so it must never be called with the flag set.

Besides the outcome the run returns a per-iteration trace, and margins() says by which factor every comparison the rule
made was decided: test inputs are chosen so that no comparison is a close call, which is what allows exact assertions
on `iterations`, `converged`, `state` and `n_corr` against kernels whose sums differ in the last bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
from scipy.spatial import cKDTree

DBL_MAX = float(np.finfo(np.float64).max)

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)


@dataclass
class Params:
    max_iterations: int = 10
    transformation_epsilon: float = 0.0
    euclidean_fitness_epsilon: float = 0.0
    max_corr_dist: float = math.sqrt(DBL_MAX)
    min_correspondences: int = 3
    mse_threshold_absolute: float = 1e-12
    failure_after_max_iter: int = 0

    def as_kwargs(self) -> dict:
        """The fields under the names both ope.default_icp_params and oracle.IcpParams use."""
        return dict(self.__dict__)


@dataclass
class Criteria:
    """DefaultConvergenceCriteria's state between two calls of hasConverged."""
    max_iterations: int
    failure_after_max_iter: int
    rotation_threshold: float
    translation_threshold: float
    mse_threshold_relative: float
    mse_threshold_absolute: float
    prev_mse: float = DBL_MAX
    cur_mse: float = DBL_MAX
    state: int = NOT_CONVERGED

    @classmethod
    def wired(cls, p: Params) -> "Criteria":
        """icp_mod.hpp:164-168."""
        return cls(p.max_iterations, p.failure_after_max_iter, 1.0 - p.transformation_epsilon, p.transformation_epsilon,
                   p.euclidean_fitness_epsilon, p.mse_threshold_absolute)


def rotation_and_translation(Tk):
    """(cos_angle, squared translation) of an incremental transform given as float32 (4,4), computed in double."""
    T = np.asarray(Tk, np.float32).astype(np.float64)
    return 0.5 * (T[0, 0] + T[1, 1] + T[2, 2] - 1.0), float(T[0, 3] ** 2 + T[1, 3] ** 2 + T[2, 3] ** 2)


def convergence_step(c: Criteria, iterations: int, Tk, mse: float):
    """One call of hasConverged.  Returns (stop, converged): `stop` ends the loop; the two differ only under
    failure_after_max_iter.  c.state, c.cur_mse and c.prev_mse are left as PCL leaves them."""
    c.state = NOT_CONVERGED
    if iterations >= c.max_iterations:
        if c.failure_after_max_iter:
            return True, False
        c.state = ITERATIONS
        return True, True
    cos_angle, tr2 = rotation_and_translation(Tk)
    if cos_angle >= c.rotation_threshold and tr2 <= c.translation_threshold:
        c.state = TRANSFORM
        return True, True
    c.cur_mse = mse
    diff = abs(c.cur_mse - c.prev_mse)
    if diff < c.mse_threshold_absolute:
        c.state = ABS_MSE
        return True, True
    if diff / c.prev_mse < c.mse_threshold_relative:
        c.state = REL_MSE
        return True, True
    c.prev_mse = c.cur_mse
    return False, False


def umeyama(src, tgt) -> np.ndarray:
    """Rigid least-squares transform src -> tgt (Umeyama 1991, no scale), fp64 (4,4)."""
    ms, mt = src.mean(0), tgt.mean(0)
    H = (tgt - mt).T @ (src - ms) / len(src)
    U, s, Vt = np.linalg.svd(H)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


@dataclass
class Outcome:
    T: np.ndarray                  # final transformation, fp64 (4,4)
    Tk: np.ndarray                 # last incremental transform (float32 values); identity if no estimate was made
    iterations: int
    converged: bool
    state: int
    last_mse: float
    n_corr: int
    corr_q: np.ndarray             # the last search's pairs: source index, target index, squared distance
    corr_m: np.ndarray
    corr_d2: np.ndarray
    trace: list = field(default_factory=list)


def icp(src, tgt, p: Params, guess=None) -> Outcome:
    """The loop.  One trace row per search: n_corr, corr_gap (how far, relatively, the pair distance nearest to
    max_corr_dist is from it), and for searches that led to an estimate Tk, one_minus_cos, tr2, mse, dmse = |mse -
    prev_mse|, rel = dmse / prev_mse (the last two against the prev_mse the rule held at that moment)."""
    src = np.asarray(src, np.float32).astype(np.float64)
    tgt = np.asarray(tgt, np.float32).astype(np.float64)
    tree = cKDTree(tgt)
    F = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)
    Tk = np.eye(4, dtype=np.float32)
    c = Criteria.wired(p)
    iterations, converged, trace = 0, False, []
    while True:
        work = src @ F[:3, :3].T + F[:3, 3]
        d, m = tree.query(work, k=1)
        keep = ~(d * d > p.max_corr_dist ** 2)
        gap = float(np.min(np.abs(d / p.max_corr_dist - 1.0)))
        q = np.flatnonzero(keep)
        m, d = m[keep], d[keep]
        row = dict(n_corr=len(q), corr_gap=gap)
        trace.append(row)
        if len(q) < p.min_correspondences:
            c.state = NO_CORRESPONDENCES
            converged = False
            break
        Tk = umeyama(work[q], tgt[m]).astype(np.float32)
        F = Tk.astype(np.float64) @ F
        iterations += 1
        mse = float(np.mean(d * d))
        cos_angle, tr2 = rotation_and_translation(Tk)
        row.update(Tk=Tk, one_minus_cos=1.0 - cos_angle, tr2=tr2, mse=mse, dmse=abs(mse - c.prev_mse),
                   rel=abs(mse - c.prev_mse) / c.prev_mse)
        stop, converged = convergence_step(c, iterations, Tk, mse)
        if stop:
            break
    return Outcome(F, Tk, iterations, converged, c.state, c.cur_mse, len(q), q.astype(np.int32), m.astype(np.int32),
                   (d * d), trace)


def _ratio(a: float, b: float) -> float:
    """How many times larger the larger of two non-negative numbers is (inf if one of them is zero or negative: such a
    threshold is switched off and such a quantity cannot be pushed across by rounding)."""
    lo, hi = min(a, b), max(a, b)
    if lo <= 0.0:
        return math.inf
    return hi / lo


def margins(trace, p: Params) -> list:
    """Every comparison the rule made, iteration by iteration up to the stop, with the factor that decided it.

    One dict per comparison: iteration (1-based search number), test, quantity, threshold, fired, margin.  For the
    threshold tests `margin` is the ratio between quantity and threshold (>= 1); the transform test is the conjunction
    of two comparisons, so where it did not fire its margin is that of the comparison that missed most clearly, where it
    fired that of the one that passed most narrowly.  For `pairs` the margin is |n_corr - min_correspondences| / n_corr
    (inf for n_corr = 0) and for `max_corr_dist` the relative distance of the nearest pair distance to the limit.  The
    iteration test compares two integers and has no margin."""
    out = []
    c = Criteria.wired(p)
    it = 0
    for k, row in enumerate(trace, 1):
        n = row["n_corr"]
        fired = n < p.min_correspondences
        out.append(dict(iteration=k, test="pairs", quantity=n, threshold=p.min_correspondences, fired=fired,
                        margin=abs(n - p.min_correspondences) / n if n else math.inf))
        out.append(dict(iteration=k, test="max_corr_dist", quantity=row["corr_gap"], threshold=p.max_corr_dist, fired=False,
                        margin=row["corr_gap"]))
        if fired:
            break
        it += 1
        if it >= c.max_iterations:
            break
        rot_q, rot_t = row["one_minus_cos"], 1.0 - c.rotation_threshold
        tr_q, tr_t = row["tr2"], c.translation_threshold
        rot_ok, tr_ok = rot_q <= rot_t, tr_q <= tr_t
        fired = rot_ok and tr_ok
        if fired:
            m = min(_ratio(rot_q, rot_t), _ratio(tr_q, tr_t))
        else:
            m = max(_ratio(rot_q, rot_t) if not rot_ok else 0.0, _ratio(tr_q, tr_t) if not tr_ok else 0.0)
        out.append(dict(iteration=k, test="transform", quantity=(rot_q, tr_q), threshold=(rot_t, tr_t), fired=fired, margin=m))
        if fired:
            break
        dm = abs(row["mse"] - c.prev_mse)
        fired = dm < c.mse_threshold_absolute
        out.append(dict(iteration=k, test="abs_mse", quantity=dm, threshold=c.mse_threshold_absolute, fired=fired,
                        margin=_ratio(dm, c.mse_threshold_absolute)))
        if fired:
            break
        rel = dm / c.prev_mse
        fired = rel < c.mse_threshold_relative
        out.append(dict(iteration=k, test="rel_mse", quantity=rel, threshold=c.mse_threshold_relative, fired=fired,
                        margin=_ratio(rel, c.mse_threshold_relative)))
        if fired:
            break
        c.prev_mse = row["mse"]
    return out


MIN_FACTOR = 4.0        # every threshold comparison is decided by at least this factor
MIN_PAIR_GAP = 0.02     # the pair count clears min_correspondences by at least this share of itself
MIN_DIST_GAP = 1e-3     # no pair distance within this relative distance of max_corr_dist (fp32 rounding is 1e-7)


def check_margins(trace, p: Params) -> float:
    """Asserts that no comparison of the run was a close call; returns the smallest threshold factor seen (inf if every
    threshold was switched off)."""
    worst = math.inf
    for m in margins(trace, p):
        if m["test"] == "pairs":
            assert m["margin"] >= MIN_PAIR_GAP, m
        elif m["test"] == "max_corr_dist":
            assert m["margin"] >= MIN_DIST_GAP, m
        else:
            assert m["margin"] >= MIN_FACTOR, m
            worst = min(worst, m["margin"])
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  Every threshold is taken from the restatement's own trace (the geometric mean of two consecutive values),
# never written down as a number.
def rigid(rx, ry, rz, t) -> np.ndarray:
    rx, ry, rz = np.deg2rad([rx, ry, rz])
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def body_a(synth):
    """A bumpy torus and a posed, noisy copy: the trace falls 50-200x per iteration down to a noise floor."""
    P = synth.bumpy_torus(2000)
    T = rigid(2, -3, 1, [0.004, -0.002, 0.003])
    Q = P.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + np.random.default_rng(1).normal(0, 0.5e-3, (2000, 3))
    return P, Q.astype(np.float32)


def body_b():
    """2000 uniform points that want to move +3 mm in x plus a 10 x 10 lattice that wants -4.5 mm: with max_corr_dist =
    5 mm the first search pairs all 2100, the second (after the estimate moved everything about +2.6 mm) only the 2000."""
    A = np.random.default_rng(3).uniform(-0.1, 0.1, (2000, 3))
    g = 0.004 * np.arange(10)
    L = np.stack([np.zeros(100), *[a.ravel() for a in np.meshgrid(g, g, indexing="ij")]], axis=1) + [0.0, 0.0, 0.15]
    src = np.concatenate([A, L])
    tgt = np.concatenate([A + [0.003, 0, 0], L - [0.0045, 0, 0]])
    return src.astype(np.float32), tgt.astype(np.float32)


OFF = dict(transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, mse_threshold_absolute=-1.0)
TRACE_ITERATIONS = 10


def _gm(a, b):
    return math.sqrt(a * b)


def _first_clear_drop(values, lo=1, floor=0.0):
    """First index k >= lo with values[k-1] / values[k] >= 16 (a factor 4 either side of the geometric mean) and
    values[k] > floor."""
    for k in range(lo, len(values)):
        if values[k] > floor and values[k - 1] / values[k] >= MIN_FACTOR ** 2:
            return k
    raise AssertionError(("no clear drop", values))


@dataclass
class Case:
    name: str
    src: np.ndarray
    tgt: np.ndarray
    params: Params
    guess: np.ndarray | None = None
    ref: Outcome | None = None


_CASES: dict = {}


def cases(synth) -> dict:
    """name -> Case, the restatement's outcome attached (computed once per process)."""
    if _CASES:
        return _CASES
    P, Q = body_a(synth)
    tr = icp(P, Q, Params(max_iterations=TRACE_ITERATIONS, **OFF)).trace
    mk = lambda **kw: Params(**{**OFF, "max_iterations": 50, **kw})
    out = {}
    out["iterations"] = Case("iterations", P, Q, mk(max_iterations=3))
    out["failure"] = Case("failure", P, Q, mk(max_iterations=3, failure_after_max_iter=1))
    # TRANSFORM: both comparisons must pass, so the quantity that decides is the larger of the two, each relative to the one
    # threshold they share; cos_angle moves in steps of 3e-8 near 1, hence the floor on the epsilon
    both = [max(r["one_minus_cos"], r["tr2"]) for r in tr]
    k = _first_clear_drop(both, lo=3, floor=1e-7)
    eps = _gm(both[k - 1], both[k])
    assert eps >= 1e-6, eps
    out["transform"] = Case("transform", P, Q, mk(transformation_epsilon=eps))
    dm = [abs(tr[i]["mse"] - tr[i - 1]["mse"]) if i else DBL_MAX for i in range(len(tr))]
    k = _first_clear_drop(dm, lo=3)
    out["abs_mse"] = Case("abs_mse", P, Q, mk(mse_threshold_absolute=_gm(dm[k - 1], dm[k])))
    rel = [dm[i] / tr[i - 1]["mse"] if i else 1.0 for i in range(len(tr))]
    k = _first_clear_drop(rel, lo=3)
    out["rel_mse"] = Case("rel_mse", P, Q, mk(euclidean_fitness_epsilon=_gm(rel[k - 1], rel[k])))
    # every point finds a partner, and that is still too few: the guess must come back untouched
    out["no_corr_at_0"] = Case("no_corr_at_0", P, Q, mk(min_correspondences=2100), guess=rigid(1, 0, -1, [0.001, 0.0, -0.001]))
    Bs, Bt = body_b()
    out["no_corr_mid_run"] = Case("no_corr_mid_run", Bs, Bt, mk(max_corr_dist=0.005, min_correspondences=2050))
    for c in out.values():
        c.ref = icp(c.src, c.tgt, c.params, c.guess)
    _CASES.update(out)
    return _CASES


EXPECTED_ENDINGS = {   # name -> (iterations or None where the trace decides, converged, state)
    "iterations": (3, True, ITERATIONS), "failure": (3, False, NOT_CONVERGED), "transform": (None, True, TRANSFORM),
    "abs_mse": (None, True, ABS_MSE), "rel_mse": (None, True, REL_MSE), "no_corr_at_0": (0, False, NO_CORRESPONDENCES),
    "no_corr_mid_run": (1, False, NO_CORRESPONDENCES),
}
