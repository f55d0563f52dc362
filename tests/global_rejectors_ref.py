"""numpy restatement of the three global correspondence rejectors (include/ope.h, global_rejectors.hip).

The rules restate PCL 1.7.2's correspondence_rejection_median_distance.cpp, correspondence_rejection_one_to_one.cpp and
correspondence_rejection_var_trimmed.cpp as applied WITHOUT a data container, which is how estimateFinePose's block
(poseestimator.cpp:250-292) uses them.  Parity with PCL itself is unpinned, as everywhere in this project; the kernels are pinned
to this file.

d_i is a pair's `distance` field (squared distance, fp32); every comparison is made in fp64 on the widened value.  Pairs stay in
the order given (PCL's one-to-one output is in match order; nothing downstream depends on it).
"""
from __future__ import annotations

import math

import numpy as np

MEDIAN_DISTANCE, ONE_TO_ONE, VAR_TRIMMED = 0, 1, 2
NAN = float("nan")


def _d64(distance):
    d = np.ascontiguousarray(distance, np.float32)
    return d.astype(np.float64)


def median_distance(distance, factor=1.0):
    """keep mask, stats {n_in, n_out, threshold (the median), ratio (NaN)}."""
    d = _d64(distance)
    m = len(d)
    if m == 0:
        return np.zeros(0, bool), dict(n_in=0, n_out=0, threshold=NAN, ratio=NAN)
    median = float(np.sort(d, kind="stable")[m // 2])
    keep = d <= median * float(factor)
    return keep, dict(n_in=m, n_out=int(keep.sum()), threshold=median, ratio=NAN)


def one_to_one(index_query, index_match, distance):
    """Per index_match the smallest distance, on equal distances the smallest index_query; pairs with index_match < 0 are dropped."""
    q = np.ascontiguousarray(index_query, np.int64)
    t = np.ascontiguousarray(index_match, np.int64)
    d = _d64(distance)
    m = len(d)
    keep = np.zeros(m, bool)
    best = {}
    for i in range(m):
        if t[i] < 0:
            continue
        key = (d[i], q[i])
        if t[i] not in best or key < best[t[i]]:
            best[int(t[i])] = key
    for i in range(m):
        if t[i] >= 0 and best[int(t[i])] == (d[i], q[i]):
            keep[i] = True
    return keep, dict(n_in=m, n_out=int(keep.sum()), threshold=NAN, ratio=NAN)


def var_trimmed(distance, min_ratio=0.05, max_ratio=0.95):
    """keep mask, stats {…, threshold (the trimmed distance), ratio, best, idx, margin}.

    margin: the relative gap between the smallest and the second smallest FRMS (inf when there is only one): a test asserts it is at
    least 1e-9, which six fp64 roundings plus the order of the head sum (at most m 2^-53) cannot bridge."""
    d = _d64(distance)
    m = len(d)
    lo = int(math.floor(float(min_ratio) * m))
    hi = int(math.floor(float(max_ratio) * m))
    if hi <= lo:   # PCL: undefined.  Here every pair stays.
        return np.ones(m, bool), dict(n_in=m, n_out=m, threshold=NAN, ratio=1.0, best=-1, idx=-1, margin=math.inf)
    s = np.sort(d, kind="stable")
    L = float(np.sum(s[:lo])) if lo > 0 else 0.0
    j = np.arange(lo, hi, dtype=np.int64)
    idn = (j + 1).astype(np.float64)
    r = idn / float(m)
    inv = 1.0 / (r * r * r)
    frms = inv * inv * (1.0 / idn) * (s[lo:hi] + L)
    k = int(np.argmin(frms))   # the first of the smallest
    best = lo + k
    if len(frms) > 1:
        rest = np.delete(frms, k)
        second = float(rest.min())
        margin = (second - float(frms[k])) / abs(second) if second != 0.0 else 0.0
    else:
        margin = math.inf
    ratio = np.float32(best) / np.float32(m)          # fp32 division, stored as fp32
    idx = int(float(m) * float(ratio))
    trimmed = float(s[idx])
    keep = d < trimmed
    return keep, dict(n_in=m, n_out=int(keep.sum()), threshold=trimmed, ratio=float(ratio), best=best, idx=idx, margin=margin)


def apply(rej, index_query, index_match, distance):
    """rej: (kind, factor, min_ratio, max_ratio) or a dict with those keys."""
    kind = rej["kind"]
    if kind == MEDIAN_DISTANCE:
        return median_distance(distance, rej.get("factor", 1.0))
    if kind == ONE_TO_ONE:
        return one_to_one(index_query, index_match, distance)
    if kind == VAR_TRIMMED:
        return var_trimmed(distance, rej.get("min_ratio", 0.05), rej.get("max_ratio", 0.95))
    raise ValueError(kind)


def apply_list(rejs, index_query, index_match, distance):
    """Each rejector over the survivors of the one before: the final keep mask over the pairs given, and the stats of each."""
    q = np.asarray(index_query)
    t = np.asarray(index_match)
    d = np.asarray(distance, np.float32)
    alive = np.arange(len(d))
    stats = []
    for rej in rejs:
        keep, st = apply(rej, q[alive], t[alive], d[alive])
        stats.append(st)
        alive = alive[keep]
    mask = np.zeros(len(d), bool)
    mask[alive] = True
    return mask, stats


def mixture(m, seed, outlier_share=0.3):
    """The var-trimmed test distances: `outlier_share` of them in [0.5, 1], the rest in [1e-6, 4e-6], shuffled, fp32."""
    rng = np.random.default_rng(seed)
    n_out = int(round(outlier_share * m))
    d = np.concatenate([rng.uniform(1e-6, 4e-6, m - n_out), rng.uniform(0.5, 1.0, n_out)]).astype(np.float32)
    rng.shuffle(d)
    return d
