"""ope_corr_sac_pose_batch restated in numpy on top of tests/corr_sac_ref.py (not a test module): the status rule, the seed rule,
the grouping of clusters into shared draw lists and the per-cluster pipeline from given key points and FPFH rows.  Nothing here
calls the library.  test_corr_sac_batch_ref.py pins this file on its own."""
from __future__ import annotations

import numpy as np

import corr_sac_ref as ref
from plane_ref import replay_loop

F = np.float32
OK, EMPTY_TARGET, FEW_TARGET_FEATURES = 0, 1, 2
MIN_TARGET_FEATURES = 10            # poseestimator.cpp:63-68


def status_of(n_points: int, n_keys: int) -> int:
    """An empty cluster, fewer than 10 cluster key points, or a cluster that reaches the matcher."""
    if n_points == 0:
        return EMPTY_TARGET
    return FEW_TARGET_FEATURES if n_keys < MIN_TARGET_FEATURES else OK


def seeds_of(statuses, seed: int, seeds=None) -> list:
    """Cluster i draws with seeds[i]; without seeds every cluster draws with `seed`, the same for all and not + i (every rejector
    of the reference's loop is a fresh object that never reseeds).  0 for a cluster that did not reach the matcher."""
    return [(seeds[i] if seeds is not None else seed) if s == OK else 0 for i, s in enumerate(statuses)]


def draw_groups(matched_src, seeds) -> list:
    """The draw list of every cluster: clusters with the same seed and the same matched model key points (in match order) share
    one; a cluster with fewer than three matches draws nothing (-1).  matched_src[i]: the model keys of cluster i's matches, or
    None for a cluster that did not reach the matcher.  Lists are numbered in the order of their first cluster."""
    lists, out = {}, []
    for ms, seed in zip(matched_src, seeds):
        if ms is None or len(ms) < 3:
            out.append(-1)
            continue
        key = (int(seed), np.asarray(ms, np.int32).tobytes())
        out.append(lists.setdefault(key, len(lists)))
    return out


def replay(counts, n_matches: int, max_iterations: int, probability: float):
    """RandomSampleConsensus::computeModel over the counts of the hypotheses drawn: (best, iterations)."""
    return replay_loop(np.asarray(counts, np.int32), max(n_matches, 1), max_iterations, probability)


def cluster_pose(model_keys, model_feat, keys, feat, samples=None, thresh=None, **kw):
    """One active cluster from its key points and FPFH rows: corr_sac_ref.coarse_pose's steps, with the draws optionally given
    (a shared list).  The rejector's dict plus matches, dropped, T_svd (float64; the identity without a match)."""
    si, ti, dist, dropped = ref.feature_matches(model_feat, feat)
    out = ref.reject(model_keys, keys, si, ti, samples=samples, thresh=thresh, **kw)
    keep = out["inlier_pos"]
    out.update(matches=(si, ti, dist), dropped=dropped,
               T_svd=ref.svd_pose(np.asarray(model_keys, F)[si[keep]], np.asarray(keys, F)[ti[keep]]))
    return out


def pose_batch(model_keys, model_feat, clusters, seeds=None, **kw):
    """clusters: (n_points, key points, FPFH rows) each.  One dict per cluster: status, seed, list (its draw list or -1) and, for the
    clusters that reached the matcher, cluster_pose's fields.  A shared list is drawn once, for its first cluster."""
    p = dict(ref.DEFAULTS, **kw)
    statuses = [status_of(n, len(k)) for n, k, _ in clusters]
    used = seeds_of(statuses, p["seed"], seeds)
    matches = [ref.feature_matches(model_feat, f) if s == OK else None for s, (_, _, f) in zip(statuses, clusters)]
    groups = draw_groups([m[0] if m is not None else None for m in matches], used)
    drawn, out = {}, []
    mk = np.asarray(model_keys, F).reshape(-1, 3)
    for i, (s, (_, keys, feat)) in enumerate(zip(statuses, clusters)):
        o = dict(status=s, seed=used[i], list=groups[i])
        if s == OK:
            si = matches[i][0]
            thresh = ref.sample_dist_thresh(mk[si]) if len(si) else 0.0
            if groups[i] >= 0 and groups[i] not in drawn:
                drawn[groups[i]] = (ref.draw_samples(mk[si], p["max_iterations"] + 1, used[i], thresh), thresh)
            samples = None
            if groups[i] >= 0:
                samples, t0 = drawn[groups[i]]
                assert t0 == thresh                                   # the same points through the same adds
            o.update(cluster_pose(mk, model_feat, keys, feat, samples=samples, thresh=thresh, **dict(kw, seed=used[i])))
        out.append(o)
    return out
