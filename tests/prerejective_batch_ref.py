"""ope_prerejective_pose_batch / ope_final_pose_batch_prerejective restated over tests/prerejective_ref.py: the statuses from the key
counts, the seed rules of both entry points, the 16-bit packing of the draws, one prerejective_ref.align per active cluster and the
NaN-row status.  The inputs are the key points and FPFH rows the front end computed (the front end itself is
ope_coarse_pose_batch's and is tested there).

Nothing here calls the library.  test_prerejective_batch_ref.py pins this file against a plain per-cluster loop."""
import numpy as np

import prerejective_ref as ref

PREREJ_OK, PREREJ_EMPTY_TARGET, PREREJ_FEW_TARGET_FEATURES, PREREJ_NAN_FEATURES = 0, 1, 2, 3
COARSE_OK, COARSE_EMPTY_TARGET, COARSE_FEW_TARGET_FEATURES = 0, 1, 2
MIN_TARGET_KEYS = 10        # poseestimator.cpp:40-45


def status_of(n_points, n_keys):
    """Before anything is drawn: an empty cluster, fewer than 10 key points, or a cluster that draws."""
    if n_points == 0:
        return PREREJ_EMPTY_TARGET
    return PREREJ_FEW_TARGET_FEATURES if n_keys < MIN_TARGET_KEYS else PREREJ_OK


def seeds_of(statuses, seed, seeds=None, by_rank=False):
    """The stream every cluster draws with (None: it draws nothing).  seeds[i] when given; otherwise seed + i
    (ope_prerejective_pose_batch) or seed + the number of clusters before i that drew (ope_final_pose_batch_prerejective: the
    estimator's coarse-call counter)."""
    out, rank = [], 0
    for i, s in enumerate(statuses):
        if s != PREREJ_OK:
            out.append(None)
            continue
        out.append(int(seeds[i]) if seeds is not None else (int(seed) + (rank if by_rank else i)) & 0xFFFFFFFFFFFFFFFF)
        rank += 1
    return out


def pack_draws(samp, pick):
    """16 bits per draw: the sample in bits 0-11 (at most 4096 key points), the pick in bits 12-14 (k <= 8)."""
    samp, pick = np.asarray(samp), np.asarray(pick)
    assert samp.min() >= 0 and samp.max() < 4096 and pick.min() >= 0 and pick.max() < 8
    return (samp.astype(np.uint32) | (pick.astype(np.uint32) << 12)).astype(np.uint16)


def unpack_draws(words):
    w = np.asarray(words, np.uint16).astype(np.int32)
    return w & 0xFFF, (w >> 12) & 7


def has_nan_row(samp, src_feat, tgt_feat):
    """A sampled source descriptor without one finite distance to a target descriptor (its row of neighbours is empty)."""
    with np.errstate(invalid="ignore", over="ignore"):
        rows = ref.feature_knn(tgt_feat, np.asarray(src_feat, np.float32)[np.unique(samp)], 1)
    return bool((rows[:, 0] < 0).any())


def no_result(n_src_keys, n_tgt_keys, status):
    return dict(T_best=np.eye(4, dtype=np.float32), error_best=ref.FLT_MAX, best_iteration=-1, inliers_best=0, converged=False, survivors=0,
                n_src_keys=n_src_keys, n_tgt_keys=n_tgt_keys, status=status, seed=0)


def align_batch(model_keys, model_feat, clusters, seeds=None, by_rank=False, seed=1, **params):
    """clusters: per cluster (n_points, key points (m, 3), FPFH rows (m, 33)).  One dict per cluster: the fields of
    ope_prerejective_batch_result and, for a cluster that ran, align()'s arrays under "hyp"."""
    params = dict(params)
    S, K, H = params.get("nr_samples", 3), params.get("k_correspondences", 5), params.get("max_iterations", 50000)
    statuses = [status_of(n, len(k)) for n, k, _ in clusters]
    streams = seeds_of(statuses, seed, seeds, by_rank)
    out = []
    for (n, keys, feat), st, sd in zip(clusters, statuses, streams):
        if st != PREREJ_OK:
            out.append(no_result(len(model_keys), len(keys), st))
            continue
        samp, pick = ref.draws(len(model_keys), S, K, H, sd)
        s2, p2 = unpack_draws(pack_draws(samp, pick))           # what the device reads
        assert (s2 == samp).all() and (p2 == pick).all()
        if has_nan_row(samp, model_feat, feat):
            out.append(no_result(len(model_keys), len(keys), PREREJ_NAN_FEATURES))
            continue
        a = ref.align(model_keys, model_feat, keys, feat, seed=sd, **params)
        b = a["best_iteration"]
        out.append(dict(T_best=a["T_best"], error_best=float(a["error"][b]) if b >= 0 else ref.FLT_MAX, best_iteration=b,
                        inliers_best=int(a["inliers"][b]) if b >= 0 else 0, converged=b >= 0, survivors=int(a["survived"].sum()),
                        n_src_keys=len(model_keys), n_tgt_keys=len(keys), status=PREREJ_OK, seed=sd, hyp=a))
    return out


def coarse_status(status):
    """out[i].coarse.status of ope_final_pose_batch_prerejective."""
    return {PREREJ_OK: COARSE_OK, PREREJ_EMPTY_TARGET: COARSE_EMPTY_TARGET}.get(status, COARSE_FEW_TARGET_FEATURES)
