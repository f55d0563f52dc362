"""tests/prerejective_batch_ref.py pinned on its own: against a plain per-cluster loop of prerejective_ref.align, the status and seed
rules on hand-made inputs, the draw packing as a round trip over its whole range, the NaN-row status."""
import numpy as np
import pytest

import prerejective_batch_ref as bref
import prerejective_ref as ref

PARAMS = dict(max_iterations=300, nr_samples=3, k_correspondences=5, similarity_threshold=0.8, max_corr_dist=0.02, inlier_fraction=0.25)


def make_inputs():
    rng = np.random.default_rng(11)
    model = rng.uniform(-0.1, 0.1, (60, 3)).astype(np.float32)
    f_model = rng.uniform(0, 100, (60, 33)).astype(np.float32)
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    moved = (model.astype(np.float64) @ R.T + [0.3, 0.0, 0.1]).astype(np.float32)
    clutter = rng.uniform(-0.1, 0.1, (25, 3)).astype(np.float32) + np.float32(0.3)
    clusters = [
        (500, moved, f_model),                                                                     # the model, moved
        (0, np.zeros((0, 3), np.float32), np.zeros((0, 33), np.float32)),                          # empty
        (400, np.concatenate([moved[:40], clutter]), np.concatenate([f_model[:40], rng.uniform(0, 100, (25, 33)).astype(np.float32)])),
        (5, moved[:5], f_model[:5]),                                                               # fewer than 10 key points
        (300, moved[::-1].copy(), f_model[::-1].copy()),
    ]
    return model, f_model, clusters


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


def test_statuses_come_from_the_counts():
    assert bref.status_of(0, 0) == bref.PREREJ_EMPTY_TARGET
    assert bref.status_of(5, 5) == bref.PREREJ_FEW_TARGET_FEATURES
    assert bref.status_of(900, 9) == bref.PREREJ_FEW_TARGET_FEATURES
    assert bref.status_of(900, 10) == bref.PREREJ_OK
    assert [bref.coarse_status(s) for s in range(4)] == [bref.COARSE_OK, bref.COARSE_EMPTY_TARGET, bref.COARSE_FEW_TARGET_FEATURES,
                                                         bref.COARSE_FEW_TARGET_FEATURES]


def test_seed_rules_of_both_entry_points():
    st = [bref.PREREJ_OK, bref.PREREJ_EMPTY_TARGET, bref.PREREJ_OK, bref.PREREJ_FEW_TARGET_FEATURES, bref.PREREJ_OK]
    assert bref.seeds_of(st, 7) == [7, None, 9, None, 11]                       # seed + i
    assert bref.seeds_of(st, 7, by_rank=True) == [7, None, 8, None, 9]          # seed + clusters before it that drew
    assert bref.seeds_of(st, 7, seeds=[50, 51, 52, 53, 54]) == [50, None, 52, None, 54]
    assert bref.seeds_of(st, 7, seeds=[50, 51, 52, 53, 54], by_rank=True) == [50, None, 52, None, 54]
    assert bref.seeds_of([bref.PREREJ_OK] * 2, 2 ** 64 - 1) == [2 ** 64 - 1, 0]   # uint64 arithmetic


def test_draw_packing_round_trips():
    samp, pick = np.meshgrid(np.arange(4096), np.arange(8), indexing="ij")
    words = bref.pack_draws(samp, pick)
    assert words.dtype == np.uint16 and len(np.unique(words)) == 4096 * 8
    s2, p2 = bref.unpack_draws(words)
    assert (s2 == samp).all() and (p2 == pick).all()
    with pytest.raises(AssertionError):
        bref.pack_draws([4096], [0])
    with pytest.raises(AssertionError):
        bref.pack_draws([0], [8])
    s, p = ref.draws(634, 3, 5, 200, 1)
    s2, p2 = bref.unpack_draws(bref.pack_draws(s, p))
    assert (s2 == s).all() and (p2 == p).all()


@pytest.mark.parametrize("by_rank", [False, True])
def test_batch_is_the_per_cluster_loop(inputs, by_rank):
    model, f_model, clusters = inputs
    got = bref.align_batch(model, f_model, clusters, by_rank=by_rank, seed=3, **PARAMS)
    assert [g["status"] for g in got] == [0, 1, 0, 2, 0]
    rank = 0
    for i, ((n, keys, feat), g) in enumerate(zip(clusters, got)):
        assert g["n_src_keys"] == len(model) and g["n_tgt_keys"] == len(keys)
        if g["status"] != bref.PREREJ_OK:
            assert g["seed"] == 0 and not g["converged"] and g["best_iteration"] == -1 and g["survivors"] == 0
            assert (g["T_best"] == np.eye(4, dtype=np.float32)).all() and g["error_best"] == ref.FLT_MAX
            continue
        seed = 3 + (rank if by_rank else i)
        rank += 1
        want = ref.align(model, f_model, keys, feat, seed=seed, **PARAMS)
        assert g["seed"] == seed and g["best_iteration"] == want["best_iteration"] and g["converged"] == want["converged"]
        assert g["T_best"].tobytes() == want["T_best"].tobytes()
        assert g["survivors"] == int(want["survived"].sum())
        for k in ("samples", "targets", "survived", "T", "inliers", "error"):
            np.testing.assert_array_equal(g["hyp"][k], want[k])
        if want["converged"]:
            assert g["error_best"] == want["error"][want["best_iteration"]] and g["inliers_best"] == want["inliers"][want["best_iteration"]]
    assert got[0]["converged"]                                   # the moved model is found
    with_seeds = bref.align_batch(model, f_model, clusters[::-1], seeds=[g["seed"] for g in got][::-1], **PARAMS)[::-1]
    for a, b in zip(got, with_seeds):                            # a cluster's result depends on its own seed and inputs alone
        assert a["status"] == b["status"] and a["best_iteration"] == b["best_iteration"] and a["T_best"].tobytes() == b["T_best"].tobytes()


def test_nan_rows_give_their_own_status(inputs):
    model, f_model, clusters = inputs
    nan_feat = np.full_like(clusters[0][2], np.nan)
    got = bref.align_batch(model, f_model, [clusters[0], (500, clusters[0][1], nan_feat), clusters[2]], seed=3, **PARAMS)
    assert [g["status"] for g in got] == [bref.PREREJ_OK, bref.PREREJ_NAN_FEATURES, bref.PREREJ_OK]
    assert got[1]["seed"] == 0 and not got[1]["converged"] and (got[1]["T_best"] == np.eye(4, dtype=np.float32)).all()
    alone = bref.align_batch(model, f_model, [clusters[2]], seeds=[5], **PARAMS)[0]
    assert got[2]["seed"] == 5 and got[2]["T_best"].tobytes() == alone["T_best"].tobytes() and got[2]["best_iteration"] == alone["best_iteration"]
    # one NaN target row among finite ones is no NaN status: NaN distances never match, the finite rows still do
    one = clusters[0][2].copy()
    one[3] = np.nan
    assert bref.align_batch(model, f_model, [(500, clusters[0][1], one)], seed=3, **PARAMS)[0]["status"] == bref.PREREJ_OK
    # a NaN MODEL row is one only if it is sampled
    fm = f_model.copy()
    fm[7] = np.nan
    samp, _ = ref.draws(len(model), 3, 5, PARAMS["max_iterations"], 3)
    assert (samp == 7).any()
    assert bref.align_batch(model, fm, [clusters[0]], seed=3, **PARAMS)[0]["status"] == bref.PREREJ_NAN_FEATURES
    assert not bref.has_nan_row(samp[(samp != 7).all(1)][:5], fm, clusters[0][2])
