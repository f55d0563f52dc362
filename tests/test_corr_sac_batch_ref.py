"""tests/corr_sac_batch_ref.py pinned on its own (no GPU, no library): a shared draw list equals each member's own corr_sac_ref draws,
clusters split into separate lists when a row is dropped or a seed differs, the statuses for 0 / 9 / 10 target rows, the cases of
0 / 2 / 3 matches, and the replay on hand-made count sequences."""
import math

import numpy as np

import corr_sac_batch_ref as bref
import corr_sac_ref as ref

F = np.float32
KW = dict(inlier_threshold=0.02, max_iterations=40, probability=0.99)


def scene(seed, n_model=24, n_tgt=30):
    """A model of n_model key points with tie-free descriptors and a target that holds a moved copy of it plus extra rows: every
    model row finds its own copy."""
    rng = np.random.default_rng(seed)
    mk = rng.uniform(-0.1, 0.1, (n_model, 3)).astype(F)
    mf = rng.uniform(0, 100, (n_model, 33)).astype(F)
    a = 0.4
    R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    order = rng.permutation(n_tgt)
    keys = np.concatenate([(mk.astype(np.float64) @ R.T + [0.03, -0.02, 0.05]).astype(F), rng.uniform(-0.1, 0.1, (n_tgt - n_model, 3)).astype(F)])
    feat = np.concatenate([mf, rng.uniform(0, 100, (n_tgt - n_model, 33)).astype(F)])
    return mk, mf, keys[order], feat[order]


def test_a_shared_draw_list_equals_each_members_own_draws():
    mk, mf, k0, f0 = scene(1)
    _, _, k1, f1 = scene(1, n_tgt=41)                 # the same model rows matched, another target
    out = bref.pose_batch(mk, mf, [(len(k0), k0, f0), (len(k1), k1, f1)], **KW)
    assert [o["list"] for o in out] == [0, 0] and [o["seed"] for o in out] == [ref.DEFAULTS["seed"]] * 2
    for o, (k, f) in zip(out, ((k0, f0), (k1, f1))):
        own = ref.coarse_pose(mk, mf, k, f, **KW)     # draws made for this cluster alone
        np.testing.assert_array_equal(o["samples"], own["samples"])
        assert o["thresh"] == own["thresh"] and o["T"].tobytes() == own["T"].tobytes()
        np.testing.assert_array_equal(o["counts"], own["counts"])
        assert (o["best"], o["iterations"], o["found"]) == (own["best"], own["iterations"], own["found"])
        np.testing.assert_array_equal(o["inlier_pos"], own["inlier_pos"])
        assert o["T_svd"].tobytes() == own["T_svd"].tobytes() and len(o["samples"]) > 0
    assert out[0]["found"] and len(out[0]["inlier_pos"]) == len(mk)


def test_a_dropped_row_or_another_seed_splits_the_lists():
    mk, mf, k0, f0 = scene(2)
    mf2 = mf.copy()
    assert bref.draw_groups([np.arange(24), np.arange(24), np.arange(24)], [5, 5, 5]) == [0, 0, 0]
    assert bref.draw_groups([np.arange(24), np.arange(24), np.arange(24)], [5, 6, 5]) == [0, 1, 0]
    assert bref.draw_groups([np.arange(24), np.delete(np.arange(24), 7), np.arange(24)], [5, 5, 5]) == [0, 1, 0]
    assert bref.draw_groups([np.arange(2), None, np.arange(3)], [5, 0, 5]) == [-1, -1, 0]
    # through the pipeline: a target whose rows are all NaN but for ten drops nothing (every model row still finds one of the ten);
    # a model row of NaN is dropped in every cluster alike, so the lists stay shared
    mf2[7] = np.nan
    out = bref.pose_batch(mk, mf2, [(len(k0), k0, f0), (len(k0), k0[::-1], f0[::-1])], **KW)
    assert [o["dropped"] for o in out] == [1, 1] and [o["list"] for o in out] == [0, 0]
    assert 7 not in out[0]["matches"][0]
    seeded = bref.pose_batch(mk, mf, [(len(k0), k0, f0), (len(k0), k0, f0), (0, k0[:0], f0[:0])], seeds=[3, 4, 9], **KW)
    assert [o["list"] for o in seeded] == [0, 1, -1] and [o["seed"] for o in seeded] == [3, 4, 0]
    own = ref.coarse_pose(mk, mf, k0, f0, **dict(KW, seed=4))
    np.testing.assert_array_equal(seeded[1]["samples"], own["samples"])
    assert not np.array_equal(seeded[0]["samples"], seeded[1]["samples"])


def test_statuses_for_0_9_and_10_target_rows():
    assert bref.status_of(0, 0) == bref.EMPTY_TARGET
    assert bref.status_of(500, 9) == bref.FEW_TARGET_FEATURES
    assert bref.status_of(500, 10) == bref.OK
    assert bref.status_of(5, 5) == bref.FEW_TARGET_FEATURES
    assert bref.seeds_of([0, 1, 2, 0], 12345) == [12345, 0, 0, 12345]            # the same seed for every cluster, not + i
    assert bref.seeds_of([0, 1, 2, 0], 12345, [7, 8, 9, 10]) == [7, 0, 0, 10]
    mk, mf, k0, f0 = scene(3)
    out = bref.pose_batch(mk, mf, [(0, k0[:0], f0[:0]), (9, k0[:9], f0[:9]), (10, k0[:10], f0[:10])], **KW)
    assert [o["status"] for o in out] == [bref.EMPTY_TARGET, bref.FEW_TARGET_FEATURES, bref.OK]
    assert "T_svd" not in out[0] and "T_svd" not in out[1] and len(out[2]["matches"][0]) == len(mk)


def test_zero_two_and_three_matches():
    mk, mf, k0, f0 = scene(4, n_model=12, n_tgt=12)
    for n_valid, want_h in ((0, 0), (2, 0), (3, None)):
        m = mf.copy()
        m[n_valid:] = np.nan                          # only the first n_valid model rows can match
        o = bref.pose_batch(mk, m, [(len(k0), k0, f0)], **KW)[0]
        assert o["status"] == bref.OK and len(o["matches"][0]) == n_valid and o["dropped"] == 12 - n_valid
        if want_h == 0:
            assert o["list"] == -1 and len(o["samples"]) == 0 and not o["found"] and o["best"] == -1 and o["iterations"] == 0
            assert (o["T_best"] == np.eye(4)).all()
            np.testing.assert_array_equal(o["inlier_pos"], np.arange(n_valid))
            if n_valid == 0:
                assert (o["T_svd"] == np.eye(4)).all()
            else:
                assert not (o["T_svd"] == np.eye(4)).all()        # the SVD over all (two) matches
        else:
            assert o["list"] == 0
            if len(o["samples"]):                     # three matches: one triangle, drawn if its edges pass the threshold
                assert sorted(o["samples"][0]) == [0, 1, 2] and o["found"]
            else:
                assert not o["found"] and o["best"] == -1
                np.testing.assert_array_equal(o["inlier_pos"], np.arange(3))


def test_replay_on_hand_made_counts():
    # 10 matches, probability 0.99: k = log(0.01) / log(1 - (c / 10)^3)
    assert bref.replay([], 10, 100, 0.99) == (-1, 0)                   # nothing drawn: no model
    assert bref.replay([10], 10, 100, 0.99) == (0, 1)                  # every match: k collapses, one iteration
    k5 = math.log(0.01) / math.log(1 - 0.5 ** 3)                       # 34.5
    assert bref.replay([5] * 100, 10, 100, 0.99) == (0, math.ceil(k5))
    assert bref.replay([5] * 20, 10, 100, 0.99) == (0, 20)             # the list runs dry first
    assert bref.replay([5] * 100, 10, 7, 0.99) == (0, 8)               # max_iterations + 1 at the most
    assert bref.replay([3, 3, 6, 6, 10, 10], 10, 100, 0.99) == (4, 5)  # a tie keeps the earlier one
    assert bref.replay([0, 0, 0], 10, 100, 0.99) == (0, 3)             # a count of zero still beats -INT_MAX
