"""Batched coarse stage (ope_coarse_pose_batch, coarse_batch.hip): estimateCoarsePose of one model against many raw candidate
clusters in one call.

Stage by stage (uniform sampling, normals, FPFH) against the single-cloud calls and the oracle; every cluster's pose against
oracle.estimate_coarse_pose and against ope_sacia on the same inputs; byte-reproducible whatever else is in the batch; the same
launches for any batch size; edge cases, refusals, and the reference's candidate loop (rosinterface.cpp:243-262) at C1 size.
"""
import importlib
import os

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(ROOT, "tests", "golden")
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def ctx():
    ope = load_pkg()
    c = ope.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model():
    xyz, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    return np.ascontiguousarray(xyz, np.float32)


def rigid(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = synth.rot_xyz(rx, ry, rz)
    T[:3, 3] = t
    return T


def apply(T, p):
    return (p.astype(np.float64) @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]).astype(np.float32)


def frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


def raw_candidates(k, scene_at, seed=0):
    """K raw candidate clusters, built like test_gpu_icp_batch.c1_candidates but not reduced to fine inputs: the C1 scene
    cluster at position scene_at, rigidly moved copies of it (seeded) and synth distractors near the object."""
    g = np.load(os.path.join(GOLD, "drill_scene_c1.npz"))
    scene = g["scene"]
    rng = np.random.default_rng(seed)
    c = scene.mean(0)
    out = []
    for j in range(k):
        if j == scene_at:
            cloud = scene
        elif j % 2:
            a = rng.uniform(30, 90, 3) * rng.choice([-1, 1], 3)
            t = rng.uniform(0.08, 0.15, 3) * rng.choice([-1, 1], 3)
            M = rigid(*a, [0, 0, 0])
            cloud = ((scene - c) @ M[:3, :3].T.astype(np.float32) + c + t).astype(np.float32)
        else:
            d = synth.model_surface(4000, seed=100 + j) * np.float32(rng.uniform(0.6, 1.2))
            cloud = (d - d.mean(0) + c + rng.uniform(-0.01, 0.01, 3)).astype(np.float32)
        out.append(np.ascontiguousarray(cloud, np.float32))
    return out


def with_nans(cloud, seed):
    """The cloud with a tenth of its points set to NaN (an organised cluster keeps its holes)."""
    c = cloud.copy()
    rng = np.random.default_rng(seed)
    c[rng.choice(len(c), len(c) // 10, replace=False)] = np.nan
    return c


def key(r):
    return (r.T.tobytes(), float(r.best_error).hex(), r.best_iteration, r.n_src_keys, r.n_tgt_keys, r.status)


@pytest.fixture(scope="module")
def batch(ctx, model):
    """Model + 4 clusters (the scene at position 1, NaN holes in the last) and the batch's results."""
    ope = load_pkg()
    clouds = raw_candidates(3, scene_at=1) + [with_nans(raw_candidates(4, scene_at=0, seed=3)[3], 11)]
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    res = ctx.coarse_pose_batch(m, cs, ope.default_coarse_params(), seeds=None)
    feats = {w: ctx.coarse_batch_features(w) for w in range(-1, len(clouds))}
    return dict(clouds=clouds, m=m, cs=cs, res=res, feats=feats)


# ------------------------------------------------------------------ stage by stage
def test_stages_match_the_single_path_and_the_oracle(ctx, model, batch):
    for w in range(-1, len(batch["clouds"])):
        cloud = model if w < 0 else batch["clouds"][w]
        idx, nrm, f = batch["feats"][w]
        # uniform sampling: bit-equal indices
        np.testing.assert_array_equal(idx, ctx.uniform_sampling(ctx.upload(cloud), 0.01))
        np.testing.assert_array_equal(idx, oracle.uniform_sampling(cloud, 0.01))
        keys = cloud[idx]
        # normals bit for bit against ope_normals on the same key points, but for rows whose k + 1 nearest hold an exact fp32
        # distance tie (the exclusion test_gpu_features.py uses)
        snrm, _ = ctx.normals(ctx.upload(keys), 30)
        diff = np.flatnonzero((nrm.view(np.uint32) != snrm.view(np.uint32)).any(1))
        if len(diff):
            _, d2, _ = oracle.KdTree(keys).knn(keys[diff], 31)
            tied = (d2[:, 1:] == d2[:, :-1]).any(1)
            assert tied.all() and len(diff) <= 3, (w, diff, tied)
        # FPFH on the batch's own normals: every row within 8e-5 (L1, of 300) of the oracle's
        ref, _, _ = oracle.fpfh(keys, nrm, 0.03)
        l1 = np.abs(f.astype(np.float64) - ref.astype(np.float64)).sum(1)
        assert l1.max() < 8e-5, (w, l1.max())


# ------------------------------------------------------------------ against the oracle composite and the single path
def test_poses_match_the_oracle_composite(batch, model):
    for i, (cloud, r) in enumerate(zip(batch["clouds"], batch["res"])):
        T, info = oracle.estimate_coarse_pose(model, cloud, sacia_seed=1, call_index=i)
        assert r.status == 0, (i, r.status)
        assert r.n_src_keys == info["n_src_keys"] and r.n_tgt_keys == info["n_tgt_keys"], (i, r, info)
        assert r.best_iteration == info["sacia_best"], (i, r.best_iteration, info)
        assert frob(r.T, T) < 2e-5, (i, frob(r.T, T))
        assert abs(r.best_error - info["sacia_error"]) <= 1e-4 * abs(info["sacia_error"]), (i, r.best_error, info)


def test_poses_match_sacia_on_the_batch_features_and_on_the_single_path(ctx, model, batch):
    ope = load_pkg()
    midx, mnrm, mf = batch["feats"][-1]
    mk = model[midx]
    src = ctx.upload(mk)
    # the single path's model features, as the facade computes them
    src1 = ctx.upload(model[ctx.uniform_sampling(ctx.upload(model), 0.01)])
    ctx.normals(src1, 30, fetch=False)
    mf1 = ctx.fpfh(src1, 0.03)
    for i, (cloud, r) in enumerate(zip(batch["clouds"], batch["res"])):
        p = ope.default_sacia_params(seed=1 + i)
        tidx, tnrm, tf = batch["feats"][i]
        tgt = ctx.upload(cloud[tidx])
        T, err, best = ctx.sacia(src, mf, tgt, ctx.build_index(tgt), tf, p)
        assert best == r.best_iteration and T.tobytes() == r.T.tobytes(), (i, best, r.best_iteration, frob(T, r.T))
        # the single path's own features: same draws, descriptors equal to fp32 round-off
        t1 = ctx.upload(cloud[ctx.uniform_sampling(ctx.upload(cloud), 0.01)])
        ctx.normals(t1, 30, fetch=False)
        tf1 = ctx.fpfh(t1, 0.03)
        T1, _, best1 = ctx.sacia(src1, mf1, t1, ctx.build_index(t1), tf1, p)
        assert best1 == r.best_iteration and frob(T1, r.T) < 1e-6, (i, best1, r.best_iteration, frob(T1, r.T))


# ------------------------------------------------------------------ independence and launches
def test_results_do_not_depend_on_the_rest_of_the_batch(ctx, model, batch):
    ope = load_pkg()
    p = ope.default_coarse_params()
    cs, res = batch["cs"], batch["res"]
    seeds = [1 + i for i in range(len(cs))]
    for i, c in enumerate(cs):   # alone
        assert key(ctx.coarse_pose_batch(batch["m"], [c], p, seeds=[seeds[i]])[0]) == key(res[i]), i
    rev = ctx.coarse_pose_batch(batch["m"], cs[::-1], p, seeds=seeds[::-1])   # another position
    assert [key(r) for r in rev[::-1]] == [key(r) for r in res]
    extra = [ctx.upload(c) for c in raw_candidates(60, scene_at=5, seed=9)]   # a batch of 64
    big = ctx.coarse_pose_batch(batch["m"], extra[:20] + cs + extra[20:], p, seeds=list(range(100, 120)) + seeds + list(range(120, 160)))
    assert [key(r) for r in big[20:24]] == [key(r) for r in res]


def test_launches_do_not_depend_on_the_batch_size(ctx, model):
    cs = [ctx.upload(c) for c in raw_candidates(16, scene_at=2)]
    m = ctx.upload(model)
    counts = []
    for k in (2, 16):
        ctx.profile_kernels(True)
        ctx.coarse_pose_batch(m, cs[:k])
        rec = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        counts.append({name: v["launches"] for name, v in rec.items()})
    assert counts[0] == counts[1] and counts[0], counts
    assert all(n == 1 for n in counts[0].values()), counts[0]


# ------------------------------------------------------------------ edge cases
def test_empty_tiny_and_nan_clusters_keep_the_identity_and_their_neighbours(ctx, model, batch):
    ope = load_pkg()
    empty = ctx.upload(np.zeros((0, 3), np.float32))
    tiny = ctx.upload(batch["clouds"][1][:: 200][:9] + np.arange(9, dtype=np.float32)[:, None] * np.float32(0.02))
    nan = ctx.upload(np.full((100, 3), np.nan, np.float32))
    cs = batch["cs"]
    mixed = [empty, cs[0], tiny, cs[1], nan, cs[2], cs[3]]
    seeds = [50, 1, 51, 2, 52, 3, 4]
    res = ctx.coarse_pose_batch(batch["m"], mixed, seeds=seeds)
    I = np.eye(4, dtype=np.float32)
    assert res[0].status == ope.COARSE_EMPTY_TARGET and res[0].n_tgt_keys == 0
    assert res[2].status == ope.COARSE_FEW_TARGET_FEATURES and res[2].n_tgt_keys == 9
    assert res[4].status == ope.COARSE_FEW_TARGET_FEATURES and res[4].n_tgt_keys == 0
    for j in (0, 2, 4):
        assert np.array_equal(res[j].T, I) and res[j].best_iteration == -1, j
    assert [key(r) for r in (res[1], res[3], res[5], res[6])] == [key(r) for r in batch["res"]]
    assert len(ctx.coarse_batch_features(0)[0]) == 0 and len(ctx.coarse_batch_features(4)[0]) == 0


def test_empty_batch_is_a_no_op(ctx, model):
    assert ctx.coarse_pose_batch(ctx.upload(model), []) == []


def test_a_batch_of_256(ctx, model, batch):
    rng = np.random.default_rng(5)
    base = batch["clouds"]
    clouds = []
    for j in range(256):
        c = base[j % len(base)]
        clouds.append(c[rng.choice(len(c), len(c) * 3 // 4, replace=False)])   # 3/4 of a cluster's points
    cs = [ctx.upload(c) for c in clouds]
    res = ctx.coarse_pose_batch(batch["m"], cs, seeds=list(range(1000, 1256)))
    assert len(res) == 256 and all(r.status == 0 for r in res)
    for j in (0, 77, 255):
        assert key(ctx.coarse_pose_batch(batch["m"], [cs[j]], seeds=[1000 + j])[0]) == key(res[j]), j
        T, info = oracle.estimate_coarse_pose(model, clouds[j], sacia_seed=1000 + j, call_index=0)
        assert res[j].best_iteration == info["sacia_best"] and frob(res[j].T, T) < 2e-5, j


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(ctx, model, batch):
    ope = load_pkg()
    m, c = batch["m"], batch["cs"][1]
    few = ctx.upload(model[:: 600][:3])                         # a model with fewer key points than nr_samples
    big = ctx.upload(np.random.default_rng(0).uniform(-1, 1, (65537, 3)).astype(np.float32))
    g = np.stack(np.meshgrid(np.arange(70), np.arange(70), [0.0], indexing="ij"), -1).reshape(-1, 3)
    many_keys = ctx.upload((g * 0.012).astype(np.float32))      # 4 900 points, 4 900 key points
    bad = [
        (few, [c], {}),
        (m, [c], dict(normals_k=0)),
        (m, [c], dict(normals_k=33)),
        (m, [c], dict(sacia=ope.default_sacia_params(k_correspondences=0))),
        (m, [c], dict(sacia=ope.default_sacia_params(k_correspondences=9))),
        (m, [c], dict(key_leaf=0.0)),
        (m, [c], dict(fpfh_radius=-0.03)),
        (m, [c, big], {}),
        (big, [c], {}),
        (m, [many_keys, c], {}),
    ]
    for mm, cc, kw in bad:
        with pytest.raises(ope.OpeError) as ei:
            ctx.coarse_pose_batch(mm, cc, ope.default_coarse_params(**kw))
        assert ei.value.code == ope.OPE_EINVAL, kw
        r = ctx.coarse_pose_batch(m, [c], seeds=[2])[0]
        assert key(r) == key(batch["res"][1]), kw


# ------------------------------------------------------------------ the candidate loop at C1 size
FINE = dict(max_iterations=100, transformation_epsilon=1e-8, euclidean_fitness_epsilon=1e-8, corr_mode=1, k_normal_shooting=20,
            use_surface_normal_rej=1, surface_normal_thr=0.7)   # estimateFinePose (poseestimator.cpp:242-337)


def fine_inputs(ctx, cloud):
    """NaN removal, UniformSampling(0.008), normals k = 30, NaN normals dropped (the fine stage's inputs)."""
    cloud = cloud[np.isfinite(cloud).all(1)]
    keys = cloud[ctx.uniform_sampling(ctx.upload(cloud), 0.008)]
    nrm, _ = ctx.normals(ctx.upload(keys), 30)
    ok = np.isfinite(nrm).all(1)
    return keys[ok], nrm[ok]


def test_candidate_loop_at_c1_size_matches_the_sequential_loop(ctx, model):
    ope = load_pkg()
    clouds = raw_candidates(8, scene_at=3)
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    p = ope.default_icp_params(**FINE)

    def accept(fit, strength):   # rosinterface.cpp:256
        return fit < 1e-4 or strength > 0.4

    # batched: coarse stage, fine inputs per candidate, icp_batch, the selection rule
    coarse = ctx.coarse_pose_batch(m, cs)
    assert all(r.status == 0 for r in coarse)
    src = [ctx.upload(*fine_inputs(ctx, apply(r.T, model))) for r in coarse]
    ix = [ctx.build_index(ctx.upload(*fine_inputs(ctx, c))) for c in clouds]
    res = ctx.icp_batch(src, ix, p, None, fitness_max_range=DBL_MAX)
    sel = next((j for j, r in enumerate(res) if accept(r.fitness, r.align_strength)), None)

    # sequential: the single-path coarse chain per candidate, ctx.icp and ctx.fitness, until accept
    mk = ctx.upload(model[ctx.uniform_sampling(ctx.upload(model), 0.01)])
    ctx.normals(mk, 30, fetch=False)
    mf = ctx.fpfh(mk, 0.03)
    seq = None
    for j, c in enumerate(clouds):
        t = ctx.upload(c[ctx.uniform_sampling(ctx.upload(c), 0.01)])
        ctx.normals(t, 30, fetch=False)
        T, _, best = ctx.sacia(mk, mf, t, ctx.build_index(t), ctx.fpfh(t, 0.03), ope.default_sacia_params(seed=1 + j))
        assert best == coarse[j].best_iteration and frob(T, coarse[j].T) < 1e-6, j
        # fine inputs from the batch's coarse pose (within 1e-6 of T, above): identical inputs on both sides
        one = ctx.icp(src[j], ix[j], p)
        fit = ctx.fitness(src[j], ix[j], one.T)[0]
        if accept(fit, one.align_strength):
            seq = (j, one)
            break
    print("[coarse batch c1] candidate", sel, [(round(r.fitness, 7), round(r.align_strength, 3)) for r in res])
    assert seq is not None and sel == seq[0], (sel, seq and seq[0])
    assert frob(res[sel].T, seq[1].T) < 1e-6
