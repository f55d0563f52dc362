"""Batched final pose (ope_final_pose_batch, final_batch.hip): the reference's first-frame candidate loop
(rosinterface.cpp:243-262), estimateFinalPose of one model against many clusters in one call.

Stage by stage against the single-call chain (float32 transform, uniform_sampling, normals, NaN drop, upload, build_index,
icp_batch) and the oracle; the loop's rules (skipped clusters, seeds, statuses, the selected cluster) against an explicit
sequential loop; byte-reproducible whatever else is in the batch; the same launches for any batch size; edge cases and refusals.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(ROOT, "tests", "golden")
DBL_MAX = float(np.finfo(np.float64).max)
FINE = dict(max_iterations=100, transformation_epsilon=1e-8, euclidean_fitness_epsilon=1e-8, corr_mode=1, k_normal_shooting=20,
            use_surface_normal_rej=1, surface_normal_thr=0.7)   # estimateFinePose (poseestimator.cpp:242-337)


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


def frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


def raw_candidates(k, scene_at, seed=0):
    """K raw candidate clusters, as test_gpu_coarse_batch.raw_candidates builds them: the C1 scene cluster at position scene_at,
    rigidly moved copies of it and synth distractors near the object."""
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


def transform_f32(T, p):
    """pcl::transformPointCloud in float32, operation by operation: m0*x + m4*y + m8*z + m12; non-finite points left alone."""
    M = np.asarray(T, np.float32)
    out = p.copy()
    fin = np.isfinite(p).all(1)
    x, y, z = p[fin, 0], p[fin, 1], p[fin, 2]
    for r in range(3):
        out[fin, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    return out


def chain(ctx, cloud):
    """The fine stage's preparation one call at a time: NaN removal, UniformSampling(0.008), normals k = 30, NaN normals dropped."""
    cloud = cloud[np.isfinite(cloud).all(1)]
    if len(cloud) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    keys = cloud[ctx.uniform_sampling(ctx.upload(cloud), 0.008)]
    nrm, _ = ctx.normals(ctx.upload(keys), 30)
    ok = np.isfinite(nrm).all(1)
    return keys[ok], nrm[ok]


def ckey(r):
    return (r.T.tobytes(), float(r.best_error).hex(), r.best_iteration, r.n_src_keys, r.n_tgt_keys, r.status)


def fkey(o):
    f = o.fine
    fk = None if f is None else (f.T.tobytes(), f.iterations, f.converged, f.state, float(f.last_mse).hex(), f.n_corr,
                                 float(f.align_strength).hex(), float(f.fitness).hex(), f.fitness_n)
    return (ckey(o.coarse), o.seed, fk, o.n_fine_src, o.n_fine_tgt, o.status, o.accepted)


def same_normals_but_ties(a, b, keys):
    """Normals bit for bit, but for rows whose k + 1 nearest hold an exact fp32 distance tie (test_gpu_features.py's exclusion)."""
    diff = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))
    if len(diff):
        _, d2, _ = oracle.KdTree(keys).knn(keys[diff], 31)
        assert (d2[:, 1:] == d2[:, :-1]).any(1).all() and len(diff) <= 3, diff


@pytest.fixture(scope="module")
def c1(ctx, model):
    """C1 size, 8 clusters, the scene at position 3."""
    clouds = raw_candidates(8, scene_at=3)
    m = ctx.upload(model)
    cs = [ctx.upload(c) for c in clouds]
    res, sel = ctx.final_pose_batch(m, cs)
    inputs = [(ctx.final_batch_inputs(i, 0), ctx.final_batch_inputs(i, 1)) for i in range(len(cs))]
    return dict(clouds=clouds, m=m, cs=cs, res=res, sel=sel, inputs=inputs)


# ------------------------------------------------------------------ stage by stage
def test_coarse_stage_is_the_coarse_batch_with_the_loops_seeds(ctx, c1):
    ref = ctx.coarse_pose_batch(c1["m"], c1["cs"], seeds=[1 + i for i in range(8)])
    assert [o.seed for o in c1["res"]] == [1 + i for i in range(8)]
    assert [ckey(o.coarse) for o in c1["res"]] == [ckey(r) for r in ref]


def test_fine_inputs_equal_the_single_call_chain(ctx, model, c1):
    for i, o in enumerate(c1["res"]):
        assert o.status == 0, (i, o.status)
        for side, cloud in ((0, transform_f32(o.coarse.T, model)), (1, c1["clouds"][i])):
            xyz, nrm = c1["inputs"][i][side]
            rx, rn = chain(ctx, cloud)
            assert xyz.tobytes() == rx.tobytes(), (i, side)
            same_normals_but_ties(nrm, rn, xyz)
        assert (o.n_fine_src, o.n_fine_tgt) == (len(c1["inputs"][i][0][0]), len(c1["inputs"][i][1][0]))


def test_fine_icp_equals_icp_batch_on_the_uploads(ctx, c1):
    ope = load_pkg()
    src = [ctx.upload(*c1["inputs"][i][0]) for i in range(8)]
    ix = [ctx.build_index(ctx.upload(*c1["inputs"][i][1])) for i in range(8)]
    ref = ctx.icp_batch(src, ix, ope.default_icp_params(**FINE), None, fitness_max_range=DBL_MAX)
    for i, (o, r) in enumerate(zip(c1["res"], ref)):
        f = o.fine
        assert f.T.tobytes() == r.T.tobytes(), (i, frob(f.T, r.T))
        assert (f.iterations, f.converged, f.state, f.n_corr, f.fitness_n) == (r.iterations, r.converged, r.state, r.n_corr, r.fitness_n), i
        assert float(f.fitness).hex() == float(r.fitness).hex() and float(f.align_strength).hex() == float(r.align_strength).hex(), i
        assert o.accepted == (r.fitness < 1e-4 or r.align_strength > 0.4), i
    acc = [i for i, r in enumerate(ref) if r.fitness < 1e-4 or r.align_strength > 0.4]
    assert c1["sel"] == (acc[0] if acc else -1)
    print("[final batch c1] selected", c1["sel"], [(round(o.fine.fitness, 7), round(o.fine.align_strength, 3)) for o in c1["res"]])


def test_selected_fine_pose_matches_the_oracle(ctx, c1):
    sel = c1["sel"]
    assert sel == 3, sel   # the scene cluster
    (sk, sn), (tk, tn) = c1["inputs"][sel]
    p = oracle.default_icp_params()
    p.acc_mode = 1
    p.transform_mode = 1
    for k, v in FINE.items():
        setattr(p, k, v)
    ref = oracle.icp(sk, tk, p, src_nrm=sn, tgt_nrm=tn)
    f = c1["res"][sel].fine
    assert frob(f.T, ref.T) < 1e-4 and f.iterations == ref.iterations, (frob(f.T, ref.T), f.iterations, ref.iterations)


# ------------------------------------------------------------------ the loop's rules
def test_skipped_clusters_use_no_seed_and_the_selection_follows_the_sequential_loop(ctx, model, c1):
    ope = load_pkg()
    scene = c1["clouds"][3]
    empty = np.zeros((0, 3), np.float32)
    nan = np.full((100, 3), np.nan, np.float32)
    tiny = scene[::200][:9] + np.arange(9, dtype=np.float32)[:, None] * np.float32(0.02)   # 9 coarse key points
    sparse = scene[ctx.uniform_sampling(ctx.upload(scene), 0.01)][:60]                    # >= 10 coarse keys, < 100 fine points
    clouds = [c1["clouds"][0], empty, nan, tiny, sparse, scene, c1["clouds"][1]]
    cs = [ctx.upload(c) for c in clouds]
    res, sel = ctx.final_pose_batch(c1["m"], cs)
    assert [o.status for o in res[:6]] == [ope.FINAL_OK, ope.FINAL_EMPTY_TARGET, ope.FINAL_FEW_FINE_POINTS,
                                           ope.FINAL_FEW_FINE_POINTS if res[3].n_fine_tgt < 100 else ope.FINAL_FEW_TARGET_FEATURES,
                                           ope.FINAL_FEW_FINE_POINTS, ope.FINAL_OK], [o.status for o in res]
    assert res[3].coarse.status == ope.COARSE_FEW_TARGET_FEATURES and res[4].coarse.status == ope.COARSE_OK
    # the explicit loop: a seed per SAC-IA call, in order; fine stage per non-empty cluster; stop at the first accepted
    seed, want_sel = 1, -1
    for i, c in enumerate(clouds):
        o = res[i]
        if len(c) == 0:
            assert o.seed == 0 and o.fine is None
            continue
        coarse = ctx.coarse_pose_batch(c1["m"], [cs[i]], seeds=[seed])[0]
        if coarse.status == ope.COARSE_OK:
            assert o.seed == seed, i
            seed += 1
        else:
            assert o.seed == 0, i
        assert ckey(o.coarse) == ckey(coarse), i
        T = coarse.T if coarse.status == ope.COARSE_OK else np.eye(4, dtype=np.float32)
        (sk, sn), (tk, tn) = chain(ctx, transform_f32(T, model)), chain(ctx, c)
        assert o.n_fine_tgt == len(tk) and o.n_fine_src == len(sk), i
        if len(tk) < 100:
            assert o.status == ope.FINAL_FEW_FINE_POINTS and o.fine is None and not o.accepted, i
            continue
        r = ctx.icp_batch([ctx.upload(*ctx.final_batch_inputs(i, 0))], [ctx.build_index(ctx.upload(*ctx.final_batch_inputs(i, 1)))],
                          ope.default_icp_params(**FINE), None, fitness_max_range=DBL_MAX)[0]
        assert o.fine.T.tobytes() == r.T.tobytes(), i
        if want_sel < 0 and (r.fitness < 1e-4 or r.align_strength > 0.4):
            want_sel = i
    assert sel == want_sel == 5, (sel, want_sel)


def test_few_target_features_runs_the_fine_icp_from_the_unmoved_model(ctx, model, c1):
    """< 10 coarse key points leave the coarse pose at the identity; with min_fine_points lowered the fine ICP still runs, from the
    model as it is (estimateCoarsePose :40-45 keeps alignedSource = source), and uses up no seed."""
    ope = load_pkg()
    scene = c1["clouds"][3]
    tiny = scene[::60][:9] + np.arange(9, dtype=np.float32)[:, None] * np.float32(0.02)   # 9 coarse key points, 9 fine
    clouds = [tiny, scene]
    cs = [ctx.upload(c) for c in clouds]
    p = ope.default_final_params(min_fine_points=5)
    res, sel = ctx.final_pose_batch(c1["m"], cs, p)
    o = res[0]
    assert o.coarse.status == ope.COARSE_FEW_TARGET_FEATURES and o.status == ope.FINAL_FEW_TARGET_FEATURES and o.seed == 0
    assert np.array_equal(o.coarse.T, np.eye(4, dtype=np.float32)) and o.fine is not None
    assert res[1].seed == 1 and res[1].status == ope.FINAL_OK   # the scene draws the first seed
    # the sequential loop's fine stage for the tiny cluster: the unmoved model and the cluster, through the single calls
    (sk, sn), (tk, tn) = chain(ctx, model), chain(ctx, tiny)
    xyz0, _ = ctx.final_batch_inputs(0, 0)
    xyz1, _ = ctx.final_batch_inputs(0, 1)
    assert xyz0.tobytes() == sk.tobytes() and xyz1.tobytes() == tk.tobytes() and o.n_fine_tgt == len(tk) == 9
    r = ctx.icp_batch([ctx.upload(*ctx.final_batch_inputs(0, 0))], [ctx.build_index(ctx.upload(*ctx.final_batch_inputs(0, 1)))],
                      ope.default_icp_params(**FINE), None, fitness_max_range=DBL_MAX)[0]
    assert o.fine.T.tobytes() == r.T.tobytes() and o.fine.iterations == r.iterations
    assert float(o.fine.fitness).hex() == float(r.fitness).hex() and float(o.fine.align_strength).hex() == float(r.align_strength).hex()
    assert o.accepted == (r.fitness < 1e-4 or r.align_strength > 0.4)
    assert sel == (0 if o.accepted else 1 if res[1].accepted else -1)


def test_a_fine_target_of_more_than_2048_points_is_indexed_as_build_index_does(ctx, model, c1):
    """2 049..4 096 fine target points: build_bvh_device sorts level 0 device-wide and the rest from L0 = 1, the batch sorts all
    levels in one block; the ICP results must still be byte-equal."""
    ope = load_pkg()
    g = np.stack(np.meshgrid(np.arange(58), np.arange(58), indexing="ij"), -1).reshape(-1, 2).astype(np.float64) * 0.009
    z = 0.02 * np.sin(g[:, 0] * 25.0) * np.cos(g[:, 1] * 19.0)
    c0 = c1["clouds"][3].mean(0)
    big = (np.column_stack([g - g.mean(0), z]) + c0).astype(np.float32)
    cs = [ctx.upload(big), c1["cs"][3]]
    res, _ = ctx.final_pose_batch(c1["m"], cs)
    assert 2048 < res[0].n_fine_tgt <= ope.COARSE_MAX_KEYS, res[0].n_fine_tgt
    src = [ctx.upload(*ctx.final_batch_inputs(i, 0)) for i in range(2)]
    ix = [ctx.build_index(ctx.upload(*ctx.final_batch_inputs(i, 1))) for i in range(2)]
    ref = ctx.icp_batch(src, ix, ope.default_icp_params(**FINE), None, fitness_max_range=DBL_MAX)
    for i in range(2):
        f, r = res[i].fine, ref[i]
        assert f.T.tobytes() == r.T.tobytes() and (f.iterations, f.n_corr, f.fitness_n) == (r.iterations, r.n_corr, r.fitness_n), i
        assert float(f.fitness).hex() == float(r.fitness).hex() and float(f.align_strength).hex() == float(r.align_strength).hex(), i
    xyz, _ = ctx.final_batch_inputs(0, 1)
    assert xyz.tobytes() == chain(ctx, big)[0].tobytes()


# ------------------------------------------------------------------ the C++ façade and the driver
EXE = os.path.join(ROOT, "object-pose-estimation_amd", "build", "detect_and_localize")


def _driver(model_path, cluster_paths, flag):
    r = subprocess.run([EXE, model_path, *cluster_paths, "--seed", "1", flag], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cand = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("candidates ")]
    frames = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert len(cand) == 1 and len(frames) == 1, r.stdout
    tok = frames[0]
    rec = {"selected": int(cand[0][2]), "fitness": float(tok[3]), "strength": float(tok[5]), "coarse_calls": int(tok[7]),
           "icp_iterations": int(tok[9])}
    i = 10
    for name in ("final", "coarse", "fine", "rigid"):
        assert tok[i] == name
        rec[name] = np.array([float(v) for v in tok[i + 1:i + 17]]).reshape(4, 4).T
        i += 17
    aligned = [ln.split(None, 1)[1] for ln in r.stdout.splitlines() if ln.startswith("aligned ")][0]
    rec["aligned"] = pcd.read_pcd(aligned)[0]
    return rec


@pytest.mark.parametrize("layout", ["scene_fourth", "none_accepted"])
def test_driver_candidates_matches_the_loop_of_estimate_final_pose(tmp_path, model, c1, layout):
    if not os.path.exists(EXE):
        import __graft_entry__ as g
        g.build()
    clouds = raw_candidates(8, scene_at=3)
    scene = clouds[3]
    tiny = scene[::200][:9] + np.arange(9, dtype=np.float32)[:, None] * np.float32(0.02)
    if layout == "scene_fourth":
        clouds = [clouds[0], tiny, clouds[1], clouds[3], clouds[4]]       # a skipped coarse stage before the accepted cluster
    else:
        clouds = [clouds[2], tiny, clouds[4]]                             # nothing accepted: the state after the last cluster
    mp = str(tmp_path / "model.pcd")
    pcd.write_pcd(mp, model)
    paths = []
    for j, c in enumerate(clouds):
        paths.append(str(tmp_path / f"cluster{j}.pcd"))
        pcd.write_pcd(paths[-1], c)
    one = _driver(mp, paths, "--candidates")
    loop = _driver(mp, paths, "--candidates-loop")
    print("[final batch driver]", layout, one["selected"], one["fitness"], one["strength"], one["coarse_calls"], one["icp_iterations"])
    assert one["selected"] == loop["selected"] == (3 if layout == "scene_fourth" else -1)
    assert one["coarse_calls"] == loop["coarse_calls"] and one["icp_iterations"] == loop["icp_iterations"]
    assert abs(one["fitness"] - loop["fitness"]) <= 1e-6 * abs(loop["fitness"])
    assert abs(one["strength"] - loop["strength"]) <= 1e-9
    for name in ("final", "coarse", "fine", "rigid"):
        assert frob(one[name], loop[name]) < 1e-4, (name, frob(one[name], loop[name]))
    assert one["aligned"].shape == loop["aligned"].shape and np.abs(one["aligned"] - loop["aligned"]).max() < 1e-4


# ------------------------------------------------------------------ independence and launches
def test_results_do_not_depend_on_the_rest_of_the_batch(ctx, c1):
    cs, res = c1["cs"], c1["res"]
    seeds = [1 + i for i in range(len(cs))]
    for i in (0, 3, 7):   # alone
        r, _ = ctx.final_pose_batch(c1["m"], [cs[i]], seeds=[seeds[i]])
        assert fkey(r[0]) == fkey(res[i]), i
    rev, _ = ctx.final_pose_batch(c1["m"], cs[::-1], seeds=seeds[::-1])   # another position
    assert [fkey(r) for r in rev[::-1]] == [fkey(r) for r in res]
    extra = [ctx.upload(c) for c in raw_candidates(56, scene_at=5, seed=9)]   # a batch of 64
    big, _ = ctx.final_pose_batch(c1["m"], extra[:20] + cs + extra[20:], seeds=list(range(100, 120)) + seeds + list(range(120, 156)))
    assert [fkey(r) for r in big[20:28]] == [fkey(r) for r in res]


def test_launches_do_not_depend_on_the_batch_size(ctx, model, c1):
    cs = c1["cs"] * 2
    counts = []
    for k in (2, 16):
        ctx.profile_kernels(True)
        ctx.final_pose_batch(c1["m"], cs[:k])
        rec = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        counts.append({name: v["launches"] for name, v in rec.items()})
    assert counts[0] == counts[1] and counts[0], counts
    for name in ("fine_transform_kernel", "fine_order_kernel", "bvh_batch_order_kernel", "bvh_batch_root_kernel"):
        assert counts[0][name] == 1, (name, counts[0])


# ------------------------------------------------------------------ edge cases and refusals
def test_empty_batch_is_a_no_op(ctx, model):
    assert ctx.final_pose_batch(ctx.upload(model), []) == ([], -1)


def test_refusals_leave_the_context_usable(ctx, model, c1):
    ope = load_pkg()
    m, c = c1["m"], c1["cs"][3]
    want = fkey(c1["res"][3])
    g = np.stack(np.meshgrid(np.arange(70), np.arange(70), [0.0], indexing="ij"), -1).reshape(-1, 3)
    grid = (g * 0.009).astype(np.float32)   # <= 4096 key points at 1 cm, 4 900 at 8 mm: refused only after sampling
    assert len(oracle.uniform_sampling(grid, 0.01)) <= ope.COARSE_MAX_KEYS < len(oracle.uniform_sampling(grid, 0.008))
    grid_c = ctx.upload(grid)
    bad = [
        (m, [c], dict(fine_leaf=0.0), "fine_leaf must be > 0"),
        (m, [c], dict(fine_normals_k=0), "1 <= fine_normals_k <= 32"),
        (m, [c], dict(fine_normals_k=33), "1 <= fine_normals_k <= 32"),
        (m, [c], dict(icp=ope.default_icp_params(**FINE, use_reciprocal=1)), "reciprocal correspondences are not supported"),
        (m, [c], dict(icp=ope.default_icp_params(**FINE, estimator=ope.EST_POINT_TO_PLANE_LM)), "the LM estimator is not supported"),
        (m, [c], dict(coarse=ope.default_coarse_params(normals_k=0)), "ope_coarse_pose_batch: 1 <= normals_k <= 32"),
        # a cluster with too many fine key points: counted before anything is launched
        (m, [grid_c, c], {}, "more than OPE_COARSE_MAX_KEYS fine key points (cluster 0)"),
        # the moved model: found after sampling
        (grid_c, [c], {}, "more than OPE_COARSE_MAX_KEYS fine key points (the model moved for cluster 0)"),
    ]
    for mm, cc, kw, msg in bad:
        with pytest.raises(ope.OpeError) as ei:
            ctx.final_pose_batch(mm, cc, ope.default_final_params(**kw), seeds=[4] * len(cc))
        assert ei.value.code == ope.OPE_EINVAL and msg in str(ei.value), (kw, str(ei.value))
        with pytest.raises(ope.OpeError):   # a refused call leaves no fine inputs behind
            ctx.final_batch_inputs(0, 0)
        r, sel = ctx.final_pose_batch(m, [c], seeds=[4])
        assert fkey(r[0]) == want and sel == 0, kw
