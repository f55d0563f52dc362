"""FPFH on the device against the fp64 reference (fpfh_ref.py) where the kernels can go wrong: a neighbour at exactly d^2 == r^2,
duplicate points, NaN normals and points, a thousand neighbours, a cluster of exactly OPE_COARSE_MAX_KEYS key points, and the
stages that feed it (key points under exact ties, normals of degenerate neighbourhoods).

Both sets of kernels: spfh_kernel / fpfh_kernel (ope_fpfh: tree walk, 32-bit LDS counters, sums in tree order) and
coarse_spfh_kernel / coarse_fpfh_kernel (ope_coarse_pose_batch: the segment in LDS, 16-bit counters, sums in slot order).  The cases,
the bound and the assert are fpfh_cases.py's; test_fpfh_ref.py passes the C oracle through the same assert on the CPU.

The batch path cannot see duplicate points: its uniform sampling keeps one point per voxel, and duplicates share a voxel.  The
dups_* cases therefore run on the single path only.
"""
import numpy as np
import pytest

import oracle
from conftest import load_pkg
from fpfh_cases import (CASE_NAMES, H7, L1_BOUND, MAX_KEYS, TIE_LEAF, cases, compare, lattice_4096, plane_lattice, reference,
                        tie_voxel_cloud)
from fpfh_ref import fpfh_ref, undefined_rows
from test_oracle_independent import uniform_sampling_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    ope = load_pkg()
    c = ope.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ single path
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fpfh_against_the_fp64_reference(ctx, name):
    c = cases()[name]
    ref, _, _, fragile = reference(name)
    cloud = ctx.upload(c.P, c.N)
    if name == "line":
        # the chain a thin cluster really takes: the device's own normals, all NaN, stay attached to the cloud
        nrm, _ = ctx.normals(cloud, 30)
        assert np.isnan(nrm).all()
    out = ctx.fpfh(cloud, c.r)
    # bound: fpfh_cases.L1_BOUND (1e-3; dense_lattice 1.16e-3), from the oracle's own distance to the reference, at most a quarter
    # of it in every case; fragile rows exempt up to 10 %, none in the exact cases.  Measured, max L1 of the oracle
    # over all rows / fragile share / max L1 of this call over the rows that count:
    #   surface_r020 6.9e-5 / 7.3 % / 7.6e-5    surface_r012 5.2e-5 / 0.9 % / 5.4e-5    random_normals 4.7e-5 / 0 / 4.8e-5
    #   dups_same 8.0e-5 / 7.5 % / 9.0e-5       dups_other 9.7e-5 / 7.5 % / 9.3e-5      sphere 7.4e-5 / 0 / 6.7e-5
    #   nan_normals 7.2e-5 / 7.3 % / 7.6e-5     nan_point_isolated 1.1e-4 / 11.4 % (none exempt) / 1.0e-4
    #   lattice_tie 2.9e-5 / 0 / 2.7e-5         lattice_4096 4.0e-5 / 0 / 3.8e-5        line 2.3e-5 / 0 / 2.3e-5
    #   dense_ball 2.4e-4 / 0 / 2.3e-4          dense_lattice 2.9e-4 / 0 / 2.9e-4
    compare(out, ref, fragile, c.exact, "ope_fpfh " + name, c.bound)


# ------------------------------------------------------------------ batched path
BATCH_R = 3 * H7      # lattice_tie: neighbours at exactly d^2 == 9 h^2; line: its own radius; the dense cases: every point in range
H12 = 2.0 ** -12      # a key leaf under which every lattice point, and all but a few points of dense_ball, keep their own voxel


def batch_compare(ctx, clouds, exact, r, label):
    """Every segment of the last coarse_pose_batch (clouds[0] is the model) against fpfh_ref on its key points and the normals
    the batch returned, under fpfh_cases.compare: {which: (idx, normals, fpfh, m)}.

    The bound follows the rule of fpfh_cases.py for normals that no CPU test has seen: 1e-3 while the oracle is within a quarter
    of it on these inputs, 4 x the oracle's own maximum otherwise, and the oracle no further than 5e-4 at all.

    The batch computes its normals itself, and the k-NN normals of a lattice are parallel, perpendicular and mirror images of one
    another: such pairs sit exactly on the swap test and on atan2(0, 0), and no reference decides them, in fp64 or in fp32
    (fpfh_ref.undefined_rows).  The rows that see one are compared with ope_fpfh on the same key points and normals instead:
    the single path shares the pair arithmetic (feature_math.hpp) and is itself held to the reference above, so what this leaves
    under test is the batch's own part: the neighbourhoods with their ties, the 16-bit counters, the order of the sums."""
    seen = {}
    for w, (cloud, ex) in enumerate(zip(clouds, exact), start=-1):
        idx, nrm, f = ctx.coarse_batch_features(w)
        keys = np.ascontiguousarray(cloud[idx])
        ref, _, m, fragile = fpfh_ref(keys, nrm, r, exact=ex)
        undefined = undefined_rows(keys, nrm, r)
        o_l1 = np.abs(oracle.fpfh(keys, nrm, r)[0].astype(np.float64) - ref).sum(1)[~undefined]
        o_max = float(np.nanmax(o_l1)) if len(o_l1) else 0.0
        bound = L1_BOUND if o_max <= L1_BOUND / 4 else 4 * o_max
        print(f"[fpfh edges] {label} segment {w}: {len(idx)} key points, m {m.min()}..{m.max()}, undefined rows {int(undefined.sum())}, "
              f"oracle max L1 {o_max:.3e}")
        assert o_max <= 5e-4, (label, w, o_max)
        compare(f, ref, fragile, ex, f"{label} segment {w}", bound, skip=undefined)
        if undefined.any():
            single = ctx.fpfh(ctx.upload(keys, nrm), r)
            l1 = np.abs(f.astype(np.float64) - single.astype(np.float64)).sum(1)[undefined]
            print(f"[fpfh edges] {label} segment {w}: max L1 from ope_fpfh over the undefined rows {np.nanmax(l1):.3e}")
            assert np.nanmax(l1) < bound, (label, w, np.nanmax(l1))
        seen[w] = (idx, nrm, f, m)
    return seen


def test_batch_against_the_fp64_reference(ctx):
    """surface (the model), lattice_tie, dense_lattice, line and dense_ball in one batch: one key leaf, 2^-12, under which every
    lattice point keeps its own voxel, and one radius for all."""
    ope = load_pkg()
    cs = cases()
    names = ("surface_r020", "lattice_tie", "dense_lattice", "line", "dense_ball")
    clouds = [np.ascontiguousarray(cs[n].P) for n in names]
    p = ope.default_coarse_params(key_leaf=H12, fpfh_radius=BATCH_R, normals_k=30, sacia=ope.default_sacia_params(max_iterations=4))
    res = ctx.coarse_pose_batch(ctx.upload(clouds[0]), [ctx.upload(c) for c in clouds[1:]], p)
    assert [r.status for r in res] == [0, 0, 0, 0]
    seen = batch_compare(ctx, clouds, (False, True, True, True, False), BATCH_R, "batch")
    for w, n in ((0, 432), (1, 1024), (2, 40)):
        np.testing.assert_array_equal(np.sort(seen[w][0]), np.arange(n))           # every lattice point is a key point
    assert seen[0][3].max() > 70 and (seen[1][3] == 1024).all()
    assert np.isnan(seen[2][1]).all()                                              # line: NaN normals on this path too
    assert len(seen[3][0]) > 1000 and (seen[3][3] == len(seen[3][0])).all()        # dense_ball: counts near 1000 in 16-bit counters,
    assert not undefined_rows(clouds[4][seen[3][0]], seen[3][1], BATCH_R).any()    # and every row judged by the fp64 reference
    assert len(seen[-1][0]) > 1100 and np.isfinite(seen[-1][1]).all()


def test_batch_accepts_exactly_the_key_point_cap(ctx):
    """lattice_4096 as the model and as a cluster: 2 x 4096 float4 and the histograms in LDS.  One more point in a new voxel is
    refused, as a cluster and as the model."""
    ope = load_pkg()
    big, surface = lattice_4096(), np.ascontiguousarray(cases()["surface_r020"].P)
    p = ope.default_coarse_params(key_leaf=H7, fpfh_radius=BATCH_R, normals_k=30, sacia=ope.default_sacia_params(max_iterations=4))
    m = ctx.upload(big)
    res = ctx.coarse_pose_batch(m, [ctx.upload(big), ctx.upload(surface)], p)
    assert [r.status for r in res] == [0, 0] and res[0].n_src_keys == MAX_KEYS and res[0].n_tgt_keys == MAX_KEYS
    got = batch_compare(ctx, [big, big, surface], (True, True, False), BATCH_R, "cap")
    for w in (-1, 0):
        idx, nrm, f, _ = got[w]
        np.testing.assert_array_equal(np.sort(idx), np.arange(MAX_KEYS))
        np.testing.assert_array_equal(nrm, np.tile(np.float32([0, 0, -1]), (MAX_KEYS, 1)))
        # a plane with one normal: every pair has f1 = f2 = f3 = 0, the middle bin of each group
        expect = np.zeros(33, np.float32); expect[[5, 16, 27]] = 100.0
        np.testing.assert_allclose(f, np.tile(expect, (MAX_KEYS, 1)), atol=1e-3, rtol=0)
    np.testing.assert_array_equal(got[-1][2], got[0][2])
    more = ctx.upload(np.r_[big, np.float32([[40 * H7, 0, 0.5]])])
    for mm, cc in ((m, [more]), (more, [m])):
        with pytest.raises(ope.OpeError, match="more than OPE_COARSE_MAX_KEYS key points") as e:
            ctx.coarse_pose_batch(mm, cc, p)
        assert e.value.code == ope.OPE_EINVAL


# ------------------------------------------------------------------ key points under ties
@pytest.mark.parametrize("late_winner", [False, True])
def test_key_points_keep_the_lowest_index_among_exact_ties(ctx, late_winner):
    ope = load_pkg()
    P = tie_voxel_cloud(late_winner)
    want = uniform_sampling_dict(P, TIE_LEAF)
    assert (903 if late_winner else 102) in want
    np.testing.assert_array_equal(ctx.uniform_sampling(ctx.upload(P), TIE_LEAF), want)
    model = ctx.upload(np.ascontiguousarray(cases()["surface_r020"].P))
    ctx.coarse_pose_batch(model, [ctx.upload(P)], ope.default_coarse_params(key_leaf=TIE_LEAF, sacia=ope.default_sacia_params(max_iterations=4)))
    np.testing.assert_array_equal(ctx.coarse_batch_features(0)[0], want)


# ------------------------------------------------------------------ the contexts these tests come after
def test_small_uploads_after_a_context_of_the_same_thread_is_gone():
    """Small host-to-device copies go through a ring of 16 pinned slots that belongs to the thread, each guarded by an event that
    was recorded on the stream of the context that used it last.  Contexts come and go on one thread (every module of this suite
    has its own), and a later context comes round to slots whose stream has been destroyed: it must not wait through those events
    (the runtime's event still points at the stream; seen as "operation not permitted on an event last recorded in a capturing
    stream" from ope_depth_to_cloud, by the layout of the heap).  Three contexts in turn, 20 small copies each, the right answer."""
    ope = load_pkg()
    rng = np.random.default_rng(5)
    a = rng.uniform(-0.1, 0.1, (16, 3)).astype(np.float32)
    t = np.float32([0.25, -0.5, 0.125])
    want = np.eye(4, dtype=np.float32); want[:3, 3] = t
    for _ in range(3):
        c = ope.Context(0)
        for _ in range(10):                                    # two copies of 192 bytes per call
            np.testing.assert_allclose(c.rigid_transform_svd(a, a + t), want, atol=1e-5, rtol=0)
        c.close()


# ------------------------------------------------------------------ the normals that feed it
@pytest.mark.parametrize("k", [10, 12, 30])          # the LDS list and the two register lists of normals_kernel
def test_degenerate_neighbourhoods_give_the_oracles_normals(ctx, k):
    line = np.ascontiguousarray(cases()["line"].P)
    nrm, curv = ctx.normals(ctx.upload(line), k)
    onrm, ocurv = oracle.normals_knn(line, k)
    assert np.isnan(nrm).all() and np.isnan(onrm).all()                            # collinear: NaN normals,
    np.testing.assert_array_equal(curv, 0.0)                                       # curvature 0
    np.testing.assert_array_equal(ocurv, 0.0)
    nrm, curv = ctx.normals(ctx.upload(plane_lattice()), k)
    np.testing.assert_array_equal(nrm, np.tile(np.float32([0, 0, -1]), (64, 1)))   # a plane: exactly its normal, towards the origin
    np.testing.assert_array_equal(curv, 0.0)


def test_batch_normals_of_degenerate_neighbourhoods(ctx):
    ope = load_pkg()
    line, plane = np.ascontiguousarray(cases()["line"].P), plane_lattice()
    p = ope.default_coarse_params(key_leaf=H7, fpfh_radius=BATCH_R, normals_k=30, sacia=ope.default_sacia_params(max_iterations=4))
    ctx.coarse_pose_batch(ctx.upload(plane), [ctx.upload(line)], p)
    idx, nrm, _ = ctx.coarse_batch_features(-1)
    np.testing.assert_array_equal(np.sort(idx), np.arange(64))
    np.testing.assert_array_equal(nrm, np.tile(np.float32([0, 0, -1]), (64, 1)))
    idx, nrm, _ = ctx.coarse_batch_features(0)
    assert len(idx) == 40 and np.isnan(nrm).all()
