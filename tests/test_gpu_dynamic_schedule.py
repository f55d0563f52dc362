"""The slot queue of the tree accumulate kernel (icp_kernels.hip: deal_next): planned launches deal their slots to the waves
from striped device counters instead of a static hand.  What can go wrong is a slot taken twice, a slot never taken, or a
stale counter:

  * a query answered twice shows as n_corr above the number of finite queries;
  * a skipped query keeps the previous launch's d2, which differs because the transform has moved.

So every case steps a run launch by launch and compares, after a launch, n_corr, the per-query d2 BIT FOR BIT and the
matched indices (exact fp32 ties may pick another index, as in test_gpu_icp.py) against oracle.KdTree searching with the
very transform the launch searched with, and the transform the launch's update produced against the oracle's Umeyama step
over the oracle's correspondences (1e-5: the tolerance of test_icp_large_launch_each_kernel_matches_oracle_d2_bit_exact).
Kernels are forced by name and asserted through ope_icp_kernel_launches (KERNELS of test_gpu_icp.py).
"""
import numpy as np
import pytest
import torch

import oracle
from conftest import load_pkg

pytestmark = pytest.mark.gpu

synth = __import__("importlib").import_module("object-pose-estimation_amd.synth")

KERNELS = {"tree_lane": dict(grid=0, tree_walk=1), "tree_packet": dict(grid=0, tree_walk=2)}
FIXED = dict(transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, mse_threshold_absolute=-1.0)
# the library's constants this file sizes its cases by (ope_internal.hpp): stripes of the queue, and waves a CU holds of the
# plain accumulate kernel (kAccWavesPerSimd = 6 on 4 SIMDs)
DEAL_STRIPES = 64
WAVES_PER_CU = 24


@pytest.fixture(scope="module")
def ctx():
    ope = load_pkg()
    c = ope.Context(0)
    yield c
    c.close()


def frob(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


def orc_params(**kw):
    p = oracle.default_icp_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_MODEL = {}


def model():
    """20 k model points and their oracle tree, shared by every case of this file (never modified)."""
    if not _MODEL:
        tgt = synth.model_surface(20_000, 1)
        _MODEL.update(tgt=tgt, tree=oracle.KdTree(tgt))
    return _MODEL


_LARGE = {}


def large():
    """420 k queries with 10 % clutter (> 6144 chunks: several slots per wave on an MI355X); the oracle's 10-iteration run once."""
    if not _LARGE:
        src = synth.scene_cloud(420_000)
        ref = oracle.icp(src, model()["tgt"], orc_params(acc_mode=1, transform_mode=1, max_iterations=10, **FIXED))
        _LARGE.update(src=src, ref=ref)
    return _LARGE


def check_launch(ctx, src, Tprev, Tnow, n_finite=None):
    """The launch that searched with Tprev and whose update produced Tnow, against the oracle."""
    m = model()
    q, mi, d2 = ctx.icp_correspondences(len(src))
    n_finite = len(src) if n_finite is None else n_finite
    assert len(q) == n_finite, (len(q), n_finite)                   # a slot taken twice / not at all moves the count
    assert ctx.icp_poll().n_corr == n_finite
    moved = oracle.transform_points(src, Tprev)
    oi, od, _ = m["tree"].knn(moved[q], 1)
    np.testing.assert_array_equal(d2, od[:, 0])                     # bit for bit: a skipped query keeps a stale d2
    assert (mi != oi[:, 0]).mean() < 1e-4                           # exact fp32 distance ties may pick another index
    if n_finite >= 3:
        step = oracle.umeyama(moved[q], m["tgt"][oi[:, 0]], 1).astype(np.float64) @ np.asarray(Tprev, np.float64)
        assert frob(Tnow, step) < 1e-5, frob(Tnow, step)


def stepped_run(ctx, kernel, src, iterations, check_at, n_finite=None, certifying=False, **kw):
    """`iterations` launches, one per call, on the named kernel; the launches listed in check_at (1-based) are checked."""
    ope = load_pkg()
    cs = ctx.upload(src)
    ix = ctx.build_index(ctx.upload(model()["tgt"]), grid=KERNELS[kernel]["grid"])
    p = ope.default_icp_params(tree_walk=KERNELS[kernel]["tree_walk"], max_iterations=iterations, **{**FIXED, **kw})
    ctx.icp_begin(cs, ix, p, None)
    T = np.eye(4, dtype=np.float32)
    for it in range(1, iterations + 1):
        Tprev = T
        ctx.icp_iterate(1)
        T = ctx.icp_current_transform()                             # (synchronises)
        if it in check_at:
            check_launch(ctx, src, Tprev, T, n_finite)
        else:
            nf = len(src) if n_finite is None else n_finite
            assert ctx.icp_poll().n_corr == nf
    c = ctx.icp_kernel_launches()
    assert c[kernel] == iterations and sum(c.values()) == iterations, (kernel, c)
    if certifying:
        assert ctx.icp_certificate_stats()["launches"] > 0
    return ctx.icp_end()


@pytest.mark.parametrize("update_launch", [0, 1], ids=["overlapped", "in_line"])
@pytest.mark.parametrize("kernel", ["tree_lane", "tree_packet"])
def test_several_rounds_with_group_walks_in_the_plan(ctx, kernel, update_launch):
    """Ten launches under the plans made after launches 1, 2, 4 and 8.  Launch 3 is the first dealt from the queue; 4 and 8
    are measuring launches (no group walks: the list is the chunk order itself); 5, 6 and 10 each run under a plan of their
    own with group walks merged in: those six are compared query by query, all ten by their counts."""
    c = large()
    out = stepped_run(ctx, kernel, c["src"], 10, check_at=(3, 4, 5, 6, 8, 10), update_launch=update_launch)
    assert ctx.icp_overlapped_updates() == (10 if update_launch == 0 else 0)
    assert out.iterations == c["ref"].iterations == 10 and out.n_corr == c["ref"].n_corr == len(c["src"])
    assert frob(out.T, c["ref"].T) < 2e-5                           # (test_icp_fixed_iterations_per_iteration_parity's bound)


def test_ragged_stripes(ctx):
    """n_waves + stripes + 3 chunks and a partial one of 7 queries: the stripes have unequal lengths (one, two or no entries
    beyond the group walks' slots) and most waves' first pop comes back past the end.  n_waves as the library computes it:
    the blocks the device holds (in-line updates: none held back for the update's wave)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_waves = n_cu * WAVES_PER_CU
    n = (n_waves + DEAL_STRIPES + 3) * 64 + 7
    src = synth.scene_cloud(n)
    out = stepped_run(ctx, "tree_packet", src, 5, check_at=(3, 4, 5), update_launch=1)
    assert out.iterations == 5 and out.n_corr == n


@pytest.mark.parametrize("n", [64 * 3 + 5, 1])
def test_fewer_slots_than_waves(ctx, n):
    """Every wave that has a slot got it statically: nobody's pop succeeds (one query: one chunk, and no plan at all)."""
    src = synth.scene_cloud(n)
    for kernel in ("tree_lane", "tree_packet"):
        if n >= 3:
            out = stepped_run(ctx, kernel, src, 6, check_at=(2, 3, 4, 5, 6))
            assert out.iterations == 6 and out.n_corr == n
        else:
            # one pair determines no rigid transform: the run is compared with the oracle's as a whole
            ope = load_pkg()
            cs = ctx.upload(src)
            ix = ctx.build_index(ctx.upload(model()["tgt"]), grid=0)
            out = ctx.icp(cs, ix, ope.default_icp_params(tree_walk=KERNELS[kernel]["tree_walk"], max_iterations=6, **FIXED))
            ref = oracle.icp(src, model()["tgt"], orc_params(acc_mode=1, transform_mode=1, max_iterations=6, **FIXED))
            assert out.iterations == ref.iterations and out.state == ref.state and out.n_corr == ref.n_corr
            np.testing.assert_allclose(out.T, ref.T, atol=1e-5)
            if out.iterations > 0:
                q, mi, d2 = ctx.icp_correspondences(n)
                assert len(q) == 1


def test_certifying_instantiation_has_its_own_number_of_waves(ctx):
    """skip_certificates = CERT_ALWAYS at 30 000 queries: the certifying instantiation holds fewer blocks per CU (another
    number of waves) and keeps the static deal, fed by the same plans, next to the queue's counters that every launch of the
    kernel clears for its successor."""
    ope = load_pkg()
    src = synth.scene_cloud(30_000)
    for kernel in ("tree_lane", "tree_packet"):
        out = stepped_run(ctx, kernel, src, 10, check_at=(3, 4, 5, 6, 8, 10), certifying=True, skip_certificates=ope.CERT_ALWAYS)
        assert out.iterations == 10 and out.n_corr == len(src)


def _final_launch(ctx, cs, ix, params, iterations, how, cap):
    """A run of `iterations` launches; returns (transform before the last launch, d2 of the last launch, result)."""
    ctx.icp_begin(cs, ix, params, None)
    T = np.eye(4, dtype=np.float32)
    for it in range(iterations):
        Tprev = T
        if how == "step":
            ctx.icp_accumulate()
            ctx.icp_update()
        else:
            ctx.icp_iterate(1)
        T = ctx.icp_current_transform()
    q, mi, d2 = ctx.icp_correspondences(cap)
    return Tprev, q.copy(), d2.copy(), ctx.icp_end()


def test_counters_stay_clean_across_runs_on_one_context(ctx):
    """On ONE context: a run ended after 3 of its 10 iterations, then a full run, then the same one iteration per call
    through accumulate / update — each against a run of the same length on a FRESH context.

    Two runs of the same inputs are not bit-equal by themselves: the blocks' fp64 sums are added atomically in an order that
    varies (before this queue as well), so the fp32 transform a later launch searches with may differ in a last bit.  The d2 of
    each run's last launch are therefore compared bit for bit with the oracle under that run's OWN transform — which is what
    "the same as a fresh run" means query by query — and with the fresh run's directly whenever the two transforms are the same
    bits; the transforms at the run-to-run level of the atomic sums.

    Measured, not yet settled: 30 such pairs of 10-iteration runs (fresh context against a long-lived one, these inputs, one
    MI355X) gave a handful of distinct distances, 0 to 1.1239e-6, 9 of the 30 above the 1e-6 below (1.0243e-6, 1.0344e-6, 1.0496e-6,
    1.0931e-6, 1.1226e-6, 1.1239e-6); the same library under the Python binding as it was before its shared helpers and as it
    is with them gave the same set of values (9 and 12 of 30 above).  So this test misses from time to time whatever else
    changes; the bound is left as it was set."""
    ope = load_pkg()
    c, m = large(), model()
    src = c["src"]
    p = ope.default_icp_params(tree_walk=2, max_iterations=10, **FIXED)

    def run_on(cx, iterations, how):
        cs = cx.upload(src)
        ix = cx.build_index(cx.upload(m["tgt"]), grid=0)
        Tprev, q, d2, out = _final_launch(cx, cs, ix, p, iterations, how, len(src))
        assert len(q) == len(src) and out.n_corr == len(src) and out.iterations == iterations
        _, od, _ = m["tree"].knn(oracle.transform_points(src, Tprev)[q], 1)
        np.testing.assert_array_equal(d2, od[:, 0])
        return Tprev, d2, out

    fresh = {}
    for iterations in (3, 10):
        cx = ope.Context(0)
        fresh[iterations] = run_on(cx, iterations, "iterate")
        cx.close()
    for iterations, how in ((3, "iterate"), (10, "iterate"), (10, "step")):
        Tprev, d2, out = run_on(ctx, iterations, how)
        fT, fd2, fout = fresh[iterations]
        assert frob(out.T, fout.T) <= 1e-6
        if np.array_equal(Tprev, fT):
            np.testing.assert_array_equal(d2, fd2)


def test_deterministic_sums_do_not_use_the_queue_and_stay_bit_reproducible():
    """deterministic_sums = 1 on C2, twice: no plan, natural chunk order, the same bits."""
    ope = load_pkg()
    src, tgt = synth.config_clouds("C2")
    outs = []
    for _ in range(2):
        cx = ope.Context(0)
        cs = cx.upload(src); ix = cx.build_index(cx.upload(tgt))
        outs.append(cx.icp(cs, ix, ope.default_icp_params(max_iterations=40, mse_threshold_absolute=-1.0, check_every=0, deterministic_sums=1)))
        cx.close()
    assert np.array_equal(outs[0].T, outs[1].T) and outs[0].last_mse == outs[1].last_mse and outs[0].n_corr == outs[1].n_corr
