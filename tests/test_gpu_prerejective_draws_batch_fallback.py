"""The fallback path of the batched prerejective aligner under device draws (prerejective_batch.hip, step b): a problem the device
could not finish inside the window or the stream budget is drawn on the host, uploaded into its slice, and the prerejection runs
again.  The path is reached through ope_prerejective_set_draws_limits alone, at a budget (a window) worked out from the serial
loop on the CPU so that exactly the predicted clusters fall back; results and kept hypotheses must be host mode's, byte for byte,
and the extra launches and synchronisations the counted ones."""
import numpy as np
import pytest

import prerejective_draws_ref as dref
import test_gpu_prerejective_batch as tb
import test_gpu_prerejective_draws as td
from conftest import load_pkg

pytestmark = pytest.mark.gpu

HOST_LAUNCHES, DEVICE_LAUNCHES, SYNCS = 9, 12, 3
H = 300          # short streams: the serial loop on the CPU stays cheap


@pytest.fixture(scope="module")
def ope():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(ope, ctx):
    """The first three clusters in host mode: the run every device-mode run below must equal."""
    model, cl = tb.load_model(), tb.six_clusters()[:3]
    ctx.prerejective_set_draws(ope.DRAWS_HOST)
    run = tb.run_batch(ope, ctx, model, cl, max_iterations=H)
    assert (run["stats"]["launches"], run["stats"]["host_syncs"]) == (HOST_LAUNCHES, SYNCS)
    assert [r.status for r in run["res"]] == [ope.PREREJ_OK] * 3
    return run


def device_run(ope, ctx, host, window=0, budget=0, **kw):
    ctx.prerejective_set_draws(ope.DRAWS_DEVICE)
    ctx.prerejective_set_draws_limits(window, budget)
    try:
        run = tb.run_batch(ope, ctx, host["model"], host["clouds"], **dict(dict(max_iterations=H), **kw))
        run["draws"] = ctx.prerejective_draws_stats()
    finally:
        ctx.prerejective_set_draws_limits(0, 0)
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
    return run


def assert_equals_host(host, dev, fallbacks):
    assert [r.raw for r in dev["res"]] == [r.raw for r in host["res"]]
    for i in range(len(dev["res"])):
        assert tb.hyp_key(dev["hyps"][i]) == tb.hyp_key(host["hyps"][i]), i
    # per fallen-back problem one upload and one synchronisation, then NaN words, polygon, select, offsets and their synchronisation
    extra = (fallbacks + 4, fallbacks + 1) if fallbacks else (0, 0)
    assert (dev["stats"]["launches"], dev["stats"]["host_syncs"]) == (DEVICE_LAUNCHES + extra[0], SYNCS + extra[1])
    assert sum(r.survivors for r in dev["res"]) == dev["stats"]["survivors"] == host["stats"]["survivors"] > 0


def test_a_budget_between_the_clusters_sends_the_predicted_ones_back(ope, ctx, host):
    ns, seeds = host["res"][0].n_src_keys, [r.seed for r in host["res"]]
    last = [int(dref.iteration_starts(ns, 3, 5, H, sd)[H - 1]) for sd in seeds]
    assert len(set(last)) > 1, last                                          # the streams differ, so a budget can separate them
    budget = max(last)                                # the latest last iteration starts AT it: not inside
    short = sum(v >= budget for v in last)
    assert 0 < short < 3
    dev = device_run(ope, ctx, host, budget=budget)
    assert td.fallback_counts(dev["draws"]) == (3 - short, 0, short, 0) and dev["draws"]["positions"] == budget
    assert_equals_host(host, dev, short)
    for i, r in enumerate(dev["res"]):                                       # host-drawn and device-drawn slices alike
        np.testing.assert_array_equal(dev["hyps"][i]["samples"], td.ref_draws(ns, 3, 5, H, r.seed)[0])
    # one more position and everything stays on the device
    dev = device_run(ope, ctx, host, budget=budget + 1)
    assert td.fallback_counts(dev["draws"]) == (3, 0, 0, 0)
    assert_equals_host(host, dev, 0)


def test_a_window_of_six_sends_every_cluster_with_a_redraw_back(ope, ctx, host):
    ns, seeds = host["res"][0].n_src_keys, [r.seed for r in host["res"]]
    over = sum(int(max(np.diff(dref.iteration_starts(ns, 3, 5, H, sd)))) > 6 for sd in seeds)
    assert over > 0                                                          # 300 iterations of 3 from ~634 redraw somewhere
    dev = device_run(ope, ctx, host, window=6)
    assert td.fallback_counts(dev["draws"]) == (3 - over, over, 0, 0)
    assert_equals_host(host, dev, over)


def test_after_a_fallback_the_defaults_draw_on_the_device_again(ope, ctx, host):
    device_run(ope, ctx, host, window=6)
    dev = device_run(ope, ctx, host)
    assert td.fallback_counts(dev["draws"]) == (3, 0, 0, 0)
    assert_equals_host(host, dev, 0)


def test_limits_are_refused_out_of_range(ope, ctx, host):
    for window, budget in ((5, 0), (1025, 0), (-1, 0), (0, -1)):
        with pytest.raises(ope.OpeError) as e:
            ctx.prerejective_set_draws_limits(window, budget)
        assert e.value.code == ope.OPE_EINVAL
    # a window below 2 * nr_samples is refused by the call that would use it, before anything is launched; host mode ignores it
    ctx.prerejective_set_draws_limits(6, 0)
    try:
        p8 = tb.params(ope, max_iterations=H, nr_samples=8, k_correspondences=1)
        before = ctx.prerejective_batch_stats()
        ctx.prerejective_set_draws(ope.DRAWS_DEVICE)
        with pytest.raises(ope.OpeError) as e:
            ctx.prerejective_pose_batch(host["m"], host["cs"], None, p8)
        assert e.value.code == ope.OPE_EINVAL and "window" in str(e.value) and ctx.prerejective_batch_stats() == before
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
        ctx.prerejective_pose_batch(host["m"], host["cs"], None, p8)
        st = ctx.prerejective_batch_stats()
        assert (st["launches"], st["host_syncs"]) == (HOST_LAUNCHES, SYNCS)
    finally:
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
        ctx.prerejective_set_draws_limits(0, 0)
