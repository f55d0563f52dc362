"""The device draws of the batched prerejective aligner (prerejective_draws.hip) against tests/prerejective_ref.draws, the serial
loop in numpy: every sample and every pick, on the shapes at which the stream does something else (every index repeats, eight of
eight, 4096 indices, one iteration), at the tile boundaries, through both fallbacks and the refusals; then the batch and the
batched final pose in device mode against host mode on the same context, byte for byte.

The batch cases are the smallest of tests/test_gpu_prerejective_batch.py, whose clouds and helpers they use."""
import ctypes as C
import dataclasses
import multiprocessing as mp
import sys

import numpy as np
import pytest

import prerejective_draws_ref as dref
import prerejective_ref as ref
import test_gpu_prerejective_batch as tb
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

SEEDS = [1, 7, 2 ** 63 + 5, 2 ** 64 - 1, 9]
SHAPES = [(634, 3, 5, 2000), (3, 3, 1, 300), (8, 8, 8, 300), (9, 8, 2, 300), (4096, 3, 8, 1000), (10, 3, 1, 1)]
_REF = {}


def ref_draws(ns, S, K, H, seed):
    """prerejective_ref.draws, computed once per problem and never written to."""
    key = (ns, S, K, H, seed)
    if key not in _REF:
        samp, pick = ref.draws(*key)
        samp.setflags(write=False); pick.setflags(write=False)
        _REF[key] = (samp, pick)
    return _REF[key]


@pytest.fixture(scope="module")
def ope():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(ope):
    c = ope.Context(0)
    yield c
    c.close()


def check(got_s, got_p, ns, S, K, H, seeds):
    assert got_s.shape == got_p.shape == (len(seeds), H, S)
    for a, seed in enumerate(seeds):
        samp, pick = ref_draws(ns, S, K, H, seed)
        np.testing.assert_array_equal(got_s[a], samp, err_msg=f"samples of seed {seed}")
        np.testing.assert_array_equal(got_p[a], pick, err_msg=f"picks of seed {seed}")


def all_on_device(st, n):
    return (st["mode"], st["device"], st["overflow"], st["short"], st["host_for_size"]) == (1, n, 0, 0, 0)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_draws_equal_the_serial_loop(ope, ctx, shape):
    ns, S, K, H = shape
    s, p, st = ctx.prerejective_draws_device(ns, S, K, H, SEEDS)
    check(s, p, ns, S, K, H, SEEDS)
    assert all_on_device(st, len(SEEDS)) and st == ctx.prerejective_draws_stats()
    assert st["tile"] > 0 and st["positions"] == dref.budget(ns, S, H) and st["launches"] == 4
    rs, rp, _ = ctx.prerejective_draws_device(ns, S, K, H, SEEDS[::-1])
    assert rs[::-1].tobytes() == s.tobytes() and rp[::-1].tobytes() == p.tobytes()
    for a, seed in enumerate(SEEDS):
        one_s, one_p, one_st = ctx.prerejective_draws_device(ns, S, K, H, [seed])
        assert one_s[0].tobytes() == s[a].tobytes() and one_p[0].tobytes() == p[a].tobytes(), seed
        assert all_on_device(one_st, 1) and one_st["launches"] == st["launches"]


# ------------------------------------------------------------------ tile boundaries
def test_iterations_at_the_tile_boundaries(ope, ctx):
    ns, S, K, seed = 634, 3, 5, 1
    T = ctx.prerejective_draws_device(ns, S, K, 1, [seed])[2]["tile"]
    starts = np.array(dref.iteration_starts(ns, S, K, 20000, seed))          # starts[h] = where iteration h - 1 ends
    on = np.flatnonzero((starts % T == 0) & (starts > 0))
    assert len(on), "no iteration starts on a tile boundary in 20000"
    j = int(on[0])
    ends_on = j                                                              # iteration j - 1 ends exactly at a multiple of T
    starts_on = j + 1                                                        # iteration j starts exactly on it and is the last
    inside = np.flatnonzero((starts[:-1] // T) != ((starts[1:] - 1) // T))   # iterations that cross a boundary
    assert len(inside)
    straddles = int(inside[0]) + 1                                           # the last iteration straddles it
    assert starts[straddles - 1] % T != 0 and starts[straddles] % T != 0
    for H in (ends_on, straddles, starts_on):
        s, p, st = ctx.prerejective_draws_device(ns, S, K, H, [seed, 7])
        check(s, p, ns, S, K, H, [seed, 7])
        assert all_on_device(st, 2), (H, st)


# ------------------------------------------------------------------ fallbacks, reached through the arguments alone
# Every problem of a call shares ns, S, H, the window and the budget.  At (8, 8, 8, 300) an iteration takes 29.7 positions on
# average, so no seed keeps 300 iterations inside a window of 24, and at (3, 3, 1, 300) 300 iterations take 2 515 positions on
# average, so no seed starts them all inside 2 S H = 1 800: at a window of 24 or a budget of 2 S H no problem of such a call can
# stay on the device.  Those arguments are therefore run with a second seed and the counts the serial loop predicts for both, and the call with exactly one fallback beside exactly one device-drawn problem is made at the window (the
# budget) that separates the two seeds, worked out from the serial loop on the CPU: the shorter of the two fits it exactly.
def longest_iteration(ns, S, K, H, seed):
    return int(max(np.diff(dref.iteration_starts(ns, S, K, H, seed))))


def last_start(ns, S, K, H, seed):
    return int(dref.iteration_starts(ns, S, K, H, seed)[H - 1])


def fallback_counts(st):
    return st["device"], st["overflow"], st["short"], st["host_for_size"]


def test_window_24_falls_back_by_overflow(ope, ctx):
    shape, seeds = (8, 8, 8, 300), [9, 1]
    over = sum(longest_iteration(*shape, sd) > 24 for sd in seeds)
    assert longest_iteration(*shape, 9) > 24
    s, p, st = ctx.prerejective_draws_device(*shape, seeds, window=24)
    check(s, p, *shape, seeds)
    assert fallback_counts(st) == (len(seeds) - over, over, 0, 0)
    s, p, st = ctx.prerejective_draws_device(*shape, [9], window=24)
    check(s, p, *shape, [9])
    assert fallback_counts(st) == (0, 1, 0, 0)


def test_one_overflow_beside_a_problem_that_stays_on_the_device(ope, ctx):
    shape = (8, 8, 8, 300)
    other = next(sd for sd in range(1, 50) if longest_iteration(*shape, sd) != longest_iteration(*shape, 9))
    window = min(longest_iteration(*shape, 9), longest_iteration(*shape, other))       # fits the shorter one exactly
    assert 16 <= window <= 1024
    for seeds in ([9, other], [other, 9]):
        s, p, st = ctx.prerejective_draws_device(*shape, seeds, window=window)
        check(s, p, *shape, seeds)
        assert fallback_counts(st) == (1, 1, 0, 0)
    s, p, st = ctx.prerejective_draws_device(*shape, [9, other], window=window - 1)
    check(s, p, *shape, [9, other])
    assert fallback_counts(st) == (0, 2, 0, 0)


def test_budget_2SH_falls_back_by_short(ope, ctx):
    ns, S, K, H = shape = (3, 3, 1, 300)
    seeds = [7, 1]
    short = sum(last_start(*shape, sd) >= 2 * S * H for sd in seeds)
    assert last_start(*shape, 7) >= 2 * S * H
    s, p, st = ctx.prerejective_draws_device(*shape, seeds, budget=2 * S * H)
    check(s, p, *shape, seeds)
    assert fallback_counts(st) == (len(seeds) - short, 0, short, 0) and st["positions"] == 2 * S * H
    s, p, st = ctx.prerejective_draws_device(*shape, [7], budget=2 * S * H)
    check(s, p, *shape, [7])
    assert fallback_counts(st) == (0, 0, 1, 0)


def test_one_short_budget_beside_a_problem_that_stays_on_the_device(ope, ctx):
    shape = (3, 3, 1, 300)
    other = next(sd for sd in range(1, 50) if last_start(*shape, sd) != last_start(*shape, 7))
    budget = max(last_start(*shape, 7), last_start(*shape, other))   # the later of the two last iterations starts AT it: not inside
    for seeds in ([7, other], [other, 7]):
        s, p, st = ctx.prerejective_draws_device(*shape, seeds, budget=budget)
        check(s, p, *shape, seeds)
        assert fallback_counts(st) == (1, 0, 1, 0) and st["positions"] == budget
    s, p, st = ctx.prerejective_draws_device(*shape, [7, other], budget=budget + 1)
    check(s, p, *shape, [7, other])
    assert fallback_counts(st) == (2, 0, 0, 0)


# ------------------------------------------------------------------ refusals
def good_call(ctx):
    s, p, st = ctx.prerejective_draws_device(10, 3, 1, 1, [5])
    samp, pick = ref_draws(10, 3, 1, 1, 5)
    return (s[0] == samp).all() and (p[0] == pick).all() and all_on_device(st, 1)


BAD = [dict(H=0), dict(H=(1 << 20) + 1), dict(S=2), dict(S=9), dict(K=0), dict(K=9), dict(ns=2), dict(ns=4097), dict(window=5),
       dict(window=1025), dict(window=-1), dict(budget=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_parameters_are_refused(ope, ctx, bad):
    assert good_call(ctx)
    before = ctx.prerejective_draws_stats()
    a = dict(dict(ns=10, S=3, K=1, H=4, window=0, budget=0), **bad)
    with pytest.raises(ope.OpeError) as e:
        ctx.prerejective_draws_device(a["ns"], a["S"], a["K"], a["H"], [1, 2], window=a["window"], budget=a["budget"])
    assert e.value.code == ope.OPE_EINVAL and "ope_prerejective_draws_device" in str(e.value)
    assert ctx.prerejective_draws_stats() == before                          # nothing launched: the last call's stats stand
    assert good_call(ctx)


def test_bad_arguments_are_refused(ope, ctx):
    L = ope.lib()
    seeds = (C.c_uint64 * 2)(1, 2)
    samp, pick, st = (C.c_int32 * 24)(), (C.c_int32 * 24)(), (C.c_int64 * 8)()
    full = [ctx.h, 10, 3, 1, 4, seeds, 2, 0, 0, samp, pick, st]
    for hole in (0, 5, 9, 10):                                               # ctx, seeds, samples, picks
        args = list(full)
        args[hole] = None
        assert L.ope_prerejective_draws_device(*args) == ope.OPE_EINVAL, hole
        assert good_call(ctx)
    args = list(full)
    args[11] = None                                                          # stats may be NULL
    assert L.ope_prerejective_draws_device(*args) == ope.OPE_OK
    assert np.array_equal(np.array(samp[:12]).reshape(4, 3), ref_draws(10, 3, 1, 4, 1)[0])
    args = list(full)
    args[6] = 0                                                              # n == 0 does nothing, whatever the pointers
    args[5] = args[9] = args[10] = None
    before = ctx.prerejective_draws_stats()
    assert L.ope_prerejective_draws_device(*args) == ope.OPE_OK and ctx.prerejective_draws_stats() == before
    assert L.ope_prerejective_draws_last_stats(ctx.h, None) == ope.OPE_EINVAL
    with pytest.raises(ope.OpeError) as e:
        ctx.prerejective_set_draws(2)
    assert e.value.code == ope.OPE_EINVAL and ctx.prerejective_get_draws() == ope.DRAWS_HOST
    assert good_call(ctx)


def _communicator_worker(out_path):
    sys.path.insert(0, ROOT)
    import importlib
    import torch  # noqa: F401  (librccl / libamdhip64 of the torch wheel first, as the sharded tests do)
    ope = importlib.import_module("object-pose-estimation_amd")
    c = ope.Context(0)
    c.comm_init(ope.comm_unique_id(), 1, 0)
    try:
        c.prerejective_draws_device(10, 3, 1, 4, [1])
        code = 0
    except ope.OpeError as e:
        code = e.code
    c.comm_destroy()
    s, _, st = c.prerejective_draws_device(10, 3, 1, 4, [1])
    c.close()
    np.save(out_path, np.array([code, st["device"]] + s.reshape(-1).tolist()))


@pytest.mark.timeout(300)
def test_context_with_a_communicator_is_refused(tmp_path):
    path = str(tmp_path / "comm.npy")
    pr = mp.get_context("spawn").Process(target=_communicator_worker, args=(path,))
    pr.start(); pr.join(240)
    assert pr.exitcode == 0
    got = np.load(path).tolist()
    assert got[:2] == [load_pkg().OPE_EINVAL, 1]
    assert got[2:] == ref_draws(10, 3, 1, 4, 1)[0].reshape(-1).tolist()


# ------------------------------------------------------------------ the batch: device mode against host mode
DEVICE_LAUNCHES = 12    # seeds, tables, compose, emit, NaN words, rows, polygon, select, offsets, fit, score, sums


@pytest.fixture(scope="module")
def clouds():
    return tb.load_model(), tb.six_clusters()


def both_modes(ope, ctx, model, cl, **kw):
    """The same batch with host draws, then with device draws, on one context; the device run's draw stats."""
    ctx.prerejective_set_draws(ope.DRAWS_HOST)
    host = tb.run_batch(ope, ctx, model, cl, **kw)
    ctx.prerejective_set_draws(ope.DRAWS_DEVICE)
    try:
        dev = tb.run_batch(ope, ctx, model, cl, **kw)
        dev["draws"] = ctx.prerejective_draws_stats()
    finally:
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
    return host, dev


def assert_same_batch(ope, host, dev, S=3, K=5, H=tb.H):
    assert [r.raw for r in dev["res"]] == [r.raw for r in host["res"]]
    active = 0
    for i, r in enumerate(dev["res"]):
        assert tb.hyp_key(dev["hyps"][i]) == tb.hyp_key(host["hyps"][i]), i
        if r.status == ope.PREREJ_OK:
            active += 1
            np.testing.assert_array_equal(dev["hyps"][i]["samples"], ref_draws(r.n_src_keys, S, K, H, r.seed)[0])
    assert active > 0 and sum(r.survivors for r in dev["res"]) > 0
    assert (host["stats"]["launches"], host["stats"]["host_syncs"]) == (9, 3)
    assert (dev["stats"]["launches"], dev["stats"]["host_syncs"]) == (DEVICE_LAUNCHES, 3)
    assert {k: v for k, v in dev["stats"].items() if k != "launches"} == {k: v for k, v in host["stats"].items() if k != "launches"}
    assert all_on_device(dev["draws"], active) and dev["draws"]["launches"] == 4
    return active


def test_batch_of_six_is_the_host_batch(ope, ctx, clouds):
    model, cl = clouds
    host, dev = both_modes(ope, ctx, model, cl)
    assert assert_same_batch(ope, host, dev) == 4
    assert [r.seed for r in dev["res"]] == [tb.SEED, tb.SEED + 1, tb.SEED + 2, tb.SEED + 3, 0, 0]
    assert ctx.prerejective_get_draws() == ope.DRAWS_HOST


@pytest.mark.parametrize("n_keys", [255, 256, 257])
def test_batch_at_the_chunk_boundary_of_the_model(ope, ctx, clouds, n_keys):
    model, cl = clouds
    sub = tb.model_keys(ctx, model)[:n_keys]
    host, dev = both_modes(ope, ctx, sub, cl[:3])
    assert [r.n_src_keys for r in dev["res"]] == [n_keys] * 3
    assert assert_same_batch(ope, host, dev) == 3


def test_batch_with_a_cluster_of_exactly_ten_key_points(ope, ctx, clouds):
    model, cl = clouds
    feats = tb.run_batch(ope, ctx, model, cl[:1], keep=False, max_iterations=100)["feats"]
    keys = cl[0][feats[1][0]]
    ten = keys[:: len(keys) // 10][:10].copy()
    host, dev = both_modes(ope, ctx, model, [cl[1], ten, ten[:9]], seeds=[tb.SEED + 1, 5, 6])
    assert [r.n_tgt_keys for r in dev["res"]][1:] == [10, 9] and [r.seed for r in dev["res"]] == [tb.SEED + 1, 5, 0]
    assert assert_same_batch(ope, host, dev) == 2


@pytest.mark.parametrize("kw", [dict(max_iterations=1999), dict(nr_samples=8, k_correspondences=1, similarity_threshold=0.5)],
                         ids=["partial-last-block", "eight-samples-one-neighbour"])
def test_batch_of_other_shapes(ope, ctx, clouds, kw):
    model, cl = clouds
    host, dev = both_modes(ope, ctx, model, cl[:3], **kw)
    assert assert_same_batch(ope, host, dev, S=kw.get("nr_samples", 3), K=kw.get("k_correspondences", 5),
                             H=kw.get("max_iterations", tb.H)) == 3


def test_batch_launches_do_not_depend_on_the_sizes(ope, ctx, clouds):
    model, cl = clouds
    m, cs = ctx.upload(model), [ctx.upload(c) for c in cl]
    counts = {}
    ctx.prerejective_set_draws(ope.DRAWS_DEVICE)
    try:
        for name, cc, kw in (("six", cs, {}), ("one", cs[:1], {}), ("six, H100", cs, dict(max_iterations=100)),
                             ("one, H100", cs[:1], dict(max_iterations=100))):
            ctx.prerejective_pose_batch(m, cc, None, tb.params(ope, **kw))
            st, ds = ctx.prerejective_batch_stats(), ctx.prerejective_draws_stats()
            assert st["clusters"] == len(cc) and st["iterations"] == kw.get("max_iterations", tb.H)
            assert all_on_device(ds, st["active"]) and ds["launches"] == 4
            counts[name] = (st["launches"], st["host_syncs"])
    finally:
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
    assert set(counts.values()) == {(DEVICE_LAUNCHES, 3)}, counts
    ctx.prerejective_pose_batch(m, cs, None, tb.params(ope))
    st = ctx.prerejective_batch_stats()
    assert (st["launches"], st["host_syncs"]) == (9, 3) and ctx.prerejective_draws_stats()["mode"] == ope.DRAWS_HOST


# ------------------------------------------------------------------ the batched final pose (the seeds by rank)
def flat(x):
    """A result object as a comparable tree: arrays by their bytes."""
    if dataclasses.is_dataclass(x):
        return tuple((f.name, flat(getattr(x, f.name))) for f in dataclasses.fields(x))
    if isinstance(x, np.ndarray):
        return x.dtype.str, x.shape, x.tobytes()
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, (list, tuple)):
        return tuple(flat(v) for v in x)
    return x


def test_final_pose_batch_equals_host_mode(ope, ctx, clouds):
    model, cl = clouds
    m = ctx.upload(model)
    cs = [ctx.upload(cl[i]) for i in (4, 2, 0, 1)]                           # an empty cluster in front uses up no seed
    p = tb.params(ope, seed=11)
    host, host_sel = ctx.final_pose_batch_prerejective(m, cs, None, p)
    host_stats = ctx.prerejective_batch_stats()
    ctx.prerejective_set_draws(ope.DRAWS_DEVICE)
    try:
        dev, dev_sel = ctx.final_pose_batch_prerejective(m, cs, None, p)
        dev_stats, ds = ctx.prerejective_batch_stats(), ctx.prerejective_draws_stats()
    finally:
        ctx.prerejective_set_draws(ope.DRAWS_HOST)
    assert [o.seed for o in dev] == [0, 11, 12, 13] and dev[0].status == ope.FINAL_EMPTY_TARGET
    assert flat(dev) == flat(host) and dev_sel == host_sel
    assert any(o.coarse.best_iteration >= 0 for o in dev[1:])
    assert (host_stats["launches"], host_stats["host_syncs"]) == (9, 3)
    assert (dev_stats["launches"], dev_stats["host_syncs"]) == (DEVICE_LAUNCHES, 3) and all_on_device(ds, 3)
