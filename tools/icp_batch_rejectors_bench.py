"""The global rejectors inside the batched ICP kernel at the reference's fine-stage size (C1): one ope_icp_run_batch_rejectors call
against what the single path offers for the same K problems, and against the batch without a list.

Inputs, candidates and parameters are those of tools/icp_batch_bench.py.  Per K and per list three columns, measured in the same
run, their repetitions alternating:
  (a) ope_icp_run_batch_rejectors with the list;
  (b) K x ope_icp_run with the list set on the context (ope_icp_set_global_rejectors): the only way to the rejectors without (a);
  (c) ope_icp_run_batch without a list: what the stage itself costs is (a) - (c), on runs that do not iterate alike.

Host clock around each synchronous call, 5 warm-up and 20 timed repetitions, median and min-max.

    python tools/icp_batch_rejectors_bench.py [--ks 1,8,32] [--lists median:0.8,one-to-one,trimmed:0.3] [--warmup 5] [--reps 20] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ope = importlib.import_module("object-pose-estimation_amd")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
base = importlib.import_module("icp_batch_bench")


def parse_list(spec):
    """median:<factor> | one-to-one | trimmed:<min_ratio>, joined by '+' for a list of several."""
    out = []
    for item in spec.split("+"):
        name, _, value = item.partition(":")
        if name == "median":
            out.append(ope.global_rejector(0, factor=float(value or 1.0)))
        elif name == "one-to-one":
            out.append(ope.global_rejector(1))
        elif name == "trimmed":
            out.append(ope.global_rejector(2, min_ratio=float(value or 0.05)))
        else:
            raise SystemExit(f"unknown rejector {item!r}")
    return out


def alternating(fns, warmup, reps):
    """Every function once per round, warm-up rounds first: per function (median, min, max) in ms."""
    t = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                t[i].append(dt)
    return [(float(np.median(x)), float(np.min(x)), float(np.max(x))) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--lists", default="median:0.8,one-to-one,trimmed:0.3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = ope.Context(0)
    model, _ = pcd.read_pcd(os.path.join(base.GOLD, "drill_model_decimated.pcd"))
    sk, sn = base.fine_inputs(ctx, model)
    ks = [int(k) for k in a.ks.split(",")]
    cands, guess = base.candidates(ctx, max(ks))
    cs = ctx.upload(sk, sn)
    ix = [ctx.build_index(ctx.upload(tk, tn)) for tk, tn in cands]
    p = ope.default_icp_params(**base.FINE)
    print(f"source {len(sk)} key points; targets {min(len(t) for t, _ in cands)}-{max(len(t) for t, _ in cands)} key points")
    rows = []
    for spec in a.lists.split(","):
        lst = parse_list(spec)
        for k in ks:
            srcs, idx, gs = [cs] * k, ix[:k], [guess] * k
            res, _, _ = ctx.icp_batch_rejectors(srcs, idx, lst, p, gs)
            it_a = sum(r.iterations for r in res)
            it_c = sum(r.iterations for r in ctx.icp_batch(srcs, idx, p, gs))

            def single():
                ctx.icp_set_global_rejectors(lst)
                try:
                    return sum(ctx.icp(cs, x, p, guess).iterations for x in idx)
                finally:
                    ctx.icp_set_global_rejectors(None)

            it_b = single()
            ta, tb, tc = alternating([lambda: ctx.icp_batch_rejectors(srcs, idx, lst, p, gs), single, lambda: ctx.icp_batch(srcs, idx, p, gs)],
                                     a.warmup, a.reps)
            rows.append(dict(list=spec, K=k, iterations=dict(batch_rejectors=it_a, single=it_b, batch=it_c), batch_rejectors_ms=ta, single_ms=tb,
                             batch_ms=tc))
            print(f"{spec:14s} K={k:3d} | (a) batch + list {ta[0]:8.3f} ms [{ta[1]:.3f}-{ta[2]:.3f}] {it_a:5d} it | (b) {k} x ope_icp_run + list "
                  f"{tb[0]:8.3f} ms [{tb[1]:.3f}-{tb[2]:.3f}] {it_b:5d} it | (c) batch, no list {tc[0]:8.3f} ms [{tc[1]:.3f}-{tc[2]:.3f}] {it_c:5d} it "
                  f"| (b)/(a) x{tb[0] / ta[0]:.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
