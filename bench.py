#!/usr/bin/env python3
"""bench.py — ICP iterations/sec on the BASELINE.json workload, one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is ONE ICP iteration (icp_mod.hpp:171-259: correspondence search over all scene points,
17-sum reduction, SVD transform update, convergence test) on synthetic config C3: a 1 M-point frame
(source/queries, 10 % clutter included) against a 100 k-point model (target/indexed), inputs resident in HBM,
target index prebuilt, early exit disabled so exactly W + K (+ the steady-state phase's) iterations execute.
With N > 1 the frame is sharded across ranks (strong scaling: total work fixed), the model index is replicated and
the 17 fp64 sums are all-reduced over RCCL once per iteration.

The run starts where the reference's own flow would start it (config C3 = "FPFH init + 100 ICP iters"): pass-through
crop of the frame (rosinterface.cpp:212), the reference's statistical outlier removal (processingpcd.cpp:62-77) standing
in for the segmentation this repo does not build, estimateCoarsePose (uniform key points, normals, FPFH, SAC-IA) on the
resulting cluster.  `pose_check` then asserts two things: the cluster's ICP from that pose lands within 1e-2 Frobenius of
the generator's pose (the reference flow end to end), and the timed run over the whole frame ends in the right basin
(its 10 % clutter, with no correspondence distance limit, pulls the fit by a few degrees — the oracle lands on the same
pose).  A failed check prints the JSON line and exits 4.

Rank 0 prints one JSON line with `roofline` (dominant kernel = the accumulate kernel, timed with HIP events on its
launch stream inside the timed region), `phases` (from the coarse pose = `value`; steady state, reported separately),
`coarse_stage` (per-kernel HIP-event times with the algorithmic bytes of SURVEY 8d, FPFH points/s, SAC-IA hypotheses/s)
and, at N = 1, `cpu_baseline` (the C oracle, a scalar single-thread port of the PCL path, on a bounded sample of the same
workload).  A timed window during which an overlapped update launch gave up its bounded wait (ope.h: ope_icp_update_fallbacks)
has timed launches that did nothing: it is detected and measured again (`config.update_launch` says how).

`--dump-outputs DIR` writes, after the timed steps, what the last timed step handed its caller as DIR/<name>.npy: the pose
(`transform`, float32 4x4, ope_icp_current_transform) and the run's state (`iterations`, `mse`, `n_corr`, `align_strength`,
float64, ope_icp_poll).  The inputs are generated from fixed seeds, so two builds run with the same arguments can be compared
output for output.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
WORKLOADS = {
    # name: (n_scene, n_model, description)
    "C3": (1_000_000, 100_000, "C3: synthetic 1M-pt scene (source) vs 100k-pt model (target), point-to-point ICP"),
    "C2": (100_000, 20_000, "C2: synthetic 100k-pt scene vs 20k-pt model, point-to-point ICP"),
}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="C3", choices=sorted(WORKLOADS))
    ap.add_argument("--comm", default="native", choices=["torch", "native"],
                    help="under torch.distributed.run: all-reduce through the library's own RCCL communicator (whole loop in "
                         "C++, default) or through torch.distributed; 'native' falls back to 'torch' if RCCL init fails")
    ap.add_argument("--leaf", type=int, default=0, help="index leaf size override (0 = library default)")
    ap.add_argument("--no-grid", action="store_true", help="OBB tree only (A/B against the bucketed search)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--wait-limit", type=float, default=None,
                    help="rehearsal: the bound of the device-side waits of overlapped update launches in seconds (ope_ctx_set_wait_limit; 1e-6 forces the fall-back to in-line launches)")
    ap.add_argument("--wait-limit-every-context", action="store_true", help="rehearsal: --wait-limit also on the fresh context of the second attempt (forces the in-line measurement)")
    ap.add_argument("--update-launch", default="overlapped", choices=["overlapped", "in-line"],
                    help="ope_icp_params.update_launch (include/ope.h): the library's default, or accumulate -> update -> accumulate "
                         "on one stream as in rounds 1-2 (A/B; and what a profiler that serialises dispatches, rocprofv3 --pmc, wants)")
    ap.add_argument("--certificates", default="auto", choices=["auto", "off", "always"],
                    help="ope_icp_params.skip_certificates (include/ope.h): the library's default, never, or from the first launch (A/B)")
    ap.add_argument("--no-ns", action="store_true", help="skip the normal-shooting leg (the correspondence estimation the reference's "
                                                          "estimateFinePose really installs), reported beside `value` at N = 1")
    ap.add_argument("--no-coarse", action="store_true", help="skip the FPFH + SAC-IA initial alignment (identity start)")
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (pose and run state) as DIR/<name>.npy")
    ap.add_argument("--steady", type=int, default=100, help="iterations timed in the converged regime, after the run has been taken to --settle iterations (reported, not `value`)")
    ap.add_argument("--settle", type=int, default=150, help="iterations from the coarse pose after which the run counts as settled (the steady-state phase starts there)")
    ap.add_argument("--full-run", type=int, default=100, help="a second run from the coarse pose, this many iterations timed as a whole (reported as phases.full_run; 0: skip)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal of the N-rank path on a box with ONE GPU: every rank uses device 0, the process group is gloo and the "
                         "sums travel through the library's peer-to-peer slots (handles passed over gloo; RCCL refuses two ranks on one "
                         "device).  The JSON line is marked; it is not a measurement of N GPUs")
    args = ap.parse_args()
    # Everything libraries print through fd 1 (RCCL's version banner, for one) goes to stderr; the one JSON line is
    # written to the real stdout at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            print(f"bench.py: --gpus {args.gpus} needs torch.distributed.run with --nproc-per-node {args.gpus}", file=sys.stderr)
            return 2
        args.gpus = world

    import numpy as np
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the hot path is HIP-only and has no CPU fallback", file=sys.stderr)
        return 3
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    cdev = "cpu" if args.share_gpu else "cuda"   # where the small tensors of the process-group collectives live
    # launched by torch.distributed.run (even with one rank): go through the process group, so the
    # collective path is the one exercised
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    ope = importlib.import_module("object-pose-estimation_amd")
    synth = importlib.import_module("object-pose-estimation_amd.synth")

    n_scene, n_model, desc = WORKLOADS[args.workload]
    K, W = args.steps, args.warmup
    scene = synth.scene_cloud(n_scene)
    model = synth.model_surface(n_model, 1)
    lo, hi = rank * n_scene // world, (rank + 1) * n_scene // world
    shard = scene[lo:hi]

    ctx = ope.Context(local_rank)
    use_torch_comm = launched and args.comm == "torch"
    if launched:
        # launch on torch's current stream so torch.distributed orders the collective with our kernels
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    cs = ctx.upload(shard)
    ix = ctx.build_index(ctx.upload(model), leaf_size=args.leaf or None, grid=not args.no_grid)
    sums = None
    if use_torch_comm:
        sums = torch.zeros(ope.NUM_SUMS, dtype=torch.float64, device="cuda")   # SVD estimator: exactly OPE_NUM_SUMS doubles are used
        ctx.icp_set_sums_buffer(sums.data_ptr())
    elif launched:
        ok = torch.ones(1, device=cdev)
        try:
            if args.share_gpu:
                handles = [None] * world
                dist.all_gather_object(handles, ctx.comm_p2p_open())
                ctx.comm_p2p_connect(handles, rank)
            else:
                ids = [ope.comm_unique_id() if rank == 0 else None]
                dist.broadcast_object_list(ids, src=0)
                ctx.comm_init(ids[0], world, rank)
        except Exception as e:  # pragma: no cover - depends on the node's RCCL
            print(f"[rank {rank}] native RCCL init failed ({e}); using torch.distributed", file=sys.stderr)
            ok.zero_()
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)        # every rank must agree on the transport
        if float(ok) == 0.0 and args.share_gpu:
            print("bench.py: --share-gpu needs the peer-to-peer slots and they could not be set up", file=sys.stderr)
            return 5
        if float(ok) == 0.0:
            try:
                ctx.comm_destroy()
            except Exception:
                pass
            args.comm = "torch"
            use_torch_comm = True
            sums = torch.zeros(ope.NUM_SUMS, dtype=torch.float64, device="cuda")   # SVD estimator: exactly OPE_NUM_SUMS doubles are used
            ctx.icp_set_sums_buffer(sums.data_ptr())

    # ---- what the reference does with a captured frame before and during estimateCoarsePose:
    #   ProcessingPcd::getPassThrough with the -l limits (rosinterface.cpp:212)  -> the workspace crop
    #   [plane segmentation + clustering, rosinterface.cpp:213: out of scope; the synthetic frame has no table.  What it
    #    does for the pose estimator — hand over the object's points without the surroundings — is done here by the
    #    reference's own ProcessingPcd::getOutlierRemove (StatisticalOutlierRemoval, meanK 30, processingpcd.cpp:62-77):
    #    at 1.4 clutter points per cm^3 EVERY 1 cm keypoint voxel of the crop box is occupied, and FPFH / SAC-IA see fog]
    #   estimateCoarsePose (poseestimator.cpp:16-73): uniform keypoints (leaf 0.01) -> normals (k=30) -> FPFH (r=0.03)
    #   on both clouds -> SAC-IA (400 x 5 x 5).
    # Every rank computes the initial pose (rank 0's is broadcast and used); it is reported, not part of `value`.
    coarse = None
    guess = None
    cluster = None
    gt_inv = np.linalg.inv(synth.ground_truth_pose())
    if not args.no_coarse:
        def front_end():
            """One frame through the reference's steps in front of the ICP; every stage hands its survivors on as a
            device-resident cloud (ope_*_cloud): no host round trip between the stages."""
            lo_w, hi_w = synth.workspace_limits(0.01)
            ctx.sync()
            t_c = time.perf_counter()
            stage = {}
            frame = ctx.upload(scene)
            t1 = time.perf_counter(); crop_c, _ = ctx.pass_through_cloud(frame, lo_w, hi_w)
            t2 = time.perf_counter(); clus, _ = ctx.statistical_outlier_removal_cloud(crop_c, 30, 1.0)
            t3 = time.perf_counter()
            stage["frame"] = {"points": int(len(scene)), "upload_ms": (t1 - t_c) * 1e3, "pass_through_kept": int(crop_c.n), "pass_through_ms": (t2 - t1) * 1e3,
                              "outlier_removal_kept": int(clus.n), "outlier_removal_ms": (t3 - t2) * 1e3}
            feats, kclouds = [], []
            for name, full in (("cluster", clus), ("model", ix.cloud)):
                t1 = time.perf_counter(); kc, _ = ctx.uniform_sampling_cloud(full, 0.01)
                t2 = time.perf_counter(); ctx.normals(kc, 30, fetch=False)
                t3 = time.perf_counter(); feats.append(ctx.fpfh(kc, 0.03))
                t4 = time.perf_counter()
                stage[name] = {"points": int(full.n), "keypoints": int(kc.n), "uniform_sampling_ms": (t2 - t1) * 1e3,
                               "normals_ms": (t3 - t2) * 1e3, "fpfh_ms": (t4 - t3) * 1e3}
                kclouds.append(kc)
            t5 = time.perf_counter()
            # SAC-IA in the reference's direction: source = the model, target = the scene cluster (rosinterface.cpp:250 hands
            # estimateFinalPose the loaded model as source); the ICP below runs scene -> model, so it starts from the inverse
            kix = ctx.build_index(kclouds[0])
            m2s, sac_err, sac_it = ctx.sacia(kclouds[1], feats[1], kclouds[0], kix, feats[0], ope.default_sacia_params(seed=1))
            t6 = time.perf_counter()
            return dict(stage=stage, total_ms=(t6 - t_c) * 1e3, sacia_ms=(t6 - t5) * 1e3, m2s=m2s, sac_err=sac_err, sac_it=sac_it, cluster=clus)

        # the first frame pays for the lazy loading of every kernel it touches (~35 ms of the first upload alone); the reference's
        # loop sees one frame after another, so the frame that is reported is the second one, the first one's total beside it
        first = front_end()
        ctx.profile_kernels(True)
        fe = front_end()
        ktimes = ctx.profile_kernels_read()
        ctx.profile_kernels(False)
        assert np.array_equal(np.asarray(first["m2s"]), np.asarray(fe["m2s"]))      # same frame, same pose
        stage, cluster, sac_err, sac_it = fe["stage"], fe["cluster"], fe["sac_err"], fe["sac_it"]
        guess = np.linalg.inv(np.asarray(fe["m2s"], np.float64)).astype(np.float32)
        kroof = {}
        for kname, rec in sorted(ktimes.items()):
            gbs = rec["algorithmic_bytes"] / (rec["ms"] * 1e-3) / 1e9 if rec["ms"] > 0 else 0.0
            kroof[kname] = {"bound": "hbm", "ms": rec["ms"], "launches": rec["launches"],
                            "algorithmic_bytes": rec["algorithmic_bytes"], "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": gbs / HBM_PEAK_GBS}
        n_kp = stage["cluster"]["keypoints"] + stage["model"]["keypoints"]
        fp_ms = ktimes.get("spfh_kernel", {}).get("ms", 0.0) + ktimes.get("fpfh_kernel", {}).get("ms", 0.0)
        sa_ms = ktimes.get("sacia_error_kernel", {}).get("ms", 0.0)
        coarse = {"total_ms": fe["total_ms"], "first_frame_total_ms": first["total_ms"], "sacia_ms": fe["sacia_ms"], "sacia_hypotheses": 400,
                  "sacia_best_iteration": int(sac_it), "sacia_error": float(sac_err),
                  "pose_error_vs_ground_truth_frobenius": float(np.linalg.norm(guess.astype(np.float64) - gt_inv)),
                  "fpfh_points_per_s": n_kp / (fp_ms * 1e-3) if fp_ms > 0 else None,
                  "sacia_hypotheses_per_s": 400 / (sa_ms * 1e-3) if sa_ms > 0 else None,
                  "stages": stage, "kernels": kroof,
                  "note": "total_ms: the second pass over the same frame (device-resident hand-over between the stages; host wall-clock incl. "
                          "the frame's upload, device index builds and the read-backs that are left: sizes, the outlier filter's two sums, 33 x "
                          "key points descriptors); first_frame_total_ms: the first pass, which also loads every kernel it touches; `kernels` "
                          "are HIP-event times of the launches with the algorithmic bytes of SURVEY 8d; none of it is part of value"}

    if launched and guess is not None:
        # one initial pose for the whole job: every rank computed it from the same inputs, but the ranks must not
        # depend on bit-identical results across devices, so rank 0's is the one that is used
        g = torch.from_numpy(np.ascontiguousarray(guess)).to(cdev)
        dist.broadcast(g, src=0)
        guess = g.cpu().numpy()

    # W warm-up + K timed iterations from the coarse pose (`value`), then S more in the converged regime (reported
    # separately: an iteration is cheaper once the scene has settled on the model)
    S = args.steady
    settle = max(0, args.settle - (W + K)) if S > 0 else 0      # untimed iterations between the timed window and the steady-state phase
    params = ope.default_icp_params(max_iterations=W + K + settle + S + 1, transformation_epsilon=0.0,
                                    euclidean_fitness_epsilon=0.0, mse_threshold_absolute=-1.0, check_every=0,
                                    update_launch=0 if args.update_launch == "overlapped" else 1,
                                    skip_certificates={"auto": ope.CERT_AUTO, "off": ope.CERT_OFF, "always": ope.CERT_ALWAYS}[args.certificates])
    def step():
        if use_torch_comm:
            ctx.icp_accumulate()
            dist.all_reduce(sums)
            ctx.icp_update()
        else:
            ctx.icp_iterate(1)

    def sync():
        ctx.sync()
        torch.cuda.synchronize()

    def timed(n, profile):
        """n steps bracketed by a barrier + synchronize on both sides; (seconds, kernel ms per launch)."""
        sync()
        if launched:
            dist.barrier()
        if profile:
            ctx.icp_profile(n)
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        sync()
        if launched:
            dist.barrier()
        sync()
        dt = time.perf_counter() - t0
        km, kn = ctx.icp_profile_read() if profile else (0.0, 0)
        if profile:
            timed.last_launch_ms = [round(float(v), 4) for v in ctx.icp_profile_launches()]
            ctx.icp_profile(0)
        return dt, (km / max(kn, 1)), kn

    # An overlapped update launch that gives up its bounded wait (ope.h: ope_icp_update_fallbacks — the GPU held up by something
    # else for two seconds) leaves the launches behind it as no-ops until the next poll re-enqueues them in line: a window
    # bracketed by stream synchronisation would then have timed nothing.  The counter is checked right after the window; a run
    # that fell back is ended and measured again from the same pose (the context launches in line from then on, and says so).
    update_launch_note = args.update_launch
    if args.wait_limit is not None:
        ctx.set_wait_limit(args.wait_limit)
    for attempt in range(3):
        fallbacks0 = ctx.icp_update_fallbacks()
        ctx.icp_set_global_sizes(n_scene, n_model)
        ctx.icp_begin(cs, ix, params, guess)
        for _ in range(W):
            step()
        elapsed, kern_avg_ms, kern_n = timed(K, True)
        launch_ms = getattr(timed, "last_launch_ms", None)
        kernels_timed = ctx.icp_kernel_launches()
        overlapped_updates = ctx.icp_overlapped_updates()
        T_timed = ctx.icp_current_transform()      # (polls: a fallback is noticed here at the latest)
        res_timed = ctx.icp_poll() if args.dump_outputs else None
        if ctx.icp_update_fallbacks() == fallbacks0:
            break
        assert attempt < 2, "the run fell back to in-line update launches in every attempt"
        ctx.icp_end()
        if attempt == 0 and not launched:
            # (both times this was seen, the hold-up was over within the process's first seconds: a fresh context — one that still
            # launches overlapped — gets one more try before the in-line measurement is taken)
            print("[bench] an overlapped update launch gave up its bounded wait; measuring again on a fresh context", file=sys.stderr, flush=True)
            ix.free(); cs.free(); ctx.close()
            ctx = ope.Context(local_rank)
            if args.wait_limit is not None and args.wait_limit_every_context:
                ctx.set_wait_limit(args.wait_limit)
            cs = ctx.upload(shard)
            ix = ctx.build_index(ctx.upload(model), leaf_size=args.leaf or None, grid=not args.no_grid)
            update_launch_note = args.update_launch + " (second attempt, on a fresh context: an overlapped update launch of the first gave up its bounded wait)"
        else:
            update_launch_note = "in-line (an overlapped update launch gave up its bounded wait: measured again, in line)"
            print("[bench] an overlapped update launch gave up its bounded wait; the timed window is measured again with in-line launches", file=sys.stderr, flush=True)
    cert_timed = ctx.icp_certificate_stats()
    steady, steady_invalid = None, None
    if S > 0:
        for _ in range(settle):
            step()
        c0 = ctx.icp_certificate_stats()
        s_elapsed, s_kern_ms, _ = timed(S, True)
        c1 = ctx.icp_certificate_stats()
        steady = {"steps": S, "after_iterations": W + K + settle, "ms_per_step": s_elapsed / S * 1e3, "iterations_per_s": S / s_elapsed, "kernel_ms": s_kern_ms,
                  "queries_answered_from_certificates_per_launch": (c1["certified"] - c0["certified"]) / S}
        ctx.icp_current_transform()   # (polls)
        if ctx.icp_update_fallbacks() != fallbacks0:   # (as above; this phase is reported beside `value`, not measured again)
            steady, steady_invalid = None, "an overlapped update launch gave up its bounded wait during this phase: its launches were re-enqueued outside the timed region"
    out = ctx.icp_end()
    assert out.iterations == W + K + settle + S, (out.iterations, W, K, settle, S)
    # ---- a whole run as the reference's flow has it: from the coarse pose, --full-run iterations, timed as one piece
    full = None
    if args.full_run > 0:
        pf = ope.default_icp_params(max_iterations=args.full_run + 1, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, mse_threshold_absolute=-1.0,
                                    check_every=0, update_launch=params.update_launch, skip_certificates=params.skip_certificates)
        for attempt in range(2):   # (measured again if an overlapped update launch gave up its wait, as above)
            fallbacks0 = ctx.icp_update_fallbacks()
            ctx.icp_set_global_sizes(n_scene, n_model)
            ctx.icp_begin(cs, ix, pf, guess)
            f_elapsed, f_kern_ms, f_n = timed(args.full_run, True)
            cf = ctx.icp_certificate_stats()
            f_launch_ms = getattr(timed, "last_launch_ms", None)
            of = ctx.icp_end()
            if ctx.icp_update_fallbacks() == fallbacks0:
                break
        full = {"steps": args.full_run, "ms": f_elapsed * 1e3, "ms_per_step": f_elapsed / args.full_run * 1e3, "kernel_ms_sum": f_kern_ms * f_n,
                "kernel_ms_by_tens": [round(sum(f_launch_ms[k:k + 10]) / len(f_launch_ms[k:k + 10]), 4) for k in range(0, len(f_launch_ms), 10)] if f_launch_ms else None,
                "launches_keeping_certificates": cf["launches"], "queries_answered_from_certificates": cf["certified"],
                "pose_error_vs_ground_truth_frobenius": float(np.linalg.norm(of.T.astype(np.float64) - gt_inv))}

    # ---- beside `value`: the configuration estimateFinePose / getIcpNormal really run (poseestimator.cpp:242-246,331-337;
    # regmeshpcd.cpp:140-159): normal shooting over the k = 20 nearest + the surface-normal rejector at 0.7, SVD estimator,
    # on the same clouds (normals k = 30 as subSampleAndCalculateNormals attaches them, :153), from the same coarse pose.
    ns_leg = None
    if world == 1 and args.workload == "C3" and not args.no_ns:
        t0 = time.perf_counter()
        ctx.normals(cs, 30, fetch=False)
        cmn = ctx.upload(model); ctx.normals(cmn, 30, fetch=False)
        ixn = ctx.build_index(cmn, leaf_size=args.leaf or None)
        ctx.sync(); t_prep = time.perf_counter() - t0
        Wn, Kn = 10, 30
        pn = ope.default_icp_params(max_iterations=Wn + Kn + 1, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, mse_threshold_absolute=-1.0,
                                    check_every=0, corr_mode=ope.CORR_NORMAL_SHOOTING, k_normal_shooting=20, use_surface_normal_rej=1, surface_normal_thr=0.7)
        ctx.icp_begin(cs, ixn, pn, guess)
        ctx.icp_iterate(Wn); ctx.sync()
        ctx.icp_profile(Kn)
        t0 = time.perf_counter(); ctx.icp_iterate(Kn); ctx.sync(); dtn = time.perf_counter() - t0
        kmn, knn = ctx.icp_profile_read(); ctx.icp_profile(0)
        on = ctx.icp_end()
        kms = kmn / max(knn, 1)
        ns_bytes = 60.0 * n_scene + 24.0 * n_model      # SURVEY 8d, "with normals": 60 B per source point + 24 B per target point
        ns_gbs = ns_bytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        ns_traffic = None
        try:
            ns_traffic = json.load(open(os.path.join(ROOT, "profiles", "r3_pmc_traffic.json"))).get(args.workload + "-ns", {}).get("hbm_bytes_per_launch")
        except Exception:
            ns_traffic = None
        ns_leg = {"workload": "C3-ns: the same clouds, normal shooting k = 20 + surface-normal rejector 0.7 (estimateFinePose's correspondence estimation), SVD estimator",
                  "steps": Kn, "warmup": Wn, "ms_per_step": dtn / Kn * 1e3, "iterations_per_s": Kn / dtn, "n_corr": int(on.n_corr),
                  "normals_and_index_ms": t_prep * 1e3,
                  "roofline": {"bound": "hbm", "achieved": ns_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ns_gbs / HBM_PEAK_GBS, "traffic": ns_traffic,
                               "kernel": "icp_accumulate_kernel<2,true,false,*,20>", "kernel_ms": kms, "launches_timed": knn,
                               "algorithmic_bytes_per_launch": ns_bytes}}

    if launched:
        vals = [elapsed, kern_avg_ms] + ([steady["ms_per_step"], steady["kernel_ms"]] if steady else [0.0, 0.0]) + ([full["ms"]] if full else [0.0])
        t = torch.tensor(vals, dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kern_avg_ms = float(t[0]), float(t[1])
        if steady:
            steady["ms_per_step"], steady["kernel_ms"] = float(t[2]), float(t[3])
            steady["iterations_per_s"] = 1e3 / steady["ms_per_step"]
        if full:
            full["ms"] = float(t[4]); full["ms_per_step"] = full["ms"] / full["steps"]

    rc = 0
    if rank == 0:
        n_local = hi - lo
        # 36 B per source point (read xyz 12 + gather match 12 + write correspondence 12)
        # + 12 B per target point, per launch of the accumulate kernel on this rank
        algo_bytes = 36.0 * n_local + 12.0 * n_model
        achieved = algo_bytes / (kern_avg_ms * 1e-3) / 1e9 if kern_avg_ms > 0 else 0.0
        traffic, traffic_source = None, None
        if steady and steady["kernel_ms"] > 0:
            sa = algo_bytes / (steady["kernel_ms"] * 1e-3) / 1e9
            steady["roofline"] = {"bound": "hbm", "achieved": sa, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": sa / HBM_PEAK_GBS,
                                  "algorithmic_bytes_per_launch": algo_bytes}
        tf = os.path.join(ROOT, "profiles", "r4_pmc_traffic.json")
        if not os.path.exists(tf):
            tf = os.path.join(ROOT, "profiles", "r3_pmc_traffic.json")
        if world == 1 and os.path.exists(tf):
            try:
                rec = json.load(open(tf)).get(args.workload)
                if rec:
                    traffic = rec.get("hbm_bytes_per_launch")
                    traffic_source = rec.get("source")
            except Exception:
                traffic = None
        # pose of the timed run: the 1 M-point frame INCLUDING its 10 % clutter against the model, no correspondence
        # distance limit (the reference leaves it at PCL's default, poseestimator.cpp:314-316): the clutter's pull is part
        # of the result, so this lands in the right basin but not on the generator's pose
        err_timed = float(np.linalg.norm(np.asarray(T_timed, np.float64) - gt_inv))
        err_final = float(np.linalg.norm(out.T.astype(np.float64) - gt_inv))
        checks = {"timed_run_pose_error_vs_ground_truth_frobenius": err_timed, "final_pose_error_vs_ground_truth_frobenius": err_final,
                  "timed_run_bound": 0.25}
        ok = err_final < 0.25
        # the reference's own flow end to end: crop -> outlier removal -> coarse pose -> ICP of the CLUSTER (what
        # estimateFinalPose receives, rosinterface.cpp:250), 100 iterations: this one must land on the generator's pose
        if cluster is not None and world == 1:
            # (its own index with the bucketed search forced on: the cluster is clutter-free, which is the grid kernel's case,
            # and its launches then carry their own kernel name in the rocprofv3 summary instead of blending into the timed
            # kernel's average)
            ix2 = ctx.build_index(ctx.upload(model), leaf_size=args.leaf or None, grid=2)
            t0 = time.perf_counter()
            cc = cluster                                   # the device-resident cluster the front end left behind
            p2 = ope.default_icp_params(max_iterations=100, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0,
                                        mse_threshold_absolute=-1.0, check_every=0)
            o2 = ctx.icp(cc, ix2, p2, guess)
            e2 = float(np.linalg.norm(o2.T.astype(np.float64) - gt_inv))
            checks.update({"cluster_icp_pose_error_vs_ground_truth_frobenius": e2, "cluster_icp_bound": 1e-2,
                           "cluster_points": int(cluster.n), "cluster_icp_ms_100_iterations": (time.perf_counter() - t0) * 1e3})
            ok = ok and e2 < 1e-2
        checks["passed"] = bool(ok)
        line = {
            "metric": "ICP iterations/sec (1M scene pts vs 100k model pts) at 1/2/4/8 GPU" if args.workload == "C3"
                      else "ICP iterations/sec (100k scene pts vs 20k model pts)",
            "value": K / elapsed,
            "unit": "iterations/s",
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic" + (" (REHEARSAL: all ranks share one GPU, --share-gpu)" if args.share_gpu else ""),
            "config": {"workload": desc, "n_scene": n_scene, "n_model": n_model, "scene_shard_per_gpu": n_local,
                       "parallelism": f"scene-sharded x{world}, model index replicated, 17xfp64 all-reduce/iter"
                                      + (f" ({args.comm}" + ({ope.COMM_P2P: ": peer-to-peer slots", ope.COMM_RCCL: ": ncclAllReduce"}.get(ctx.comm_transport(), "") if not use_torch_comm else "") + ")" if launched else ""),
                       "start": "identity" if guess is None else "FPFH + SAC-IA coarse pose",
                       "final_mse": out.last_mse, "n_corr": int(out.n_corr),
                       "update_launch": update_launch_note, "overlapped_updates_so_far": overlapped_updates,
                       "skip_certificates": args.certificates, "certificates_in_timed_window": cert_timed},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": "icp_accumulate_kernel", "kernel_ms": kern_avg_ms, "launches_timed": kern_n,
                         "kernel_ms_per_launch": launch_ms if (launch_ms and len(launch_ms) <= 128) else None,
                         "kernel_launches_so_far": kernels_timed,
                         "algorithmic_bytes_per_launch": algo_bytes},
            "phases": {"from_coarse_pose": {"steps": K, "after_warmup": W, "ms_per_step": elapsed / K * 1e3, "kernel_ms": kern_avg_ms},
                       "steady_state": steady if steady is not None else ({"invalid": steady_invalid} if steady_invalid else None), "full_run": full},
            "pose_check": checks,
        }
        if ns_leg is not None:
            line["normal_shooting_leg"] = ns_leg
        if coarse is not None:
            line["coarse_stage"] = coarse
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(np, scene, model, args.cpu_iters, guess)
            # "also reported with all cores" — the same port, queries split over the usable host threads
            nthr = usable_cores()
            if nthr > 1:
                line["cpu_baseline_all_cores"] = cpu_baseline(np, scene, model, max(args.cpu_iters, 2 * min(nthr, 8)), guess, nthr)
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)     # C stdio buffers (still pointing at fd 1 = stderr now)
        except Exception:
            pass
        if args.dump_outputs:
            os.makedirs(args.dump_outputs, exist_ok=True)
            dump = {"transform": np.asarray(T_timed, np.float32), "iterations": np.float64(res_timed.iterations),
                    "mse": np.float64(res_timed.last_mse), "n_corr": np.float64(res_timed.n_corr),
                    "align_strength": np.float64(res_timed.align_strength)}
            for name, a in dump.items():
                np.save(os.path.join(args.dump_outputs, name + ".npy"), np.asarray(a))
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
        if not ok:
            print(f"bench.py: pose check FAILED: {checks}", file=sys.stderr)
            rc = 4
    ctx.close()
    if launched:
        dist.barrier()
        dist.destroy_process_group()
    return rc


def usable_cores() -> int:
    """Host threads this process may really use: the affinity mask, cut by the cgroup's CPU quota where one is set."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(np, scene, model, iters: int, guess=None, threads: int = 1) -> dict:
    """The C oracle (scalar port) on a bounded sample: `iters` full ICP iterations of the same workload from the same
    initial pose, kd-tree prebuilt (as the GPU's index is); `threads` > 1: the queries split over that many host threads."""
    import oracle
    tree = oracle.KdTree(model)
    pivot = 0.5 * (model.min(0).astype(np.float64) + model.max(0).astype(np.float64))
    T = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32)
    t0 = time.perf_counter()
    for _ in range(iters):
        S = oracle.icp_partial_sums(scene, tree, T, float(np.sqrt(np.finfo(np.float64).max)), pivot, threads)
        Tk = oracle.umeyama_from_sums(S, pivot)
        T = (Tk.astype(np.float64) @ T.astype(np.float64)).astype(np.float32)
    dt = time.perf_counter() - t0
    return {"value": iters / dt, "unit": "iterations/s", "cores": threads, "kind": "port",
            "sample": f"{iters} full ICP iterations (1-NN over all {len(scene)} scene points + SVD update) of the same "
                      f"workload from the same initial pose, kd-tree prebuilt; gcc -O3, {threads} thread(s); host has "
                      f"{os.cpu_count()} logical cores, {usable_cores()} usable by this process"}


if __name__ == "__main__":
    sys.exit(main())
