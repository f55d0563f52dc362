// icp_batch.hip — many small ICP registrations in one launch (ope_icp_run_batch, gfx950, wave64).
//
// At the size of the reference's fine stage (1-2 k key points a side, poseestimator.cpp:161-379) every launch of the
// single-run path (icp_kernels.hip) is a few waves long and most of the GPU idles: an iteration costs an accumulate launch,
// an update launch and, every check_every iterations, a host poll.  Here one workgroup owns one problem and runs its whole
// loop: search -> rejectors -> sums -> update lane, then the next iteration, with no kernel boundary, no host round trip and
// no communication between workgroups (no spin-wait, no co-residency requirement).  The update step is icp_update_lane
// itself (icp_update.hpp), the same code ope_icp_run runs; the search, the rejectors and the terms of the sums follow
// icp_accumulate_kernel operation for operation.  The sums of an iteration are added in a fixed order inside the workgroup
// (the wave's reduce-scatter of icp_sums.hpp, one LDS row per wave, one ordered pass over the rows), so a problem's result depends on its own
// inputs only: not on the run, the other problems of the batch or its position among them.
#include <cfloat>
#include <climits>
#include <cmath>
#include <limits>

#include "icp_update.hpp"
#include "icp_sums.hpp"   // add_query_sums: the terms and the wave's reduce-scatter, shared with icp_kernels.hip

namespace ope {

// Threads per workgroup: 512 (eight waves, two per SIMD) was faster than 256 at C1 size, DESIGN.md 4.6.
constexpr int kBatchBlock = 512;
constexpr int kBatchRows = kBatchBlock / 64;   // one LDS row of partial sums per wave, each slot with one writing lane
constexpr size_t kBatchMaxSrc = 65536;        // valid source points of one problem at most (larger runs belong to ope_icp_run)

struct BatchProblem {
  CloudView src;
  BvhView tgt;
  size_t hint_off;   // first of this problem's entries in the batch's start-leaf buffer (one per valid source point)
};
struct BatchOut {
  double F[16];
  double cur_mse;
  long long n_corr;
  int iterations, converged, state, pad_;
  double fit_sum, fit_n;
};

// One workgroup per problem.  MODE 0: 1-NN; MODE 2: normal shooting over the k nearest, list in KREG registers (the sizes
// launch_icp_accumulate uses).  NRM: normals are read (normal shooting, rejectors, point-to-plane).
template <int MODE, bool NRM, int KREG>
__global__ __launch_bounds__(kBatchBlock, 4) void icp_batch_kernel(const BatchProblem *__restrict__ probs, IcpState *__restrict__ states,
                                                                   uint32_t *__restrict__ hints, int max_it, double fit_range, int do_fit,
                                                                   BatchOut *__restrict__ out) {
  __shared__ IcpState s_st;
  // Per-run constants in LDS, re-read where they are used (held in registers across the walks they were spilled in the
  // accumulate kernel): F rows [0..11], pivot [12..14] (as float, like the accumulate kernel), start bound of the 1-NN walk [15]
  __shared__ __attribute__((aligned(16))) float s_const[16];
  __shared__ double s_rows[kBatchRows][kNumSumsMax];
  __shared__ double s_S[kNumSumsMax];
  __shared__ double s_fit[kBatchBlock / 64][2];
  __shared__ float s_stk[kMaxDepth + 1][kBatchBlock];
  float *stk = &s_stk[0][threadIdx.x];
  const BatchProblem pr = probs[blockIdx.x];
  const IcpState *st = states + blockIdx.x;   // (the run's parameters, read once through a uniform pointer)
  uint32_t *hint = hints + pr.hint_off;
  state_to_lds(&s_st, st);

  const double max_d2 = st->max_d2;
  float best0 = INFINITY;   // the accumulate kernel's start bound with a finite max_corr_dist
  if (max_d2 < 3.0e38) {
    float f = (float)max_d2;
    if ((double)f < max_d2) f = nextafterf(f, INFINITY);
    best0 = nextafterf(f, INFINITY);
  }
  const bool rej_sn = NRM && st->use_surface_normal_rej;
  const bool rej_so = NRM && st->use_self_occluded_rej;
  const bool p2p = NRM && st->estimator == OPE_EST_POINT_TO_PLANE_LLS;
  const int nsums = p2p ? kNumSumsMax : kNumSums;
  const double thr_sn = st->surface_normal_thr, thr_so = st->self_occluded_thr;
  const double max_dist_unsq = st->max_corr_dist;
  const int kk = st->k_normal_shooting;
  const uint32_t n_valid = pr.src.n_valid;
  const uint32_t lane_id = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  double *row = s_rows[wave];
  __syncthreads();

  for (int it = 0; it < max_it && s_st.done == 0; ++it) {
    if (threadIdx.x < 12) s_const[threadIdx.x] = s_st.Ff[threadIdx.x];
    else if (threadIdx.x < 15) s_const[threadIdx.x] = (float)s_st.pivot[threadIdx.x - 12];
    else if (threadIdx.x == 15) s_const[15] = best0;
    for (int k = threadIdx.x; k < kBatchRows * kNumSumsMax; k += kBatchBlock) (&s_rows[0][0])[k] = 0.0;
    __syncthreads();
    // 64 consecutive (Morton-ordered) queries per wave and trip: the loop bound is wave-uniform, every lane reaches the sums
    for (uint32_t base = wave * 64u; base < n_valid; base += kBatchBlock) {
      const uint32_t i = base + lane_id;
      const bool active = i < n_valid;
      lds_cfloat_ptr cst = (lds_cfloat_ptr)s_const;
      asm volatile("" : "+v"(cst));
      float F[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) F[k] = cst[k];
      const float4 s = pr.src.xyzw[active ? i : base];
      const float x = xform_row(F + 0, s.x, s.y, s.z);
      const float y = xform_row(F + 4, s.x, s.y, s.z);
      const float z = xform_row(F + 8, s.x, s.y, s.z);
      float nx = 0.f, ny = 0.f, nz = 0.f;
      if (NRM && pr.src.nrm != nullptr) {
        const float4 n4 = pr.src.nrm[active ? i : base];
        nx = rot_row(F + 0, n4.x, n4.y, n4.z);
        ny = rot_row(F + 4, n4.x, n4.y, n4.z);
        nz = rot_row(F + 8, n4.x, n4.y, n4.z);
      }
      // start at the leaf that held this query's nearest neighbour one iteration ago (0 = none yet): a start leaf never
      // changes what a walk finds
      const uint32_t h = active ? hint[i] : 0u;
      bool ok;
      float d2;
      uint32_t pos;
      if constexpr (MODE == 0) {
        NearestVisitor v{active ? cst[15] : -INFINITY, kNoPos, 0};
        if (active) bvh_traverse(pr.tgt, x, y, z, v, stk, kBatchBlock, h);
        if (active && v.leaf != h) hint[i] = v.leaf;
        const bool found = active && v.pos != kNoPos;
        ok = found && !((double)v.best > max_d2);
        d2 = found ? v.best : INFINITY;
        pos = found ? v.pos : 0;
      } else {
        KnnRegVisitor<KREG> v;
        v.init(active);
        if (active) bvh_traverse(pr.tgt, x, y, z, v, stk, kBatchBlock, h);
        if (active) hint[i] = v.leaf;
        // among the k nearest, the one with the smallest squared distance to the line (s, n)
        // (…normal_shooting_weighted.hpp:115-135; cross product in double)
        double min_dist = 1.79769313486231570815e308;
        d2 = INFINITY;
        pos = 0;
#pragma unroll
        for (int j = 0; j < KREG; ++j) {
          if (j < v.count && j < kk) {
            const float4 p = pr.tgt.pts[v.p[j]];
            const double vx = (double)__fsub_rn(p.x, x), vy = (double)__fsub_rn(p.y, y), vz = (double)__fsub_rn(p.z, z);
            const double cx = (double)ny * vz - (double)nz * vy;
            const double cy = (double)nz * vx - (double)nx * vz;
            const double cz = (double)nx * vy - (double)ny * vx;
            const double dist = cx * cx + cy * cy + cz * cz;
            if (dist < min_dist) { min_dist = dist; d2 = v.d[j]; pos = v.p[j]; }
          }
        }
        // quirk Q2: squared line distance against the UNSQUARED max distance (:136)
        ok = active && v.count > 0 && !(min_dist > max_dist_unsq);
      }
      if (NRM && ok && rej_sn) {
        const float4 tn = pr.tgt.nrm[pos];
        const float score = __fadd_rn(__fadd_rn(__fmul_rn(nx, tn.x), __fmul_rn(ny, tn.y)), __fmul_rn(nz, tn.z));
        ok = (double)score > thr_sn;
      }
      if (NRM && ok && rej_so) {
        const double sl = sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
        const double score = (double)nx * (-(double)x / sl) + (double)ny * (-(double)y / sl) + (double)nz * (-(double)z / sl);
        ok = score > thr_so;
      }
      // no atomics: the wave's reduce-scatter leaves one writing lane per slot of its row, so the order of every addition is fixed
      add_query_sums<NRM, false>(row, (lds_cfloat_ptr)s_const, lane_id, ok, p2p, x, y, z, pr.tgt.pts[ok ? pos : 0],
                                 (NRM && p2p) ? pr.tgt.nrm[ok ? pos : 0] : make_float4(0.f, 0.f, 0.f, 0.f), d2);
    }
    __syncthreads();
    if ((int)threadIdx.x < nsums) {   // rows in a fixed order
      double v = 0.0;
      for (int r = 0; r < kBatchRows; ++r) v += s_rows[r][threadIdx.x];
      s_S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) icp_update_lane(&s_st, s_S);
    __syncthreads();
  }

  // getFitnessScore(max_range) of the final transform (fitness_kernel's semantics): 1-NN from +inf, d2 <= max_range counted
  double fsum = 0.0, fcnt = 0.0;
  if (do_fit) {
    if (threadIdx.x < 12) s_const[threadIdx.x] = s_st.Ff[threadIdx.x];
    __syncthreads();
    for (uint32_t base = wave * 64u; base < n_valid; base += kBatchBlock) {
      const uint32_t i = base + lane_id;
      const bool active = i < n_valid;
      lds_cfloat_ptr cst = (lds_cfloat_ptr)s_const;
      asm volatile("" : "+v"(cst));
      float F[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) F[k] = cst[k];
      const float4 s = pr.src.xyzw[active ? i : base];
      const float x = xform_row(F + 0, s.x, s.y, s.z);
      const float y = xform_row(F + 4, s.x, s.y, s.z);
      const float z = xform_row(F + 8, s.x, s.y, s.z);
      NearestVisitor v{active ? INFINITY : -INFINITY, kNoPos, 0};
      if (active) bvh_traverse(pr.tgt, x, y, z, v, stk, kBatchBlock, hint[i]);
      if (active && v.pos != kNoPos && (double)v.best <= fit_range) { fsum += (double)v.best; fcnt += 1.0; }
    }
    fsum = wave_sum(fsum);
    fcnt = wave_sum(fcnt);
    if (lane_id == 0) { s_fit[wave][0] = fsum; s_fit[wave][1] = fcnt; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    BatchOut &o = out[blockIdx.x];
    for (int k = 0; k < 16; ++k) o.F[k] = s_st.F[k];
    o.cur_mse = s_st.cur_mse;
    o.n_corr = s_st.n_corr;
    o.iterations = s_st.iterations;
    o.converged = s_st.converged;
    o.state = s_st.state;
    o.pad_ = 0;
    double a = 0.0, b = 0.0;
    if (do_fit)
      for (int w = 0; w < kBatchBlock / 64; ++w) { a += s_fit[w][0]; b += s_fit[w][1]; }
    o.fit_sum = a;
    o.fit_n = b;
  }
}

static void launch_icp_batch(hipStream_t stream, int n, int mode, bool nrm, int k, const BatchProblem *probs, IcpState *states,
                             uint32_t *hints, int max_it, double fit_range, int do_fit, BatchOut *out) {
#define OPE_LAUNCH_BATCH(M, N, KR) \
  hipLaunchKernelGGL((icp_batch_kernel<M, N, KR>), dim3(n), dim3(kBatchBlock), 0, stream, probs, states, hints, max_it, fit_range, do_fit, out)
  if (mode == OPE_CORR_NEAREST) {
    if (nrm) OPE_LAUNCH_BATCH(0, true, 4);
    else OPE_LAUNCH_BATCH(0, false, 4);
    return;
  }
  // normal shooting: the register-list sizes of launch_icp_accumulate
  if (k == 10) OPE_LAUNCH_BATCH(2, true, 10);
  else if (k <= 4) OPE_LAUNCH_BATCH(2, true, 4);
  else if (k <= 8) OPE_LAUNCH_BATCH(2, true, 8);
  else if (k <= 12) OPE_LAUNCH_BATCH(2, true, 12);
  else if (k <= 16) OPE_LAUNCH_BATCH(2, true, 16);
  else if (k <= 20) OPE_LAUNCH_BATCH(2, true, 20);
  else if (k <= 24) OPE_LAUNCH_BATCH(2, true, 24);
  else if (k <= 28) OPE_LAUNCH_BATCH(2, true, 28);
  else OPE_LAUNCH_BATCH(2, true, 32);
#undef OPE_LAUNCH_BATCH
}

}  // namespace ope

using namespace ope;

extern "C" int ope_icp_run_batch(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                                 const ope_icp_params *params, double fitness_max_range, ope_icp_batch_result *out) {
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: bad argument");
  if (n == 0) return OPE_OK;
  if (!src || !tgt || !out) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: bad argument");
  if (n > (size_t)INT_MAX) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: too many problems");
  ope_icp_params p;
  ope_icp_default_params(&p);
  if (params) p = *params;
  { const int rc = icp_batch_check_params(ctx, p); if (rc != OPE_OK) return rc; }
  const bool need_src_nrm = p.corr_mode == OPE_CORR_NORMAL_SHOOTING || p.use_surface_normal_rej || p.use_self_occluded_rej;
  const bool p2p = p.estimator == OPE_EST_POINT_TO_PLANE_LLS;
  for (size_t i = 0; i < n; ++i) {
    const std::string at = " (problem " + std::to_string(i) + ")";
    if (!src[i]) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: no source cloud" + at);
    if (!tgt[i]) return set_err(ctx, OPE_EEMPTY, "ope_icp_run_batch: no input target dataset was given" + at);
    if (need_src_nrm && !src[i]->d_nrm) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: source normals required but absent" + at);
    if (p2p && !tgt[i]->d_nrm) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: the point-to-plane estimator needs target normals" + at);
    if (p.use_surface_normal_rej && !tgt[i]->d_nrm) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: target normals required" + at);
    if (src[i]->n_valid > kBatchMaxSrc)
      return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: more than 65536 valid source points (use ope_icp_run)" + at);
    if (ctx->n_fixed > 0 && ctx->fixed_src == src[i])
      return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: fixed correspondences are set for this source cloud" + at);
  }
  return icp_batch_core(ctx, n, src, tgt, guesses, p, fitness_max_range, out);
}

int ope::icp_batch_check_params(ope_ctx *ctx, const ope_icp_params &p) {
  if (ctx->nccl_comm != nullptr || ctx->p2p_ok || ctx->p2p_broken)
    return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: not on a context with a communicator (batched problems are not sharded)");
  if (ctx->n_grej > 0)
    return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: global correspondence rejectors are set (ope_icp_set_global_rejectors): the batched and tracked loops do not run them");
  if (p.use_reciprocal) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: reciprocal correspondences are not supported");
  if (p.estimator == OPE_EST_POINT_TO_PLANE_LM) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: the LM estimator is not supported");
  if (p.estimator != OPE_EST_SVD && p.estimator != OPE_EST_POINT_TO_PLANE_LLS) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: unknown estimator");
  if (p.corr_mode != OPE_CORR_NEAREST && p.corr_mode != OPE_CORR_NORMAL_SHOOTING) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: unknown corr_mode");
  if (p.corr_mode == OPE_CORR_NORMAL_SHOOTING && (p.k_normal_shooting < 1 || p.k_normal_shooting > 32))
    return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: 1 <= k_normal_shooting <= 32");
  return OPE_OK;
}

// problems that passed ope_icp_run_batch's checks: ope_icp_run_batch and ope_final_pose_batch (its fine stage, on clouds and trees
// that live in that call's buffers)
int ope::icp_batch_core(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                        const ope_icp_params &p, double fitness_max_range, ope_icp_batch_result *out) {
  if (n == 0) return OPE_OK;
  const bool need_src_nrm = p.corr_mode == OPE_CORR_NORMAL_SHOOTING || p.use_surface_normal_rej || p.use_self_occluded_rej;
  const bool p2p = p.estimator == OPE_EST_POINT_TO_PLANE_LLS;
  size_t n_hints = 0;
  for (size_t i = 0; i < n; ++i) n_hints += src[i]->n_valid;
  OPE_HIP(ctx, hipSetDevice(ctx->device));

  // one temporary block: [problems | states | results | start leaves]; the first two go up in one copy
  auto up8 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t b_prob = up8(sizeof(BatchProblem) * n), b_state = up8(sizeof(IcpState) * n), b_out = up8(sizeof(BatchOut) * n);
  const size_t b_hint = sizeof(uint32_t) * std::max<size_t>(n_hints, 1);
  std::vector<unsigned char> host(b_prob + b_state);
  BatchProblem *hp = reinterpret_cast<BatchProblem *>(host.data());
  IcpState *hs = reinterpret_cast<IcpState *>(host.data() + b_prob);
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    hp[i] = BatchProblem{src[i]->view(), tgt[i]->view(), off};
    off += src[i]->n_valid;
    // the state ope_icp_begin starts a run with (no skip certificates: the batch has no host that could see them asked for)
    icp_state_init(hs + i, src[i], tgt[i], guesses ? guesses + 16 * i : nullptr, p, false, false);
  }
  unsigned char *blk = nullptr;
  OPE_HIP(ctx, tmp_malloc(ctx->stream, (void **)&blk, b_prob + b_state + b_out + b_hint));
  struct FreeBlk { hipStream_t s; void *p; ~FreeBlk() { tmp_free(s, p); } } free_blk{ctx->stream, blk};
  BatchProblem *d_prob = reinterpret_cast<BatchProblem *>(blk);
  IcpState *d_state = reinterpret_cast<IcpState *>(blk + b_prob);
  BatchOut *d_out = reinterpret_cast<BatchOut *>(blk + b_prob + b_state);
  uint32_t *d_hint = reinterpret_cast<uint32_t *>(blk + b_prob + b_state + b_out);
  OPE_HIP(ctx, h2d_copy(ctx->stream, blk, host.data(), host.size()));
  OPE_HIP(ctx, hipMemsetAsync(d_hint, 0, b_hint, ctx->stream));
  const bool nrm = need_src_nrm || p2p;
  const bool do_fit = fitness_max_range >= 0.0;
  launch_icp_batch(ctx->stream, (int)n, p.corr_mode, nrm, p.k_normal_shooting, d_prob, d_state, d_hint, std::max(p.max_iterations, 1),
                   do_fit ? fitness_max_range : 0.0, do_fit ? 1 : 0, d_out);
  OPE_HIP(ctx, hipGetLastError());
  std::vector<BatchOut> ho(n);
  OPE_HIP(ctx, hipMemcpyAsync(ho.data(), d_out, sizeof(BatchOut) * n, hipMemcpyDeviceToHost, ctx->stream));
  OPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i) {
    const BatchOut &o = ho[i];
    ope_icp_batch_result &r = out[i];
    r.result.iterations = o.iterations;
    r.result.converged = o.converged;
    r.result.state = o.state;
    r.result.last_mse = o.cur_mse;
    r.result.n_corr = o.n_corr;
    // getAlignStrength of a single-rank run (api.hip, fill_result): n_corr / (N_src + N_tgt), full cloud sizes
    const double denom = (double)((int64_t)src[i]->n + (int64_t)tgt[i]->n_total);
    r.result.align_strength = denom > 0 ? (double)o.n_corr / denom : 0.0;
    for (int k = 0; k < 16; ++k) r.T[k] = (float)o.F[k];
    if (do_fit) {
      r.fitness = o.fit_n > 0 ? o.fit_sum / o.fit_n : std::numeric_limits<double>::max();
      r.fitness_n = (int64_t)o.fit_n;
    } else {
      r.fitness = std::numeric_limits<double>::max();
      r.fitness_n = -1;
    }
  }
  return OPE_OK;
}
