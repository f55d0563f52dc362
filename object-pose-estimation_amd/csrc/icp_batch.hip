// icp_batch.hip — many small ICP registrations in one launch (ope_icp_run_batch, gfx950, wave64).
//
// At the size of the reference's fine stage (1-2 k key points a side, poseestimator.cpp:161-379) every launch of the
// single-run path (icp_kernels.hip) is a few waves long and most of the GPU idles: an iteration costs an accumulate launch,
// an update launch and, every check_every iterations, a host poll.  Here one workgroup owns one problem and runs its whole
// loop: search -> rejectors -> sums -> update lane, then the next iteration, with no kernel boundary, no host round trip and
// no communication between workgroups (no spin-wait, no co-residency requirement).  The update step is icp_update_lane
// itself (icp_update.hpp), the same code ope_icp_run runs; the per-query rules of the search and the per-pair rejectors are those
// of icp_pair.hpp, the terms of the sums those of icp_sums.hpp, as in icp_accumulate_kernel.  The sums of an iteration are added in a fixed order inside the workgroup
// (the wave's reduce-scatter of icp_sums.hpp, one LDS row per wave, one ordered pass over the rows), so a problem's result depends on its own
// inputs only: not on the run, the other problems of the batch or its position among them.
// ope_icp_run_batch_rejectors runs the same body with a list of global rejectors between the search and the sums (the staged
// instantiations, below).
#include <cfloat>
#include <climits>
#include <cmath>
#include <limits>

#include "icp_update.hpp"
#include "icp_sums.hpp"   // add_query_sums: the terms and the wave's reduce-scatter, shared with icp_kernels.hip
#include "icp_pair.hpp"   // the per-query rules, shared with icp_kernels.hip
#include "grej_rules.hpp" // the rules of the global rejectors, shared with global_rejectors.hip

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

// ---- The global rejectors of a list (ope.h: median distance, one to one, var trimmed) inside the problem's workgroup: the staged
// instantiations (ope_icp_run_batch_rejectors).  The search pass stores every query's outcome in the problem's slice of the call's
// temporary block (pos: the matched point's position in the index, bit 31 = the pair is alive; d2: its distance field) and adds
// nothing; the rejectors clear bit 31 of the pairs they drop, in the order of the list; a second pass over the same queries, same
// trip, wave and lane, adds the survivors' sums.  Between the passes the walk stacks (s_stk) are idle: they hold the histograms of
// the median selection, the one-to-one words and the keys of the var-trimmed sort while those fit, else the slice does.  Nothing
// here uses a floating-point atomic or depends on the order in which waves run: counts and minima are integer, the two fp64
// reductions (head sum, first minimum of FRMS) go over lanes, then waves, in a fixed order.
constexpr uint32_t kStageLdsWords = (uint32_t)(kMaxDepth + 1) * kBatchBlock;   // the walk stacks: 10 752 words
constexpr uint32_t kStageSortLds = 8192;                 // var trimmed: valid source points whose keys sort in LDS; more sort in the slice
constexpr uint32_t kStageOtoLds = kStageLdsWords / 2;    // one to one: target points whose 64-bit words fit LDS (5 376); more use the slice
constexpr uint32_t kStageAlive = 0x80000000u;
static_assert(kStageSortLds <= kStageLdsWords && (kStageSortLds & (kStageSortLds - 1)) == 0, "the in-LDS sort is a power of two inside the stacks");

struct BatchStageProblem {   // offsets in 4-byte words into BatchStage::work
  size_t pos_off, d2_off;    // n_valid entries each
  size_t keys_off;           // the padded keys of a sort too large for LDS
  size_t words_off;          // (even) the one-to-one words of a target too large for LDS
  size_t pair_off;           // first entry of this problem in the pair outputs (ORIGINAL source indices)
};
struct BatchStage {
  const BatchStageProblem *probs;
  uint32_t *work;
  const ope_global_rejector *list;
  GrejStat *stats;   // n problems x OPE_GREJ_MAX
  int32_t *pair_match;     // or null
  float *pair_d2;          // or null
  int n_list;
};

// The problem's own pointers, the list and the stage's small reductions, in LDS: read where they are used (like s_const), they
// cost the walks no register.
struct BatchStageLds {
  uint32_t *pos;
  float *d2;
  uint32_t *keys;
  unsigned long long *words;
  GrejStat *stats;
  int32_t *pair_match;
  float *pair_d2;
  ope_global_rejector list[OPE_GREJ_MAX];
  GrejStat stat[OPE_GREJ_MAX];   // as the last iteration that searched left them
  double dred[2][kBatchRows];
  uint32_t jred[kBatchRows], cnt[kBatchRows], sel[4];
  int n_list, searched;
  float best0;   // the start bound of the 1-NN walk (a per-run constant the loop would otherwise carry in a register)
};
typedef __attribute__((address_space(3))) BatchStageLds *lds_stage_ptr;
typedef __attribute__((address_space(3))) uint32_t *lds_u32_ptr;

// the sum of c over the workgroup (integers: any order gives it); s_cnt: one word per wave
__device__ __forceinline__ uint32_t stage_count(uint32_t c, uint32_t *s_cnt) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
  __syncthreads();   // (the words may still be read from the count before)
  if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  uint32_t total = 0u;
#pragma unroll
  for (int w = 0; w < kBatchRows; ++w) total += s_cnt[w];
  return total;
}

// Median distance (grej_rules.hpp) over the alive pairs: each pass's histogram in LDS, scanned by wave 0.  s_sel = {prefix, rank within it, m}.
__device__ __forceinline__ void stage_median(uint32_t *g_pos, const float *g_d2, uint32_t nv, double factor, uint32_t *hist, uint32_t *s_cnt,
                                             uint32_t *s_sel, GrejStat *stat) {
  const uint32_t lane = threadIdx.x & 63u;
  if (threadIdx.x == 0) { s_sel[0] = 0u; s_sel[1] = 0u; s_sel[2] = 0u; }
  for (int pass = 0; pass < 4; ++pass) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t prefix = s_sel[0];
    for (uint32_t i = threadIdx.x; i < nv; i += kBatchBlock) {
      if (!(g_pos[i] & kStageAlive)) continue;
      uint32_t digit;
      if (grej_median_digit(__float_as_uint(g_d2[i]), pass, prefix, digit)) atomicAdd(&hist[digit], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // lane l owns digits 4l .. 4l + 3
      const uint32_t c[4] = {hist[4 * lane], hist[4 * lane + 1], hist[4 * lane + 2], hist[4 * lane + 3]};
      const uint32_t tot = c[0] + c[1] + c[2] + c[3];
      uint32_t incl = tot;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
        if ((int)lane >= off) incl += v;
      }
      const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
      const uint32_t rank = pass == 0 ? grej_median_rank(total) : s_sel[1];
      uint32_t d, r;
      if (grej_digit_pick(c, incl, rank, d, r)) {   // one lane at most
        s_sel[0] = (prefix << 8) | (4u * lane + d);
        s_sel[1] = r;
      }
      if (pass == 0 && lane == 0u) s_sel[2] = total;
    }
    __syncthreads();
  }
  const uint32_t m = s_sel[2];
  const GrejMedianRule rule(m, s_sel[0], factor);
  uint32_t kept = 0u;
  for (uint32_t i = threadIdx.x; i < nv; i += kBatchBlock) {
    const uint32_t p = g_pos[i];
    if (!(p & kStageAlive)) continue;
    const bool k = rule.keep(g_d2[i]);
    if (!k) g_pos[i] = p & ~kStageAlive;
    kept += k ? 1u : 0u;
  }
  const uint32_t n_out = stage_count(kept, s_cnt);
  if (threadIdx.x == 0) { stat->n_in = m; stat->n_out = n_out; stat->threshold = rule.threshold(); stat->ratio = grej_nan(); }
}

// One to one (grej_rules.hpp: grej_word of the distance field and the ORIGINAL query index) over the alive pairs; the target point
// is named by its position in the index, which is one to one with its original index.
__device__ __forceinline__ void stage_one_to_one(uint32_t *g_pos, const float *g_d2, const float4 *__restrict__ src_xyzw, uint32_t nv, uint32_t n_tgt,
                                                 unsigned long long *words, uint32_t *s_cnt, GrejStat *stat) {
  for (uint32_t t = threadIdx.x; t < n_tgt; t += kBatchBlock) words[t] = ~0ull;
  __syncthreads();
  uint32_t cnt = 0u;
  for (uint32_t i = threadIdx.x; i < nv; i += kBatchBlock) {
    const uint32_t p = g_pos[i];
    if (!(p & kStageAlive)) continue;
    ++cnt;
    const unsigned long long word = grej_word(g_d2[i], __float_as_int(src_xyzw[i].w));
    atomicMin(words + (p & ~kStageAlive), word);
  }
  __syncthreads();
  uint32_t kept = 0u;
  for (uint32_t i = threadIdx.x; i < nv; i += kBatchBlock) {
    const uint32_t p = g_pos[i];
    if (!(p & kStageAlive)) continue;
    const unsigned long long word = grej_word(g_d2[i], __float_as_int(src_xyzw[i].w));
    const bool k = words[p & ~kStageAlive] == word;
    if (!k) g_pos[i] = p & ~kStageAlive;
    kept += k ? 1u : 0u;
  }
  const uint32_t n_in = stage_count(cnt, s_cnt);
  const uint32_t n_out = stage_count(kept, s_cnt);
  if (threadIdx.x == 0) { stat->n_in = n_in; stat->n_out = n_out; stat->threshold = grej_nan(); stat->ratio = grej_nan(); }
}

// keys[0 .. n) ascending, n a power of two >= 2: the bitonic network, one compare-exchange per thread and step
__device__ __forceinline__ void stage_bitonic(uint32_t *keys, uint32_t n) {
  for (uint32_t k = 2u; k <= n; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (n >> 1); t += kBatchBlock) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
        const uint32_t a = keys[i], b = keys[p];
        if ((a > b) == ((i & k) == 0u)) { keys[i] = b; keys[p] = a; }
      }
      __syncthreads();
    }
  }
}

// Var trimmed (grej_rules.hpp): the alive pairs' keys ascending (the others and the padding keyed to the top), then the head sum L,
// FRMS_j and its first minimum over the lanes, then the waves, and the keep.  n2: the power of two the keys are padded to.
__device__ __forceinline__ void stage_var_trimmed(uint32_t *g_pos, const float *g_d2, uint32_t nv, uint32_t n2, double min_ratio, double max_ratio,
                                                  uint32_t *keys, uint32_t *s_cnt, double (*s_dred)[kBatchRows], uint32_t *s_jred,
                                                  GrejStat *stat) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t cnt = 0u;
  for (uint32_t t = threadIdx.x; t < n2; t += kBatchBlock) {
    uint32_t key = 0xffffffffu;
    if (t < nv && (g_pos[t] & kStageAlive)) { key = __float_as_uint(g_d2[t]); ++cnt; }
    keys[t] = key;
  }
  const uint32_t m = stage_count(cnt, s_cnt);   // (its barriers also publish the keys)
  stage_bitonic(keys, n2);
  uint32_t lo, hi;
  grej_vt_range(m, min_ratio, max_ratio, lo, hi);
  double acc = 0.0;
  for (uint32_t j = threadIdx.x; j < lo; j += kBatchBlock) acc += (double)__uint_as_float(keys[j]);
  acc = wave_sum(acc);
  double best = std::numeric_limits<double>::infinity();
  uint32_t best_j = 0xffffffffu;
  if (lane == 0u) s_dred[0][wave] = acc;
  __syncthreads();
  double L = 0.0;
#pragma unroll
  for (int w = 0; w < kBatchRows; ++w) L += s_dred[0][w];
  for (uint32_t j = lo + threadIdx.x; j < hi; j += kBatchBlock) {
    const double frms = grej_vt_frms(j, m, keys[j], L);
    if (frms < best) { best = frms; best_j = j; }
  }
  // grej_argmin_before over the lanes, then over the waves
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double v2 = __shfl_xor(best, off, 64);
    const uint32_t j2 = (uint32_t)__shfl_xor((int)best_j, off, 64);
    if (grej_argmin_before(v2, j2, best, best_j)) { best = v2; best_j = j2; }
  }
  if (lane == 0u) { s_dred[1][wave] = best; s_jred[wave] = best_j; }
  __syncthreads();
  best = s_dred[1][0];
  best_j = s_jred[0];
#pragma unroll
  for (int w = 1; w < kBatchRows; ++w) {
    const double v2 = s_dred[1][w];
    const uint32_t j2 = s_jred[w];
    if (grej_argmin_before(v2, j2, best, best_j)) { best = v2; best_j = j2; }
  }
  const GrejVtRule rule(m, lo, hi, best_j, keys);
  uint32_t kept = 0u;
  for (uint32_t i = threadIdx.x; i < nv; i += kBatchBlock) {
    const uint32_t p = g_pos[i];
    if (!(p & kStageAlive)) continue;
    const bool k = rule.keep(g_d2[i]);
    if (!k) g_pos[i] = p & ~kStageAlive;
    kept += k ? 1u : 0u;
  }
  const uint32_t n_out = stage_count(kept, s_cnt);   // (its barriers also end the reads of the keys)
  if (threadIdx.x == 0) { stat->n_in = m; stat->n_out = n_out; stat->threshold = rule.trimmed; stat->ratio = (double)rule.ratio; }
}

// The list over the pairs the search pass stored, by the whole workgroup.  Out of line: the kernel's walks keep the registers they
// have without a stage.  lds: the walk stacks (kStageLdsWords words), idle between the passes.
__device__ __noinline__ void stage_apply(lds_stage_ptr sl3, lds_u32_ptr lds3, const float4 *__restrict__ src_xyzw, uint32_t nv, uint32_t n_tgt) {
  BatchStageLds *sl = (BatchStageLds *)sl3;
  uint32_t *lds = (uint32_t *)lds3;
  uint32_t *const g_pos = sl->pos;
  float *const g_d2 = sl->d2;
  const int n_list = sl->n_list;
  for (int k = 0; k < n_list; ++k) {
    const ope_global_rejector rj = sl->list[k];
    if (rj.kind == OPE_GREJ_MEDIAN_DISTANCE) {
      stage_median(g_pos, g_d2, nv, rj.factor, lds, sl->cnt, sl->sel, &sl->stat[k]);
    } else if (rj.kind == OPE_GREJ_ONE_TO_ONE) {
      if (n_tgt <= kStageOtoLds) stage_one_to_one(g_pos, g_d2, src_xyzw, nv, n_tgt, reinterpret_cast<unsigned long long *>(lds), sl->cnt, &sl->stat[k]);
      else stage_one_to_one(g_pos, g_d2, src_xyzw, nv, n_tgt, sl->words, sl->cnt, &sl->stat[k]);
    } else {
      uint32_t n2 = 2u;
      while (n2 < nv) n2 <<= 1;
      if (nv <= kStageSortLds) stage_var_trimmed(g_pos, g_d2, nv, n2, rj.min_ratio, rj.max_ratio, lds, sl->cnt, sl->dred, sl->jred, &sl->stat[k]);
      else stage_var_trimmed(g_pos, g_d2, nv, n2, rj.min_ratio, rj.max_ratio, sl->keys, sl->cnt, sl->dred, sl->jred, &sl->stat[k]);
    }
    __syncthreads();
  }
}

// One workgroup per problem.  MODE 0: 1-NN; MODE 2: normal shooting over the k nearest, list in KREG registers (the sizes
// launch_icp_accumulate uses).  NRM: normals are read (normal shooting, rejectors, point-to-plane).
// STAGED: the search pass stores its pairs, the list of `stg` runs over them and a second pass adds the survivors (see above).
template <int MODE, bool NRM, int KREG, bool STAGED>
__device__ __forceinline__ void icp_batch_body(const BatchProblem *__restrict__ probs, IcpState *__restrict__ states, uint32_t *__restrict__ hints,
                                               int max_it, double fit_range, int do_fit, BatchOut *__restrict__ out, const BatchStage stg) {
  __shared__ IcpState s_st;
  // Per-run constants in LDS, re-read where they are used (held in registers across the walks they were spilled in the
  // accumulate kernel): F rows [0..11], pivot [12..14] (as float, like the accumulate kernel), start bound of the 1-NN walk [15]
  __shared__ __attribute__((aligned(16))) float s_const[16];
  __shared__ double s_rows[kBatchRows][kNumSumsMax];
  __shared__ double s_S[kNumSumsMax];
  __shared__ double s_fit[kBatchBlock / 64][2];
  __shared__ __attribute__((aligned(STAGED ? 16 : 4))) float s_stk[kMaxDepth + 1][kBatchBlock];
  // the staged instantiations' own words (the others use none of them)
  __shared__ BatchStageLds s_stg;
  float *stk = &s_stk[0][threadIdx.x];
  const BatchProblem pr = probs[blockIdx.x];
  const IcpState *st = states + blockIdx.x;   // (the run's parameters, read once through a uniform pointer)
  uint32_t *hint = hints + pr.hint_off;
  state_to_lds(&s_st, st);

  const double max_d2 = st->max_d2;
  const float best0 = pair_start_bound(max_d2);
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
  if constexpr (STAGED) {
    if ((int)threadIdx.x < OPE_GREJ_MAX) {
      s_stg.stat[threadIdx.x] = grej_stat_none();
      if ((int)threadIdx.x < stg.n_list) s_stg.list[threadIdx.x] = stg.list[threadIdx.x];
    }
    if (threadIdx.x == 0) {
      const BatchStageProblem sp = stg.probs[blockIdx.x];
      s_stg.pos = stg.work + sp.pos_off;
      s_stg.d2 = reinterpret_cast<float *>(stg.work + sp.d2_off);
      s_stg.keys = stg.work + sp.keys_off;
      s_stg.words = reinterpret_cast<unsigned long long *>(stg.work + sp.words_off);
      s_stg.stats = stg.stats + (size_t)blockIdx.x * OPE_GREJ_MAX;
      s_stg.pair_match = stg.pair_match != nullptr ? stg.pair_match + sp.pair_off : nullptr;
      s_stg.pair_d2 = stg.pair_d2 != nullptr ? stg.pair_d2 + sp.pair_off : nullptr;
      s_stg.n_list = stg.n_list;
      s_stg.searched = 0;
      s_stg.best0 = best0;
    }
  }
  __syncthreads();

  for (int it = 0; it < max_it && s_st.done == 0; ++it) {
    if (STAGED && threadIdx.x == 0) s_stg.searched = 1;
    if (threadIdx.x < 12) s_const[threadIdx.x] = s_st.Ff[threadIdx.x];
    else if (threadIdx.x < 15) s_const[threadIdx.x] = (float)s_st.pivot[threadIdx.x - 12];
    else if (threadIdx.x == 15) s_const[15] = STAGED ? s_stg.best0 : best0;
    for (int k = threadIdx.x; k < kBatchRows * kNumSumsMax; k += kBatchBlock) (&s_rows[0][0])[k] = 0.0;
    __syncthreads();
    // 64 consecutive (Morton-ordered) queries per wave and trip: the loop bound is wave-uniform, every lane reaches the sums
    for (uint32_t base = wave * 64u; base < n_valid; base += kBatchBlock) {
      const uint32_t i = base + lane_id;
      const bool active = i < n_valid;
      const lds_cfloat_ptr cst = pair_consts(s_const);
      const MovedQuery q = pair_moved_query<NRM>(cst, pr.src, active ? i : base);
      const float x = q.x, y = q.y, z = q.z, nx = q.nx, ny = q.ny, nz = q.nz;
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
        // among the k nearest, the one with the smallest squared distance to the line (s, n), the first on ties
        // (…normal_shooting_weighted.hpp:115-135).  The same loop as icp_accumulate_kernel's: as one function it made every
        // normal-shooting instantiation spill more scalar registers
        double min_dist = 1.79769313486231570815e308;
        d2 = INFINITY;
        pos = 0;
#pragma unroll
        for (int j = 0; j < KREG; ++j) {
          if (j < v.count && j < kk) {
            const double dist = pair_line_dist2(pr.tgt.pts[v.p[j]], x, y, z, nx, ny, nz);
            if (dist < min_dist) { min_dist = dist; d2 = v.d[j]; pos = v.p[j]; }
          }
        }
        ok = active && pair_ns_ok(v.count, min_dist, max_dist_unsq);
      }
      if (NRM && ok && rej_sn) ok = pair_passes_surface_normal(nx, ny, nz, pr.tgt.nrm[pos], thr_sn);
      if (NRM && ok && rej_so) ok = pair_passes_self_occlusion(x, y, z, nx, ny, nz, thr_so);
      if constexpr (STAGED) {
        lds_stage_ptr sl = (lds_stage_ptr)&s_stg;
        asm volatile("" : "+v"(sl));
        if (active) { sl->pos[i] = pos | (ok ? kStageAlive : 0u); sl->d2[i] = d2; }
      } else {
        // no atomics: the wave's reduce-scatter leaves one writing lane per slot of its row, so the order of every addition is fixed
        add_query_sums<NRM, false>(row, (lds_cfloat_ptr)s_const, lane_id, ok, p2p, x, y, z, pr.tgt.pts[ok ? pos : 0],
                                   (NRM && p2p) ? pr.tgt.nrm[ok ? pos : 0] : make_float4(0.f, 0.f, 0.f, 0.f), d2);
      }
    }
    __syncthreads();
    if constexpr (STAGED) {
      stage_apply((lds_stage_ptr)&s_stg, (lds_u32_ptr)&s_stk[0][0], pr.src.xyzw, n_valid, pr.tgt.n);
      const uint32_t *const g_pos = s_stg.pos;
      const float *const g_d2 = s_stg.d2;
      // the survivors' sums: the same queries on the same trip, wave and lane as the search pass, moved by the same fp32 rows
      for (uint32_t base = wave * 64u; base < n_valid; base += kBatchBlock) {
        const uint32_t i = base + lane_id;
        const bool active = i < n_valid;
        const MovedQuery q = pair_moved_query<false>(pair_consts(s_const), pr.src, active ? i : base);
        const float x = q.x, y = q.y, z = q.z;
        const uint32_t p = active ? g_pos[i] : 0u;
        const bool ok = (p & kStageAlive) != 0u;
        const float d2 = active ? g_d2[i] : INFINITY;
        add_query_sums<NRM, false>(row, (lds_cfloat_ptr)s_const, lane_id, ok, false, x, y, z, pr.tgt.pts[ok ? (p & ~kStageAlive) : 0u],
                                   make_float4(0.f, 0.f, 0.f, 0.f), d2);
      }
      __syncthreads();
    }
    if ((int)threadIdx.x < nsums) {   // rows in a fixed order
      double v = 0.0;
      for (int r = 0; r < kBatchRows; ++r) v += s_rows[r][threadIdx.x];
      s_S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) icp_update_lane(&s_st, s_S);
    __syncthreads();
  }

  // getFitnessScore(max_range) of the final transform (fitness_kernel's semantics): 1-NN from +inf, d2 <= max_range counted.
  // (The query is moved on this pass's own text: through pair_moved_query the large normal-shooting instantiations spill more.)
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
  if constexpr (STAGED) {
    // what the last iteration that searched left: the statistics, and the surviving pairs by ORIGINAL source index (the host has
    // set every entry to "no pair")
    __syncthreads();
    if ((int)threadIdx.x < s_stg.n_list) s_stg.stats[threadIdx.x] = s_stg.stat[threadIdx.x];
    int32_t *const pair_match = s_stg.pair_match;
    float *const pair_d2 = s_stg.pair_d2;
    if (s_stg.searched && (pair_match != nullptr || pair_d2 != nullptr)) {
      const uint32_t *g_pos = s_stg.pos;
      const float *g_d2 = s_stg.d2;
      for (uint32_t i = threadIdx.x; i < n_valid; i += kBatchBlock) {
        const uint32_t p = g_pos[i];
        if (!(p & kStageAlive)) continue;
        const uint32_t o = __float_as_uint(pr.src.xyzw[i].w);
        if (o >= pr.src.n) continue;
        if (pair_match != nullptr) pair_match[o] = __float_as_int(pr.tgt.pts[p & ~kStageAlive].w);
        if (pair_d2 != nullptr) pair_d2[o] = g_d2[i];
      }
    }
  }
}

template <int MODE, bool NRM, int KREG>
__global__ __launch_bounds__(kBatchBlock, 4) void icp_batch_kernel(const BatchProblem *__restrict__ probs, IcpState *__restrict__ states,
                                                                   uint32_t *__restrict__ hints, int max_it, double fit_range, int do_fit,
                                                                   BatchOut *__restrict__ out) {
  icp_batch_body<MODE, NRM, KREG, false>(probs, states, hints, max_it, fit_range, do_fit, out, BatchStage{});
}

// the staged instantiations (ope_icp_run_batch_rejectors): the same body with the list of `stg` between search and sums
template <int MODE, bool NRM, int KREG>
__global__ __launch_bounds__(kBatchBlock, 4) void icp_batch_rejectors_kernel(const BatchProblem *__restrict__ probs, IcpState *__restrict__ states,
                                                                             uint32_t *__restrict__ hints, int max_it, double fit_range, int do_fit,
                                                                             BatchOut *__restrict__ out, const BatchStage stg) {
  icp_batch_body<MODE, NRM, KREG, true>(probs, states, hints, max_it, fit_range, do_fit, out, stg);
}

// stg: the staged instantiation with this stage, or null
static void launch_icp_batch(hipStream_t stream, int n, int mode, bool nrm, int k, const BatchProblem *probs, IcpState *states,
                             uint32_t *hints, int max_it, double fit_range, int do_fit, BatchOut *out, const BatchStage *stg) {
#define OPE_LAUNCH_BATCH(M, N, KR) \
  do { \
    if (stg) hipLaunchKernelGGL((icp_batch_rejectors_kernel<M, N, KR>), dim3(n), dim3(kBatchBlock), 0, stream, probs, states, hints, max_it, fit_range, do_fit, out, *stg); \
    else hipLaunchKernelGGL((icp_batch_kernel<M, N, KR>), dim3(n), dim3(kBatchBlock), 0, stream, probs, states, hints, max_it, fit_range, do_fit, out); \
  } while (0)
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

// the caller's parameters, or the defaults
static ope_icp_params icp_batch_params(const ope_icp_params *params) {
  ope_icp_params p;
  ope_icp_default_params(&p);
  if (params) p = *params;
  return p;
}
// the arguments and problems of ope_icp_run_batch (and of ope_icp_run_batch_rejectors, `who`) under p: every refusal
static int icp_batch_check_call(ope_ctx *ctx, const std::string &who, size_t n, const ope_cloud *const *src, const ope_index *const *tgt,
                                const ope_icp_params &p, const void *out) {
  if (!src || !tgt || !out) return set_err(ctx, OPE_EINVAL, who + ": bad argument");
  if (n > (size_t)INT_MAX) return set_err(ctx, OPE_EINVAL, who + ": too many problems");
  { const int rc = icp_batch_check_params(ctx, p); if (rc != OPE_OK) return rc; }
  const bool need_src_nrm = p.corr_mode == OPE_CORR_NORMAL_SHOOTING || p.use_surface_normal_rej || p.use_self_occluded_rej;
  const bool p2p = p.estimator == OPE_EST_POINT_TO_PLANE_LLS;
  for (size_t i = 0; i < n; ++i) {
    const std::string at = " (problem " + std::to_string(i) + ")";
    if (!src[i]) return set_err(ctx, OPE_EINVAL, who + ": no source cloud" + at);
    if (!tgt[i]) return set_err(ctx, OPE_EEMPTY, who + ": no input target dataset was given" + at);
    if (need_src_nrm && !src[i]->d_nrm) return set_err(ctx, OPE_EINVAL, who + ": source normals required but absent" + at);
    if (p2p && !tgt[i]->d_nrm) return set_err(ctx, OPE_EINVAL, who + ": the point-to-plane estimator needs target normals" + at);
    if (p.use_surface_normal_rej && !tgt[i]->d_nrm) return set_err(ctx, OPE_EINVAL, who + ": target normals required" + at);
    if (src[i]->n_valid > kBatchMaxSrc)
      return set_err(ctx, OPE_EINVAL, who + ": more than 65536 valid source points (use ope_icp_run)" + at);
    if (ctx->n_fixed > 0 && ctx->fixed_src == src[i])
      return set_err(ctx, OPE_EINVAL, who + ": fixed correspondences are set for this source cloud" + at);
  }
  return OPE_OK;
}

extern "C" int ope_icp_run_batch(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                                 const ope_icp_params *params, double fitness_max_range, ope_icp_batch_result *out) {
  if (!ctx) return set_err(ctx, OPE_EINVAL, "ope_icp_run_batch: bad argument");
  if (n == 0) return OPE_OK;
  const ope_icp_params p = icp_batch_params(params);
  { const int rc = icp_batch_check_call(ctx, "ope_icp_run_batch", n, src, tgt, p, out); if (rc != OPE_OK) return rc; }
  return icp_batch_core(ctx, n, src, tgt, guesses, p, fitness_max_range, out);
}

// a list handed to a batched entry point (`who`): the refusals of ope_icp_set_global_rejectors, and of a single run under a list
int ope::icp_batch_check_list(ope_ctx *ctx, const std::string &who, const ope_icp_params &p, const ope_global_rejector *list, size_t n_list) {
  if (n_list > 0 && !list) return set_err(ctx, OPE_EINVAL, who + ": bad argument");
  if (n_list > OPE_GREJ_MAX) return set_err(ctx, OPE_EINVAL, who + ": at most OPE_GREJ_MAX rejectors");
  for (size_t k = 0; k < n_list; ++k)
    if (grej_check(list + k) != OPE_OK)
      return set_err(ctx, OPE_EINVAL, who + ": rejector " + std::to_string(k) +
                                          ": unknown kind, factor not finite or < 0, a ratio outside [0, 1] or min_ratio > max_ratio");
  if (p.use_reciprocal) return set_err(ctx, OPE_EINVAL, who + ": reciprocal correspondences are not supported");
  if (p.estimator != OPE_EST_SVD)
    return set_err(ctx, OPE_EINVAL, who + ": global correspondence rejectors and the pair output need the OPE_EST_SVD estimator");
  return OPE_OK;
}

extern "C" int ope_icp_run_batch_rejectors(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                                           const ope_icp_params *params, const ope_global_rejector *list, size_t n_list,
                                           double fitness_max_range, ope_icp_batch_result *out, ope_global_rejector_stats *stats,
                                           int32_t *index_match, float *distance) {
  static const char *who = "ope_icp_run_batch_rejectors";
  if (!ctx) return set_err(ctx, OPE_EINVAL, std::string(who) + ": bad argument");
  if (n_list == 0 && index_match == nullptr && distance == nullptr)   // nothing asked of the stage: ope_icp_run_batch
    return ope_icp_run_batch(ctx, n, src, tgt, guesses, params, fitness_max_range, out);
  const ope_icp_params p = icp_batch_params(params);
  { const int rc = icp_batch_check_list(ctx, who, p, list, n_list); if (rc != OPE_OK) return rc; }
  if (n == 0) return OPE_OK;
  { const int rc = icp_batch_check_call(ctx, who, n, src, tgt, p, out); if (rc != OPE_OK) return rc; }
  const BatchStageReq req{list, n_list, stats, index_match, distance};
  return icp_batch_core(ctx, n, src, tgt, guesses, p, fitness_max_range, out, &req);
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
                        const ope_icp_params &p, double fitness_max_range, ope_icp_batch_result *out, const BatchStageReq *stage) {
  if (n == 0) return OPE_OK;
  const bool need_src_nrm = p.corr_mode == OPE_CORR_NORMAL_SHOOTING || p.use_surface_normal_rej || p.use_self_occluded_rej;
  const bool p2p = p.estimator == OPE_EST_POINT_TO_PLANE_LLS;
  size_t n_hints = 0;
  for (size_t i = 0; i < n; ++i) n_hints += src[i]->n_valid;
  OPE_HIP(ctx, hipSetDevice(ctx->device));

  // one temporary block: [problems | states | stage: problems, list | results | start leaves | stage: statistics, work, pairs];
  // what comes before the results goes up in one copy
  auto up8 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t b_prob = up8(sizeof(BatchProblem) * n), b_state = up8(sizeof(IcpState) * n), b_out = up8(sizeof(BatchOut) * n);
  const size_t b_hint = up8(sizeof(uint32_t) * std::max<size_t>(n_hints, 1));
  const size_t b_sprob = stage ? up8(sizeof(BatchStageProblem) * n) : 0, b_slist = stage ? up8(sizeof(ope_global_rejector) * OPE_GREJ_MAX) : 0;
  std::vector<unsigned char> host(b_prob + b_state + b_sprob + b_slist);
  BatchProblem *hp = reinterpret_cast<BatchProblem *>(host.data());
  IcpState *hs = reinterpret_cast<IcpState *>(host.data() + b_prob);
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    hp[i] = BatchProblem{src[i]->view(), tgt[i]->view(), off};
    off += src[i]->n_valid;
    // the state ope_icp_begin starts a run with (no skip certificates: the batch has no host that could see them asked for)
    icp_state_init(hs + i, src[i], tgt[i], guesses ? guesses + 16 * i : nullptr, p, false, false);
  }
  // the stage's slices (4-byte words): per problem the pairs, then the keys and words that do not fit LDS
  size_t n_work = 0, n_pairs = 0;
  const bool want_pairs = stage && (stage->index_match || stage->distance);
  if (stage) {
    BatchStageProblem *sp = reinterpret_cast<BatchStageProblem *>(host.data() + b_prob + b_state);
    ope_global_rejector *sl = reinterpret_cast<ope_global_rejector *>(host.data() + b_prob + b_state + b_sprob);
    bool sorts = false, words = false;
    for (size_t k = 0; k < stage->n_list; ++k) {
      sl[k] = stage->list[k];
      sorts |= sl[k].kind == OPE_GREJ_VAR_TRIMMED;
      words |= sl[k].kind == OPE_GREJ_ONE_TO_ONE;
    }
    for (size_t i = 0; i < n; ++i) {
      const size_t nv = src[i]->n_valid, nt = tgt[i]->n;
      sp[i].pos_off = n_work; n_work += nv;
      sp[i].d2_off = n_work; n_work += nv;
      sp[i].keys_off = n_work;
      if (sorts && nv > kStageSortLds) {
        size_t n2 = 2;
        while (n2 < nv) n2 <<= 1;
        n_work += n2;
      }
      n_work = (n_work + 1) & ~(size_t)1;
      sp[i].words_off = n_work;
      if (words && nt > kStageOtoLds) n_work += 2 * nt;
      sp[i].pair_off = n_pairs;
      n_pairs += src[i]->n;
    }
  }
  const size_t b_sstat = stage ? up8(sizeof(GrejStat) * OPE_GREJ_MAX * n) : 0, b_work = stage ? up8(4 * std::max<size_t>(n_work, 1)) : 0;
  const size_t b_pair = want_pairs ? up8(4 * std::max<size_t>(n_pairs, 1)) : 0;
  unsigned char *blk = nullptr;
  OPE_HIP(ctx, tmp_malloc(ctx->stream, (void **)&blk, host.size() + b_out + b_hint + b_sstat + b_work + 2 * b_pair));
  struct FreeBlk { hipStream_t s; void *p; ~FreeBlk() { tmp_free(s, p); } } free_blk{ctx->stream, blk};
  BatchProblem *d_prob = reinterpret_cast<BatchProblem *>(blk);
  IcpState *d_state = reinterpret_cast<IcpState *>(blk + b_prob);
  BatchOut *d_out = reinterpret_cast<BatchOut *>(blk + host.size());
  uint32_t *d_hint = reinterpret_cast<uint32_t *>(blk + host.size() + b_out);
  OPE_HIP(ctx, h2d_copy(ctx->stream, blk, host.data(), host.size()));
  OPE_HIP(ctx, hipMemsetAsync(d_hint, 0, b_hint, ctx->stream));
  BatchStage stg{};
  if (stage) {
    unsigned char *s0 = blk + host.size() + b_out + b_hint;
    stg.probs = reinterpret_cast<const BatchStageProblem *>(blk + b_prob + b_state);
    stg.list = reinterpret_cast<const ope_global_rejector *>(blk + b_prob + b_state + b_sprob);
    stg.stats = reinterpret_cast<GrejStat *>(s0);
    stg.work = reinterpret_cast<uint32_t *>(s0 + b_sstat);
    stg.n_list = (int)stage->n_list;
    if (want_pairs) {   // "no pair" everywhere: the kernel writes the survivors
      stg.pair_match = reinterpret_cast<int32_t *>(s0 + b_sstat + b_work);
      stg.pair_d2 = reinterpret_cast<float *>(s0 + b_sstat + b_work + b_pair);
      OPE_HIP(ctx, hipMemsetAsync(stg.pair_match, 0xff, b_pair, ctx->stream));
      OPE_HIP(ctx, hipMemsetAsync(stg.pair_d2, 0, b_pair, ctx->stream));
    }
  }
  const bool nrm = need_src_nrm || p2p;
  const bool do_fit = fitness_max_range >= 0.0;
  launch_icp_batch(ctx->stream, (int)n, p.corr_mode, nrm, p.k_normal_shooting, d_prob, d_state, d_hint, std::max(p.max_iterations, 1),
                   do_fit ? fitness_max_range : 0.0, do_fit ? 1 : 0, d_out, stage ? &stg : nullptr);
  OPE_HIP(ctx, hipGetLastError());
  std::vector<BatchOut> ho(n);
  std::vector<GrejStat> hstat(stage && stage->stats ? OPE_GREJ_MAX * n : 0);
  OPE_HIP(ctx, hipMemcpyAsync(ho.data(), d_out, sizeof(BatchOut) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (!hstat.empty()) OPE_HIP(ctx, hipMemcpyAsync(hstat.data(), stg.stats, sizeof(GrejStat) * hstat.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (want_pairs && n_pairs > 0) {
    if (stage->index_match) OPE_HIP(ctx, hipMemcpyAsync(stage->index_match, stg.pair_match, 4 * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    if (stage->distance) OPE_HIP(ctx, hipMemcpyAsync(stage->distance, stg.pair_d2, 4 * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
  }
  OPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < hstat.size() / OPE_GREJ_MAX; ++i)   // (launches = 0: the stage dispatches nothing of its own)
    for (size_t k = 0; k < stage->n_list; ++k) grej_stat_to_abi(hstat[i * OPE_GREJ_MAX + k], 0, &stage->stats[i * stage->n_list + k]);
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
