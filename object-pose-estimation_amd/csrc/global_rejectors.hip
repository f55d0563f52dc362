// global_rejectors.hip — the correspondence rejectors of estimateFinePose's list that need ALL of an iteration's pairs before they
// can decide about one (poseestimator.cpp:250-292, blocks 3.1 median distance, 3.2 one to one, 3.5 var trimmed), as a second stage
// of the ICP iteration on the device, and stand-alone on given pairs (ope_reject_correspondences).  The rules are stated in
// include/ope.h and restated in numpy in tests/global_rejectors_ref.py, which the kernels are pinned to.
//
// The stage works on the run's correspondence arrays (per sorted source position: match = ORIGINAL target index or -1, d2 = the
// pair's distance field) and one byte per pair, `keep`:
//   grej_init_kernel          keep = (match >= 0); the rejectors' counters, histograms and one-to-one words start over
//   median distance           an exact selection of position m / 2 over the fp32 bit patterns (non-negative: unsigned order is numeric
//                             order): four histogram passes over 8-bit digits, most significant first, each pass choosing its digit
//                             prefix on the device from the histograms before it (a 256-bin scan per block), then the keep pass.
//                             No sort; m is known only to the device (it is the total of the first histogram).
//   one to one                one 64-bit word per target point, (distance bits << 32) | original query index, reduced with a 64-bit
//                             atomic min; then a pair stays iff the word is its own.
//   var trimmed               keys (pairs that did not reach the rejector keyed to the top) sorted by rocPRIM's radix sort; the head sum
//                             L in one partial per block and a fixed tree; FRMS_j and its first minimum per block, then over the blocks;
//                             ratio, idx and the trimmed distance by one lane of the keep pass.  All in fp64.
//   grej_sums_kernel          the 17 sums of the pairs still marked, the source point moved by the same fp32 rows the search used; pairs
//                             that fell are written back as -1.  One partial row per block, reduced by icp_reduce_update_kernel's fixed
//                             tree: the sums do not depend on the run (deterministic_sums or not).
// Every kernel of the stage early-outs on the run's "done" flag like the accumulate launches, so the statistics of the last
// iteration stay in place.  Nothing here synchronises the host or allocates between ope_icp_begin and the end of the run, and the
// launches per iteration follow from the list alone.
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include <rocprim/rocprim.hpp>

#include "bvh_traverse.hpp"
#include "icp_pair.hpp"     // the moved query of the survivor sums
#include "grej_rules.hpp"   // every rule of the three rejectors; here: their launches and reductions

namespace ope {

constexpr int kGrejBlock = 256;
constexpr int kGrejMaxBlocks = kAccMaxBlocks;   // grid-stride loops; the survivor sums keep one partial row per block
constexpr int kGrejVtBlocks = 256;              // var trimmed: blocks of the head-sum and FRMS launches (= kGrejBlock: one lane per partial)
static_assert(kGrejVtBlocks == kGrejBlock, "the partials of the var-trimmed launches are reduced by one block, one lane each");

struct GrejSlot {   // one per rejector of the list
  GrejStat stat;                    // (first: grej_read_stats copies the head of the slot)
  uint32_t hist[4][256];            // median distance: digit histograms, most significant digit first
  double vt_head[kGrejVtBlocks];    // var trimmed: partial head sums
  double vt_best[kGrejVtBlocks];    // ... the smallest FRMS of each block
  uint32_t vt_best_j[kGrejVtBlocks];   // ... and its first position
};

struct GrejWork {
  unsigned char *d_keep = nullptr; size_t keep_cap = 0;
  unsigned long long *d_words = nullptr; size_t words_cap = 0;   // n_tgt words per one-to-one rejector of the list
  size_t n_tgt = 0;
  int32_t *d_tgt_pos = nullptr; size_t pos_cap = 0;              // ORIGINAL target index -> position in the index's point order
  uint32_t *d_keys = nullptr, *d_keys_sorted = nullptr; size_t keys_cap = 0;
  void *d_sort_tmp = nullptr; size_t sort_tmp_cap = 0;
  double *d_partials = nullptr;                                  // [kNumSums][kAccMaxBlocks]
  GrejSlot *d_slots = nullptr;                                   // OPE_GREJ_MAX
};

// inclusive scan over the block's 256 lanes; s_scan[255] holds the total until the caller's next barrier
__device__ __forceinline__ uint32_t grej_scan256(uint32_t v, uint32_t *s_scan) {
  s_scan[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kGrejBlock; off <<= 1) {
    const uint32_t a = (int)threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0u;
    __syncthreads();
    s_scan[threadIdx.x] += a;
    __syncthreads();
  }
  return s_scan[threadIdx.x];
}

// The digits chosen by the histograms 0 .. upto-1: s_sel = {prefix (upto digits), rank within the prefix' bucket, m}.
__device__ __forceinline__ void grej_median_select(const GrejSlot *slot, int upto, uint32_t *s_scan, uint32_t *s_sel) {
  if (threadIdx.x == 0) { s_sel[0] = 0u; s_sel[1] = 0u; s_sel[2] = 0u; }
  __syncthreads();
  for (int q = 0; q < upto; ++q) {
    const uint32_t h = slot->hist[q][threadIdx.x];
    const uint32_t incl = grej_scan256(h, s_scan);
    const uint32_t total = s_scan[kGrejBlock - 1];
    __syncthreads();
    if (q == 0 && threadIdx.x == 0) { s_sel[2] = total; s_sel[1] = grej_median_rank(total); }
    __syncthreads();
    const uint32_t rank = s_sel[1], excl = incl - h;
    __syncthreads();
    // grej_digit_pick (grej_rules.hpp) for one digit per lane, on its own text: through the function grej_median_hist_kernel's
    // registers are numbered differently
    if (h > 0u && excl <= rank && rank < incl) { s_sel[0] = (s_sel[0] << 8) | threadIdx.x; s_sel[1] = rank - excl; }   // one lane at most
    __syncthreads();
  }
}

__device__ __forceinline__ unsigned long long grej_block_count(uint32_t c, uint32_t *s_scan) {
  const uint32_t incl = grej_scan256(c, s_scan);
  (void)incl;
  const uint32_t total = s_scan[kGrejBlock - 1];
  __syncthreads();
  return (unsigned long long)total;
}

__global__ __launch_bounds__(kGrejBlock) void grej_init_kernel(const IcpState *__restrict__ st, uint32_t n, const int32_t *__restrict__ match,
                                                                unsigned char *__restrict__ keep, int keep_from_match, GrejSlot *slots,
                                                                int n_slots, unsigned long long *__restrict__ words, size_t n_words) {
  if (st != nullptr && st->done) return;
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) keep[i] = keep_from_match ? (match[i] >= 0 ? 1 : 0) : 1;
  for (size_t w = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; w < n_words; w += stride) words[w] = ~0ull;
  if (blockIdx.x == 0) {
    for (int s = 0; s < n_slots; ++s) {
#pragma unroll
      for (int p = 0; p < 4; ++p) slots[s].hist[p][threadIdx.x] = 0u;
      if (threadIdx.x == 0) slots[s].stat = grej_stat_none();
    }
  }
}

// ---- median distance
__global__ __launch_bounds__(kGrejBlock) void grej_median_hist_kernel(const IcpState *__restrict__ st, uint32_t n, const unsigned char *__restrict__ keep,
                                                                       const float *__restrict__ d2, GrejSlot *slot, int pass) {
  if (st != nullptr && st->done) return;
  __shared__ uint32_t s_scan[kGrejBlock], s_hist[kGrejBlock], s_sel[3];
  grej_median_select(slot, pass, s_scan, s_sel);
  const uint32_t prefix = s_sel[0];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) {
    if (!keep[i]) continue;
    uint32_t digit;
    if (grej_median_digit(__float_as_uint(d2[i]), pass, prefix, digit)) atomicAdd(&s_hist[digit], 1u);
  }
  __syncthreads();
  if (s_hist[threadIdx.x] != 0u) atomicAdd(&slot->hist[pass][threadIdx.x], s_hist[threadIdx.x]);
}

__global__ __launch_bounds__(kGrejBlock) void grej_median_keep_kernel(const IcpState *__restrict__ st, uint32_t n, unsigned char *__restrict__ keep,
                                                                       const float *__restrict__ d2, GrejSlot *slot, double factor) {
  if (st != nullptr && st->done) return;
  __shared__ uint32_t s_scan[kGrejBlock], s_sel[3];
  grej_median_select(slot, 4, s_scan, s_sel);
  const uint32_t m = s_sel[2];
  const GrejMedianRule rule(m, s_sel[0], factor);
  uint32_t kept = 0u;
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) {
    if (!keep[i]) continue;
    const bool k = rule.keep(d2[i]);
    keep[i] = k ? 1 : 0;
    kept += k ? 1u : 0u;
  }
  const unsigned long long total = grej_block_count(kept, s_scan);
  if (threadIdx.x == 0) {
    if (total) atomicAdd(&slot->stat.n_out, total);
    if (blockIdx.x == 0) { slot->stat.n_in = (unsigned long long)m; slot->stat.threshold = rule.threshold(); }
  }
}

// ---- one to one
template <bool KEEP_PASS>
__global__ __launch_bounds__(kGrejBlock) void grej_one_to_one_kernel(const IcpState *__restrict__ st, uint32_t n, unsigned char *__restrict__ keep,
                                                                      const int32_t *__restrict__ match, const float *__restrict__ d2,
                                                                      const int32_t *__restrict__ qidx, const float4 *__restrict__ src_xyzw,
                                                                      unsigned long long *__restrict__ words, size_t n_words, GrejSlot *slot) {
  if (st != nullptr && st->done) return;
  __shared__ uint32_t s_scan[kGrejBlock];
  uint32_t cnt = 0u;
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) {
    if (!keep[i]) continue;
    const int32_t mt = match[i];
    const int32_t q = qidx != nullptr ? qidx[i] : __float_as_int(src_xyzw[i].w);
    const unsigned long long word = grej_word(d2[i], q);
    if (!KEEP_PASS) {
      ++cnt;
      if (mt < 0 || (size_t)mt >= n_words) { keep[i] = 0; continue; }   // stand-alone: pairs without a match are dropped
      atomicMin(words + mt, word);
    } else {
      const bool k = words[mt] == word;
      keep[i] = k ? 1 : 0;
      cnt += k ? 1u : 0u;
    }
  }
  const unsigned long long total = grej_block_count(cnt, s_scan);
  if (threadIdx.x == 0 && total) atomicAdd(KEEP_PASS ? &slot->stat.n_out : &slot->stat.n_in, total);
}

// ---- var trimmed
__global__ __launch_bounds__(kGrejBlock) void grej_vt_keys_kernel(const IcpState *__restrict__ st, uint32_t n, const unsigned char *__restrict__ keep,
                                                                   const float *__restrict__ d2, uint32_t *__restrict__ keys, GrejSlot *slot) {
  if (st != nullptr && st->done) return;
  __shared__ uint32_t s_scan[kGrejBlock];
  uint32_t cnt = 0u;
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) {
    const bool k = keep[i] != 0;
    keys[i] = k ? __float_as_uint(d2[i]) : 0xffffffffu;
    cnt += k ? 1u : 0u;
  }
  const unsigned long long total = grej_block_count(cnt, s_scan);
  if (threadIdx.x == 0 && total) atomicAdd(&slot->stat.n_in, total);
}

// fixed tree over the block's 256 values
__device__ __forceinline__ double grej_tree_sum(double v, double *s_d) {
  s_d[threadIdx.x] = v;
  __syncthreads();
  for (int off = kGrejBlock / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) s_d[threadIdx.x] += s_d[threadIdx.x + off];
    __syncthreads();
  }
  const double r = s_d[0];
  __syncthreads();
  return r;
}
// (smallest value, on equal values the smallest position) over the block's 256 candidates
__device__ __forceinline__ void grej_tree_argmin(double &v, uint32_t &j, double *s_d, uint32_t *s_j) {
  s_d[threadIdx.x] = v; s_j[threadIdx.x] = j;
  __syncthreads();
  for (int off = kGrejBlock / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const double v2 = s_d[threadIdx.x + off];
      const uint32_t j2 = s_j[threadIdx.x + off];
      if (grej_argmin_before(v2, j2, s_d[threadIdx.x], s_j[threadIdx.x])) { s_d[threadIdx.x] = v2; s_j[threadIdx.x] = j2; }
    }
    __syncthreads();
  }
  v = s_d[0]; j = s_j[0];
  __syncthreads();
}

__global__ __launch_bounds__(kGrejBlock) void grej_vt_head_kernel(const IcpState *__restrict__ st, const uint32_t *__restrict__ sorted, GrejSlot *slot,
                                                                   double min_ratio, double max_ratio) {
  if (st != nullptr && st->done) return;
  __shared__ double s_d[kGrejBlock];
  const uint32_t m = (uint32_t)slot->stat.n_in;
  uint32_t lo, hi;
  grej_vt_range(m, min_ratio, max_ratio, lo, hi);
  double acc = 0.0;
  for (size_t j = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; j < lo; j += (size_t)kGrejVtBlocks * kGrejBlock) acc += (double)__uint_as_float(sorted[j]);
  const double v = grej_tree_sum(acc, s_d);
  if (threadIdx.x == 0) slot->vt_head[blockIdx.x] = v;
}

__global__ __launch_bounds__(kGrejBlock) void grej_vt_frms_kernel(const IcpState *__restrict__ st, const uint32_t *__restrict__ sorted, GrejSlot *slot,
                                                                   double min_ratio, double max_ratio) {
  if (st != nullptr && st->done) return;
  __shared__ double s_d[kGrejBlock];
  __shared__ uint32_t s_j[kGrejBlock];
  const uint32_t m = (uint32_t)slot->stat.n_in;
  uint32_t lo, hi;
  grej_vt_range(m, min_ratio, max_ratio, lo, hi);
  const double L = grej_tree_sum(slot->vt_head[threadIdx.x], s_d);   // the same tree in every block: the same L
  double best = std::numeric_limits<double>::infinity();
  uint32_t best_j = 0xffffffffu;
  for (size_t j = (size_t)lo + (size_t)blockIdx.x * kGrejBlock + threadIdx.x; j < hi; j += (size_t)kGrejVtBlocks * kGrejBlock) {
    const double frms = grej_vt_frms((uint32_t)j, m, sorted[j], L);
    if (frms < best) { best = frms; best_j = (uint32_t)j; }
  }
  grej_tree_argmin(best, best_j, s_d, s_j);
  if (threadIdx.x == 0) { slot->vt_best[blockIdx.x] = best; slot->vt_best_j[blockIdx.x] = best_j; }
}

__global__ __launch_bounds__(kGrejBlock) void grej_vt_keep_kernel(const IcpState *__restrict__ st, uint32_t n, unsigned char *__restrict__ keep,
                                                                   const float *__restrict__ d2, const uint32_t *__restrict__ sorted, GrejSlot *slot,
                                                                   double min_ratio, double max_ratio) {
  if (st != nullptr && st->done) return;
  __shared__ double s_d[kGrejBlock];
  __shared__ uint32_t s_j[kGrejBlock];
  __shared__ uint32_t s_scan[kGrejBlock];
  const uint32_t m = (uint32_t)slot->stat.n_in;
  uint32_t lo, hi;
  grej_vt_range(m, min_ratio, max_ratio, lo, hi);
  double best = slot->vt_best[threadIdx.x];
  uint32_t best_j = slot->vt_best_j[threadIdx.x];
  grej_tree_argmin(best, best_j, s_d, s_j);
  const GrejVtRule rule(m, lo, hi, best_j, sorted);
  uint32_t kept = 0u;
  const size_t stride = (size_t)gridDim.x * kGrejBlock;
  for (size_t i = (size_t)blockIdx.x * kGrejBlock + threadIdx.x; i < n; i += stride) {
    if (!keep[i]) continue;
    const bool k = rule.all || (double)d2[i] < rule.trimmed;   // GrejVtRule::keep, on its own text: the call costs this kernel two SGPRs
    keep[i] = k ? 1 : 0;
    kept += k ? 1u : 0u;
  }
  const unsigned long long total = grej_block_count(kept, s_scan);
  if (threadIdx.x == 0) {
    if (total) atomicAdd(&slot->stat.n_out, total);
    if (blockIdx.x == 0) { slot->stat.threshold = rule.trimmed; slot->stat.ratio = (double)rule.ratio; }
  }
}

// ---- survivor sums
__global__ __launch_bounds__(kGrejBlock) void grej_tgt_pos_kernel(BvhView tgt, int32_t *__restrict__ pos_of_orig, uint32_t n_total) {
  const uint32_t p = blockIdx.x * kGrejBlock + threadIdx.x;
  if (p >= tgt.n) return;
  const int32_t o = __float_as_int(tgt.pts[p].w);
  if (o >= 0 && (uint32_t)o < n_total) pos_of_orig[o] = (int32_t)p;
}

// The 17 sums {n, sum s, sum t, sum t s^T, sum d^2} about the pivot over the pairs still marked; term by term what the accumulate
// kernels add (icp_kernels.hip: add_query_sums).  Pairs that fell are written back as "no correspondence".
__global__ __launch_bounds__(kGrejBlock) void grej_sums_kernel(CloudView src, BvhView tgt, const IcpState *__restrict__ st, const unsigned char *__restrict__ keep,
                                                                int32_t *__restrict__ match, const float *__restrict__ d2, const int32_t *__restrict__ pos_of_orig,
                                                                double *__restrict__ partials) {
  if (st->done) return;
  __shared__ double s_red[kGrejBlock / 64][kNumSums];
  float F[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) F[k] = st->Ff[k];
  const float psx = (float)st->pivot[0], psy = (float)st->pivot[1], psz = (float)st->pivot[2];
  double acc[kNumSums];
#pragma unroll
  for (int k = 0; k < kNumSums; ++k) acc[k] = 0.0;
  for (uint32_t i = blockIdx.x * kGrejBlock + threadIdx.x; i < src.n_valid; i += gridDim.x * kGrejBlock) {
    const int32_t mt = match[i];
    if (mt < 0) continue;
    if (!keep[i]) { match[i] = -1; continue; }
    float x, y, z;
    pair_move_point((const float *)F, src.xyzw[i], x, y, z);
    const float4 t = tgt.pts[pos_of_orig[mt]];
    const double sx = (double)x - (double)psx, sy = (double)y - (double)psy, sz = (double)z - (double)psz;
    const double tx = (double)t.x - (double)psx, ty = (double)t.y - (double)psy, tz = (double)t.z - (double)psz;
    acc[0] += 1.0;
    acc[1] += sx; acc[2] += sy; acc[3] += sz;
    acc[4] += tx; acc[5] += ty; acc[6] += tz;
    acc[7] += tx * sx; acc[8] += tx * sy; acc[9] += tx * sz;
    acc[10] += ty * sx; acc[11] += ty * sy; acc[12] += ty * sz;
    acc[13] += tz * sx; acc[14] += tz * sy; acc[15] += tz * sz;
    acc[16] += (double)d2[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kNumSums; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kNumSums)
    partials[threadIdx.x * kAccMaxBlocks + blockIdx.x] = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// ---- host side
static int grej_blocks(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + kGrejBlock - 1) / kGrejBlock, 1), kGrejMaxBlocks); }

int grej_check(const ope_global_rejector *r) {
  if (!r) return OPE_EINVAL;
  switch (r->kind) {
    case OPE_GREJ_MEDIAN_DISTANCE: return std::isfinite(r->factor) && r->factor >= 0.0 ? OPE_OK : OPE_EINVAL;
    case OPE_GREJ_ONE_TO_ONE: return OPE_OK;
    case OPE_GREJ_VAR_TRIMMED:
      return (r->min_ratio >= 0.0 && r->min_ratio <= 1.0 && r->max_ratio >= 0.0 && r->max_ratio <= 1.0 && r->min_ratio <= r->max_ratio) ? OPE_OK : OPE_EINVAL;
    default: return OPE_EINVAL;
  }
}

// dispatches booked per application of one rejector (ope.h: ope_global_rejector_stats.launches)
int grej_launches(int kind) {
  return kind == OPE_GREJ_MEDIAN_DISTANCE ? 5 : kind == OPE_GREJ_ONE_TO_ONE ? 2 : 5;
}

void grej_free(GrejWork *w) {
  if (!w) return;
  for (void *p : {(void *)w->d_keep, (void *)w->d_words, (void *)w->d_tgt_pos, (void *)w->d_keys, (void *)w->d_keys_sorted, w->d_sort_tmp,
                  (void *)w->d_partials, (void *)w->d_slots})
    if (p) (void)hipFree(p);
  delete w;
}

// Buffers for n_pairs pairs onto n_tgt target points under `list`; grows, never shrinks.  Called by ope_icp_begin and by the
// stand-alone entry point (with a work area of its own), never between iterations.
hipError_t grej_ensure(GrejWork **pw, hipStream_t stream, size_t n_pairs, size_t n_tgt, const ope_global_rejector *list, size_t n_list) {
  if (*pw == nullptr) *pw = new GrejWork();
  GrejWork *w = *pw;
  hipError_t e = hipSuccess;
  const size_t np = std::max<size_t>(n_pairs, 1);
  size_t n_oto = 0;
  bool sorts = false;
  for (size_t k = 0; k < n_list; ++k) { n_oto += list[k].kind == OPE_GREJ_ONE_TO_ONE; sorts |= list[k].kind == OPE_GREJ_VAR_TRIMMED; }
  if (w->d_slots == nullptr) {
    if ((e = hipMalloc((void **)&w->d_slots, sizeof(GrejSlot) * OPE_GREJ_MAX)) != hipSuccess) return e;
    if ((e = hipMalloc((void **)&w->d_partials, sizeof(double) * kNumSums * kAccMaxBlocks)) != hipSuccess) return e;
  }
  if (w->keep_cap < np) {
    if (w->d_keep) (void)hipFree(w->d_keep);
    w->d_keep = nullptr; w->keep_cap = 0;
    if ((e = hipMalloc((void **)&w->d_keep, np)) != hipSuccess) return e;
    w->keep_cap = np;
  }
  const size_t nw = std::max<size_t>(n_tgt * n_oto, 1);
  if (w->words_cap < nw) {
    if (w->d_words) (void)hipFree(w->d_words);
    w->d_words = nullptr; w->words_cap = 0;
    if ((e = hipMalloc((void **)&w->d_words, sizeof(unsigned long long) * nw)) != hipSuccess) return e;
    w->words_cap = nw;
  }
  w->n_tgt = n_tgt;
  if (sorts) {
    if (w->keys_cap < np) {
      if (w->d_keys) (void)hipFree(w->d_keys);
      if (w->d_keys_sorted) (void)hipFree(w->d_keys_sorted);
      w->d_keys = w->d_keys_sorted = nullptr; w->keys_cap = 0;
      if ((e = hipMalloc((void **)&w->d_keys, sizeof(uint32_t) * np)) != hipSuccess) return e;
      if ((e = hipMalloc((void **)&w->d_keys_sorted, sizeof(uint32_t) * np)) != hipSuccess) return e;
      w->keys_cap = np;
    }
    size_t tb = 0;
    if ((e = rocprim::radix_sort_keys(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr, np, 0, 32, stream)) != hipSuccess) return e;
    tb = std::max<size_t>(tb, 16);
    if (w->sort_tmp_cap < tb) {
      if (w->d_sort_tmp) (void)hipFree(w->d_sort_tmp);
      w->d_sort_tmp = nullptr; w->sort_tmp_cap = 0;
      if ((e = hipMalloc(&w->d_sort_tmp, tb)) != hipSuccess) return e;
      w->sort_tmp_cap = tb;
    }
  }
  return hipSuccess;
}

// The in-loop stage's extras: the map from ORIGINAL target indices to the index's point order, and clean partial rows.
hipError_t grej_prepare_run(GrejWork *w, hipStream_t stream, const BvhView &tgt, size_t n_total) {
  hipError_t e;
  const size_t nt = std::max<size_t>(n_total, 1);
  if (w->pos_cap < nt) {
    if (w->d_tgt_pos) (void)hipFree(w->d_tgt_pos);
    w->d_tgt_pos = nullptr; w->pos_cap = 0;
    if ((e = hipMalloc((void **)&w->d_tgt_pos, sizeof(int32_t) * nt)) != hipSuccess) return e;
    w->pos_cap = nt;
  }
  if ((e = hipMemsetAsync(w->d_tgt_pos, 0, sizeof(int32_t) * nt, stream)) != hipSuccess) return e;
  if (tgt.n) hipLaunchKernelGGL(grej_tgt_pos_kernel, dim3((tgt.n + kGrejBlock - 1) / kGrejBlock), dim3(kGrejBlock), 0, stream, tgt, w->d_tgt_pos, (uint32_t)n_total);
  // partial rows of blocks that do not exist in this run must read as zero (icp_reduce_update_kernel adds all kAccMaxBlocks)
  return hipMemsetAsync(w->d_partials, 0, sizeof(double) * kNumSums * kAccMaxBlocks, stream);
}

// HIP-event brackets of the stand-alone entry point under ope_profile_kernels (tools/global_rejectors_bench.py); none in the loop
struct GrejTimer {
  std::unique_ptr<KernelTimer> t;
  GrejTimer(ope_ctx *ctx, const char *name, double bytes) { if (ctx) t.reset(new KernelTimer(ctx, name, bytes)); }
};

// The list over n pairs: keep bytes in w->d_keep afterwards.  st: the run's state ("done" early-outs) or null; qidx: the pairs'
// original query indices, or null to read them from src_xyzw[i].w; keep_from_match: pairs without a match never reach the list.
hipError_t grej_apply(hipStream_t stream, GrejWork *w, const ope_global_rejector *list, size_t n_list, const IcpState *st, uint32_t n,
                      const int32_t *match, const float *d2, const int32_t *qidx, const float4 *src_xyzw, bool keep_from_match, ope_ctx *timed) {
  const int nb = grej_blocks(n);
  size_t n_oto = 0;
  for (size_t k = 0; k < n_list; ++k) n_oto += list[k].kind == OPE_GREJ_ONE_TO_ONE;
  const size_t n_words = w->n_tgt * n_oto;
  const int nb_init = grej_blocks(std::max<size_t>(n, n_words));
  hipLaunchKernelGGL(grej_init_kernel, dim3(nb_init), dim3(kGrejBlock), 0, stream, st, n, match, w->d_keep, keep_from_match ? 1 : 0, w->d_slots, (int)n_list,
                     w->d_words, n_words);
  size_t oto = 0;
  for (size_t k = 0; k < n_list; ++k) {
    GrejSlot *slot = w->d_slots + k;
    const ope_global_rejector &r = list[k];
    if (r.kind == OPE_GREJ_MEDIAN_DISTANCE) {
      {
        GrejTimer tm(timed, "grej_median_select", 4.0 * 5.0 * n);   // four passes over keep bytes and distances
        for (int pass = 0; pass < 4; ++pass)
          hipLaunchKernelGGL(grej_median_hist_kernel, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, d2, slot, pass);
      }
      GrejTimer tm(timed, "grej_median_keep", 6.0 * n);
      hipLaunchKernelGGL(grej_median_keep_kernel, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, d2, slot, r.factor);
    } else if (r.kind == OPE_GREJ_ONE_TO_ONE) {
      unsigned long long *words = w->d_words + w->n_tgt * oto++;
      GrejTimer tm(timed, "grej_one_to_one", 2.0 * 13.0 * n + 16.0 * n);
      hipLaunchKernelGGL(grej_one_to_one_kernel<false>, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, match, d2, qidx, src_xyzw, words, w->n_tgt, slot);
      hipLaunchKernelGGL(grej_one_to_one_kernel<true>, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, match, d2, qidx, src_xyzw, words, w->n_tgt, slot);
    } else {
      {
        GrejTimer tm(timed, "grej_vt_keys", 9.0 * n);
        hipLaunchKernelGGL(grej_vt_keys_kernel, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, d2, w->d_keys, slot);
      }
      if (n > 0) {
        GrejTimer tm(timed, "grej_vt_sort", 8.0 * n);
        size_t tb = w->sort_tmp_cap;
        const hipError_t e = rocprim::radix_sort_keys(w->d_sort_tmp, tb, (const uint32_t *)w->d_keys, w->d_keys_sorted, (size_t)n, 0, 32, stream);
        if (e != hipSuccess) return e;
      }
      GrejTimer tm(timed, "grej_vt_frms_keep", 4.0 * n + 6.0 * n);
      hipLaunchKernelGGL(grej_vt_head_kernel, dim3(kGrejVtBlocks), dim3(kGrejBlock), 0, stream, st, w->d_keys_sorted, slot, r.min_ratio, r.max_ratio);
      hipLaunchKernelGGL(grej_vt_frms_kernel, dim3(kGrejVtBlocks), dim3(kGrejBlock), 0, stream, st, w->d_keys_sorted, slot, r.min_ratio, r.max_ratio);
      hipLaunchKernelGGL(grej_vt_keep_kernel, dim3(nb), dim3(kGrejBlock), 0, stream, st, n, w->d_keep, d2, w->d_keys_sorted, slot, r.min_ratio, r.max_ratio);
    }
  }
  return hipGetLastError();
}

// the survivors' sums, one row per block into the work area's partials; returns the blocks launched
int grej_sums(hipStream_t stream, GrejWork *w, const CloudView &src, const BvhView &tgt, const IcpState *st, int32_t *match, const float *d2) {
  const int nb = grej_blocks(src.n_valid);
  hipLaunchKernelGGL(grej_sums_kernel, dim3(nb), dim3(kGrejBlock), 0, stream, src, tgt, st, w->d_keep, match, d2, w->d_tgt_pos, w->d_partials);
  return nb;
}
const double *grej_partials(const GrejWork *w) { return w->d_partials; }

static int grej_read_stats(ope_ctx *ctx, GrejWork *w, size_t which, int kind, ope_global_rejector_stats *out) {
  GrejStat h;
  OPE_HIP(ctx, hipMemcpyAsync(&h, &w->d_slots[which].stat, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  OPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  grej_stat_to_abi(h, grej_launches(kind), out);
  return OPE_OK;
}

}  // namespace ope

using namespace ope;

extern "C" {

void ope_global_rejector_defaults(int kind, ope_global_rejector *r) {
  if (!r) return;
  r->kind = kind;
  r->factor = 1.0;
  r->min_ratio = 0.05;
  r->max_ratio = 0.95;
}

int ope_icp_set_global_rejectors(ope_ctx *ctx, const ope_global_rejector *list, size_t n) {
  if (!ctx) return OPE_EINVAL;
  if (list == nullptr) n = 0;
  if (n > OPE_GREJ_MAX) return set_err(ctx, OPE_EINVAL, "ope_icp_set_global_rejectors: at most OPE_GREJ_MAX rejectors");
  for (size_t k = 0; k < n; ++k)
    if (grej_check(list + k) != OPE_OK)
      return set_err(ctx, OPE_EINVAL, "ope_icp_set_global_rejectors: rejector " + std::to_string(k) +
                                          ": unknown kind, factor not finite or < 0, a ratio outside [0, 1] or min_ratio > max_ratio");
  for (size_t k = 0; k < n; ++k) ctx->grej_list[k] = list[k];
  ctx->n_grej = n;
  return OPE_OK;
}

int ope_icp_global_rejector_stats(ope_ctx *ctx, size_t which, ope_global_rejector_stats *out) {
  if (!ctx || !out) return set_err(ctx, OPE_EINVAL, "ope_icp_global_rejector_stats: bad argument");
  if (ctx->grej == nullptr || ctx->n_grej_run == 0) return set_err(ctx, OPE_ESTATE, "ope_icp_global_rejector_stats: no run of this context has applied a list");
  if (which >= ctx->n_grej_run) return set_err(ctx, OPE_EINVAL, "ope_icp_global_rejector_stats: the last run's list has no such rejector");
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  return grej_read_stats(ctx, ctx->grej, which, ctx->grej_run_list[which].kind, out);
}

int ope_reject_correspondences(ope_ctx *ctx, const ope_global_rejector *r, const int32_t *index_query, const int32_t *index_match,
                               const float *distance, size_t n, unsigned char *keep, ope_global_rejector_stats *stats) {
  if (!ctx || !r || (n > 0 && (!distance || !keep))) return set_err(ctx, OPE_EINVAL, "ope_reject_correspondences: bad argument");
  if (grej_check(r) != OPE_OK)
    return set_err(ctx, OPE_EINVAL, "ope_reject_correspondences: unknown kind, factor not finite or < 0, a ratio outside [0, 1] or min_ratio > max_ratio");
  const bool oto = r->kind == OPE_GREJ_ONE_TO_ONE;
  if (oto && n > 0 && (!index_query || !index_match)) return set_err(ctx, OPE_EINVAL, "ope_reject_correspondences: one to one reads index_query and index_match");
  if (n > 0x7fffffffu) return set_err(ctx, OPE_EINVAL, "ope_reject_correspondences: more than 2^31 - 1 pairs");
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  size_t n_tgt = 0;
  if (oto)
    for (size_t i = 0; i < n; ++i)
      if (index_match[i] >= 0) n_tgt = std::max(n_tgt, (size_t)index_match[i] + 1);
  OPE_HIP(ctx, grej_ensure(&ctx->grej_alone, ctx->stream, n, n_tgt, r, 1));
  float *d_d = nullptr;
  int32_t *d_q = nullptr, *d_m = nullptr;
  struct Tmp {
    hipStream_t s; float *&d; int32_t *&q; int32_t *&m;
    ~Tmp() { tmp_free(s, d); tmp_free(s, q); tmp_free(s, m); }
  } tmp{ctx->stream, d_d, d_q, d_m};
  if (n > 0) {
    OPE_HIP(ctx, tmp_malloc(ctx->stream, (void **)&d_d, sizeof(float) * n));
    OPE_HIP(ctx, h2d_copy(ctx->stream, d_d, distance, sizeof(float) * n));
    if (oto) {
      OPE_HIP(ctx, tmp_malloc(ctx->stream, (void **)&d_q, sizeof(int32_t) * n));
      OPE_HIP(ctx, tmp_malloc(ctx->stream, (void **)&d_m, sizeof(int32_t) * n));
      OPE_HIP(ctx, h2d_copy(ctx->stream, d_q, index_query, sizeof(int32_t) * n));
      OPE_HIP(ctx, h2d_copy(ctx->stream, d_m, index_match, sizeof(int32_t) * n));
    }
  }
  OPE_HIP(ctx, grej_apply(ctx->stream, ctx->grej_alone, r, 1, nullptr, (uint32_t)n, d_m, d_d, d_q, nullptr, false, ctx));
  if (n > 0) OPE_HIP(ctx, hipMemcpyAsync(keep, ctx->grej_alone->d_keep, n, hipMemcpyDeviceToHost, ctx->stream));
  OPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) return grej_read_stats(ctx, ctx->grej_alone, 0, r->kind, stats);
  return OPE_OK;
}

}  // extern "C"
