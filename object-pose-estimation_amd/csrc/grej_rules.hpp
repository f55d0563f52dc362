// grej_rules.hpp — the rules of the three global correspondence rejectors (ope.h: median distance, one to one, var trimmed), each
// stated once for the two places that apply them: the launches of global_rejectors.hip and the stage_* functions of icp_batch.hip
// (one workgroup per problem).  The shapes of their reductions differ and are not here; every expression that decides about a pair,
// and the record a rejector leaves, is.  tests/global_rejectors_ref.py restates the same rules independently in numpy.
#pragma once

#include <cmath>

#include "ope_internal.hpp"

namespace ope {

// what one rejector of a list leaves behind: the head of GrejSlot, the batched stage's record and what the host reads
struct GrejStat {
  unsigned long long n_in, n_out;
  double threshold, ratio;
};
// launches: dispatches the rejector books per application (grej_launches; 0 where the stage dispatches nothing of its own)
inline void grej_stat_to_abi(const GrejStat &h, int64_t launches, ope_global_rejector_stats *out) {
  out->n_in = (int64_t)h.n_in;
  out->n_out = (int64_t)h.n_out;
  out->threshold = h.threshold;
  out->ratio = h.ratio;
  out->launches = launches;
}

__device__ __forceinline__ double grej_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ GrejStat grej_stat_none() { return GrejStat{0ull, 0ull, grej_nan(), grej_nan()}; }

// ---- median distance: position m / 2 of the pairs' fp32 bit patterns (non-negative: unsigned order is numeric order), selected
// by four histogram passes over 8-bit digits, most significant first.
// Whether pass `pass` counts a key — its digits above agree with the prefix chosen so far — and in which bin.
__device__ __forceinline__ bool grej_median_digit(uint32_t key, int pass, uint32_t prefix, uint32_t &digit) {
  const int shift = 24 - 8 * pass;
  if (!(pass == 0 || (key >> (shift + 8)) == prefix)) return false;
  digit = (key >> shift) & 255u;
  return true;
}
__device__ __forceinline__ uint32_t grej_median_rank(uint32_t m) { return m / 2u; }
// The digit that holds position `rank` of a pass, from the counts c[0 .. NC) of NC consecutive digits and `incl`, the keys in
// these digits and all below them.  True in the one lane at most whose digits hold it: d = which of its digits, r = the rank within
// that digit.
template <int NC>
__device__ __forceinline__ bool grej_digit_pick(const uint32_t (&c)[NC], uint32_t incl, uint32_t rank, uint32_t &d, uint32_t &r) {
  uint32_t tot = 0u;
#pragma unroll
  for (int k = 0; k < NC; ++k) tot += c[k];
  const uint32_t excl = incl - tot;
  r = rank - excl;
  d = 0u;
#pragma unroll
  for (int k = 0; k + 1 < NC; ++k)
    if (d == (uint32_t)k && r >= c[k]) { r -= c[k]; d = (uint32_t)k + 1u; }
  return tot > 0u && excl <= rank && rank < incl;
}
// The keep rule.  m: the pairs that reached the rejector; median_bits: the four digits chosen.
struct GrejMedianRule {
  uint32_t m;
  double median, thr;
  __device__ __forceinline__ GrejMedianRule(uint32_t m_, uint32_t median_bits, double factor)
      : m(m_), median((double)__uint_as_float(median_bits)), thr(median * factor) {}
  __device__ __forceinline__ bool keep(float d2) const { return m > 0u && (double)d2 <= thr; }
  __device__ __forceinline__ double threshold() const { return m > 0u ? median : grej_nan(); }   // what the statistics report
};

// ---- one to one: per target point the smallest word of its pairs, by 64-bit integer minima; a pair stays iff the word is its own
__device__ __forceinline__ unsigned long long grej_word(float d, int32_t q) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(uint32_t)q;
}

// ---- var trimmed: over the m keys ascending, FRMS_j for j in [lo, hi) and its first minimum; all fp64, the ratio in fp32
__device__ __forceinline__ void grej_vt_range(uint32_t m, double min_ratio, double max_ratio, uint32_t &lo, uint32_t &hi) {
  lo = (uint32_t)floor(min_ratio * (double)m);
  hi = (uint32_t)floor(max_ratio * (double)m);
  if (hi > m) hi = m;
  if (lo > m) lo = m;
}
// key: sorted key j; L: the sum of the keys below lo
__device__ __forceinline__ double grej_vt_frms(uint32_t j, uint32_t m, uint32_t key, double L) {
  const double id = (double)(j + 1u);
  const double r = id / (double)m;
  const double inv = 1.0 / (r * r * r);
  return inv * inv * (1.0 / id) * ((double)__uint_as_float(key) + L);
}
// (smallest value, on equal values the smallest position): whether candidate (v2, j2) comes before (v, j)
__device__ __forceinline__ bool grej_argmin_before(double v2, uint32_t j2, double v, uint32_t j) { return v2 < v || (v2 == v && j2 < j); }
// The keep rule.  best_j: the first minimum's position (0xffffffff: none); sorted: the m keys ascending.
struct GrejVtRule {
  bool all;         // every pair stays (PCL: undefined)
  float ratio;
  double trimmed;   // the trimmed distance; NaN with `all`
  __device__ __forceinline__ GrejVtRule(uint32_t m, uint32_t lo, uint32_t hi, uint32_t best_j, const uint32_t *sorted)
      : all(hi <= lo || best_j >= m), ratio(1.0f), trimmed(grej_nan()) {
    if (!all) {
      ratio = __fdiv_rn((float)best_j, (float)m);
      uint32_t idx = (uint32_t)(int)((double)m * (double)ratio);
      if (idx >= m) idx = m - 1u;
      trimmed = (double)__uint_as_float(sorted[idx]);
    }
  }
  __device__ __forceinline__ bool keep(float d2) const { return all || (double)d2 < trimmed; }
};

}  // namespace ope
