// prerejective_draws_plan.hpp — the host side of the device draws (prerejective_draws.hip): the stream budget, the sizes of a call
// and the bookkeeping of its fallbacks.  Plain C++ with no device or runtime type, so that a stand-alone program can include it
// (tools/prerejective_draws_plan_check.cpp runs it under the address and undefined-behaviour sanitizers).  DESIGN.md §4.26.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ope {

constexpr int kDrawTile = 1024;          // T: stream positions of one tile (its length table is 2 T bytes of LDS)
constexpr int kDrawWindow = 256;         // W: the default window, the positions one iteration may take
constexpr int kDrawWindowMax = 1024;
constexpr int kDrawMaxSamples = 8;       // ope_prerejective's nr_samples limit
constexpr int64_t kDrawBufferBudget = (int64_t)256 << 20;   // bytes of tile tables and entries a call may allocate

// P of DESIGN §4.26: the expected positions of H iterations, eight standard deviations of their sum, and one window.
//   E = sum_{j<S} (ns / (ns - j) - 1) redraws per iteration, V = sum_{j<S} (j/ns) / (1 - j/ns)^2 their variance.
inline int64_t draw_stream_budget(int ns, int S, int H, int W) {
  double E = 0.0, V = 0.0;
  for (int j = 0; j < S; ++j) {
    const double q = (double)j / (double)ns;
    E += (double)ns / (double)(ns - j) - 1.0;
    V += q / ((1.0 - q) * (1.0 - q));
  }
  return (int64_t)std::ceil((double)H * (2.0 * (double)S + E) + 8.0 * std::sqrt((double)H * V) + (double)W);
}

// the sizes of one call: n problems of H iterations; window / budget = 0 select the defaults
struct DrawPlan {
  int W = 0;
  int64_t P = 0, tiles = 0;
  int64_t buffer_bytes = 0;   // tile tables (tiles * W words) and tile entries (tiles * 2 words) of all problems
  bool fits = false;          // buffer_bytes <= kDrawBufferBudget and every position below 2^32
};
inline DrawPlan draw_plan(int ns, int S, int H, size_t n, int window, int64_t budget) {
  DrawPlan p;
  p.W = window ? window : kDrawWindow;
  p.P = budget ? budget : draw_stream_budget(ns, S, H, p.W);
  if (p.P < 1) p.P = 1;
  p.tiles = (p.P + kDrawTile - 1) / kDrawTile;
  const long double bytes = (long double)n * (long double)p.tiles * (4.0L * p.W + 8.0L);
  p.fits = bytes <= (long double)kDrawBufferBudget && p.P + 2 * (int64_t)kDrawTile < ((int64_t)1 << 32);
  p.buffer_bytes = p.fits ? (int64_t)bytes : -1;
  return p;
}

// the word kernel B leaves per problem
constexpr uint32_t kDrawOverflow = 1u, kDrawShort = 2u;

// ope_prerejective_draws_last_stats' eight fields
enum { kDsMode = 0, kDsDevice, kDsOverflow, kDsShort, kDsHostForSize, kDsPositions, kDsTile, kDsLaunches, kDsFields };

// stats of a call that ran the kernels: the problems that have to be drawn again on the host, in order
inline std::vector<size_t> draw_fallbacks(const uint32_t *words, size_t n, int64_t stats[kDsFields]) {
  std::vector<size_t> again;
  for (size_t a = 0; a < n; ++a) {
    if (words[a] & kDrawOverflow) ++stats[kDsOverflow];
    else if (words[a] & kDrawShort) ++stats[kDsShort];
    else { ++stats[kDsDevice]; continue; }
    again.push_back(a);
  }
  return again;
}

inline void draw_stats_begin(int64_t stats[kDsFields], int mode, const DrawPlan &plan, bool device) {
  for (int i = 0; i < kDsFields; ++i) stats[i] = 0;
  stats[kDsMode] = mode;
  stats[kDsHostForSize] = (mode == 1 && !device) ? 1 : 0;
  stats[kDsPositions] = plan.P;
  stats[kDsTile] = kDrawTile;
}

}  // namespace ope
