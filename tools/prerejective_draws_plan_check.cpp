// The host side of the device draws (csrc/prerejective_draws_plan.hpp: the stream budget, the sizes of a call, the bookkeeping of
// the fallbacks) as a program of its own, for a run under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I object-pose-estimation_amd/csrc
//       tools/prerejective_draws_plan_check.cpp -o plan_check && ./plan_check
// It prints the budgets DESIGN.md 4.26 quotes and returns 0 when every check holds.
#include <cstdio>
#include <cstdlib>

#include "prerejective_draws_plan.hpp"

using namespace ope;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

int main() {
  // the budgets of the five shapes of the tests (tests/prerejective_draws_ref.py computes the same numbers)
  const struct { int ns, S, H; int64_t P; } known[] = {{634, 3, 2000, 12291}, {3, 3, 300, 3166}, {8, 8, 300, 10387}, {9, 8, 300, 8318},
                                                       {4096, 3, 1000, 6264}};
  for (const auto &k : known) {
    const int64_t P = draw_stream_budget(k.ns, k.S, k.H, kDrawWindow);
    std::printf("ns %4d S %d H %5d: P %lld\n", k.ns, k.S, k.H, (long long)P);
    CHECK(P == k.P);
  }
  // every corner of the parameter ranges: finite, positive, and the plan's sizes consistent
  for (const int S : {3, 8})
    for (const int ns : {S, S + 1, 4096})
      for (const int H : {1, 50000, 1 << 20})
        for (const int W : {0, 2 * S, 1024})
          for (const size_t n : {(size_t)1, (size_t)111, (size_t)65535}) {
            const DrawPlan p = draw_plan(ns, S, H, n, W, 0);
            CHECK(p.W == (W ? W : kDrawWindow));
            CHECK(p.P >= (int64_t)2 * S * H + p.W && p.tiles * kDrawTile >= p.P && (p.tiles - 1) * kDrawTile < p.P);
            if (p.fits) CHECK(p.buffer_bytes == (int64_t)n * p.tiles * (4 * p.W + 8) && p.buffer_bytes <= kDrawBufferBudget);
            else CHECK(p.buffer_bytes == -1);
          }
  CHECK(draw_plan(634, 3, 50000, 32, 0, 0).fits);
  CHECK(!draw_plan(634, 3, 1 << 20, 111, 0, 0).fits);          // the call the byte budget is there for
  CHECK(draw_plan(3, 3, 300, 2, 0, 1800).P == 1800 && draw_plan(3, 3, 300, 2, 0, 1800).tiles == 2);
  CHECK(!draw_plan(8, 8, 1, 1, 0, (int64_t)1 << 33).fits);      // positions are 32-bit on the device
  // the fallback bookkeeping
  {
    const uint32_t words[6] = {0, kDrawOverflow, kDrawShort, 0, kDrawOverflow | kDrawShort, 0};
    int64_t st[kDsFields];
    const DrawPlan p = draw_plan(634, 3, 2000, 6, 0, 0);
    draw_stats_begin(st, 1, p, p.fits);
    const std::vector<size_t> again = draw_fallbacks(words, 6, st);
    CHECK(again.size() == 3 && again[0] == 1 && again[1] == 2 && again[2] == 4);
    CHECK(st[kDsMode] == 1 && st[kDsDevice] == 3 && st[kDsOverflow] == 2 && st[kDsShort] == 1 && st[kDsHostForSize] == 0);
    CHECK(st[kDsPositions] == 12291 && st[kDsTile] == kDrawTile && st[kDsLaunches] == 0);
    draw_stats_begin(st, 1, p, false);
    CHECK(st[kDsHostForSize] == 1 && st[kDsDevice] == 0);
    draw_stats_begin(st, 0, p, false);
    CHECK(st[kDsHostForSize] == 0 && st[kDsMode] == 0);
    CHECK(draw_fallbacks(nullptr, 0, st).empty());
  }
  std::printf(failures ? "%d checks failed\n" : "all checks hold\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
