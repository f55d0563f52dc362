// prerejective_draws.hip — the draws of ope_prerejective's LCG stream made on the device, entry for entry what prerej_draws
// (prerejective_math.hpp) makes on the host (gfx950, wave64).  DESIGN.md §4.26 has the argument; in short:
//
// Stream position p is the state after p steps from the seed; an LCG reaches it in <= 32 multiply-adds (x -> a_k x + c_k for the
// set bits k of p).  An iteration that starts at p takes len(p) positions: its distinct indices (an index that repeats is drawn
// again), then nr_samples picks.  len(p) depends on the stream alone, so every position can compute it; the iterations that really
// happen start at the chain 0 -> len(0) -> len(0) + len(len(0)) -> ...  The stream is cut into tiles of kDrawTile positions:
//   A. block (tile, problem): every lane computes len of its positions into LDS (0 = longer than the window W); lane e < W then
//      walks the chain that enters the tile at offset e and writes where it enters the next tile and how many iterations it started;
//   B. block (problem): composes the tiles' tables in order from offset 0 (chunks of tables staged in LDS, one lane walks): every
//      tile's true entry and first iteration; a needed iteration longer than W sets the problem's overflow bit, fewer than H
//      iterations started inside the P positions its short bit; a problem with a bit set has its whole slice of draws zeroed;
//   C. block (tile, problem): len again, one lane lists the tile's true starts, and lane k draws iteration first + k once more
//      from its own position and writes its S packed words (sample | pick << 12, the format prerej_batch_polygon_kernel reads).
// Every loop is bounded: a simulation by W steps, a walk by the tile, B by the tiles.  Flagged problems are drawn by the host.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "coarse_stages.hpp"
#include "prerejective_draws_plan.hpp"
#include "prerejective_math.hpp"
#include "stage_host.hpp"

namespace ope {
namespace {

constexpr uint64_t kLcgA = 6364136223846793005ULL, kLcgC = 1442695040888963407ULL;
constexpr int kDrawBlock = 256;
constexpr int kDrawPerLane = kDrawTile / kDrawBlock;
constexpr int kDrawStartsMax = kDrawTile / 6 + 2;     // an iteration takes at least 2 * 3 positions
constexpr int kDrawChunkWords = 8192;                 // kernel B stages this many table words at a time (32 KiB of LDS)
constexpr uint32_t kNoEntry = 0xffffffffu;
// a table word: exit offset into the next tile (12 bits) | iterations started << 12 | 1 << 31 when the chain met a len of 0
constexpr uint32_t kTabStuck = 0x80000000u;
static_assert(kDrawWindowMax <= 4096 && kDrawStartsMax < (1 << 12), "a table word holds 12 bits of each");
static_assert(kDrawTile % kDrawBlock == 0, "every lane takes the same number of positions");

// x -> a[k] x + c[k] is 2^k steps of the LCG
struct LcgJump { uint64_t a[32], c[32]; };
constexpr LcgJump lcg_jump_table() {
  LcgJump t{};
  uint64_t a = kLcgA, c = kLcgC;
  for (int k = 0; k < 32; ++k) {
    t.a[k] = a; t.c[k] = c;
    c = c * (a + 1);   // f(f(x)) = a (a x + c) + c
    a = a * a;
  }
  return t;
}
constexpr LcgJump kJump = lcg_jump_table();

__device__ __forceinline__ uint64_t lcg_at(uint64_t seed, uint32_t p) {
  uint64_t x = seed;
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if ((p >> k) & 1u) x = x * kJump.a[k] + kJump.c[k];
  return x;
}
__device__ __forceinline__ uint64_t lcg_step(uint64_t x) { return x * kLcgA + kLcgC; }
__device__ __forceinline__ double lcg_unit(uint64_t x) { return (double)(x >> 11) * (1.0 / 9007199254740992.0); }

// The iteration that starts at state x (prerej_draws' loop body): its length in positions, or 0 when it needs more than W.  With
// kEmit its S packed words go to out.  The samples live in eight named registers (no runtime-indexed array).
template <bool kEmit>
__device__ __forceinline__ uint32_t draw_iteration(uint64_t x, int ns, int S, int K, int W, uint16_t *__restrict__ out) {
  const double dns = (double)ns, dk = (double)K;
  int sm[kDrawMaxSamples];
#pragma unroll
  for (int i = 0; i < kDrawMaxSamples; ++i) sm[i] = -1;
  int cnt = 0;
  uint32_t used = 0;
  const uint32_t lim = (uint32_t)(W - S);   // the picks take S more
  while (cnt < S && used < lim) {
    x = lcg_step(x);
    ++used;
    const int si = (int)(dns * lcg_unit(x));
    bool fresh = true;
#pragma unroll
    for (int i = 0; i < kDrawMaxSamples; ++i) fresh = fresh && si != sm[i];
    if (fresh) {
#pragma unroll
      for (int i = 0; i < kDrawMaxSamples; ++i)
        if (i == cnt) sm[i] = si;
      ++cnt;
    }
  }
  if (cnt < S) return 0;
  if (kEmit) {
#pragma unroll
    for (int i = 0; i < kDrawMaxSamples; ++i)
      if (i < S) {
        x = lcg_step(x);
        const int pk = (int)(dk * lcg_unit(x));
        out[i] = (uint16_t)((uint32_t)sm[i] | ((uint32_t)pk << 12));
      }
  }
  return used + (uint32_t)S;
}

struct DrawArgs {
  const uint64_t *seeds;   // n
  uint32_t *tab;           // n * tiles * W table words
  uint32_t *ent;           // n * tiles * 2: entry offset (kNoEntry: the chain does not reach the tile), first iteration
  uint32_t P, tiles;
  int ns, S, K, H, W;
};

// len of every position of the block's tile into s_len (the block's 256 lanes, kDrawPerLane positions each, 256 apart)
__device__ __forceinline__ void tile_lengths(const DrawArgs &g, uint64_t seed, uint32_t base, uint16_t *__restrict__ s_len) {
  uint64_t x = lcg_at(seed, base + threadIdx.x);
#pragma unroll
  for (int j = 0; j < kDrawPerLane; ++j) {
    s_len[threadIdx.x + kDrawBlock * j] = (uint16_t)draw_iteration<false>(x, g.ns, g.S, g.K, g.W, nullptr);
    x = x * kJump.a[8] + kJump.c[8];   // 256 positions on
  }
}
static_assert(kDrawBlock == 256, "tile_lengths steps by kJump entry 8");

__global__ __launch_bounds__(kDrawBlock) void prerej_draws_tables_kernel(DrawArgs g) {
  __shared__ uint16_t s_len[kDrawTile];
  const uint32_t tile = blockIdx.x, a = blockIdx.y, base = tile * (uint32_t)kDrawTile;
  tile_lengths(g, g.seeds[a], base, s_len);
  __syncthreads();
  const uint32_t end = min((uint32_t)kDrawTile, g.P - base);   // starts count below P only
  uint32_t *row = g.tab + ((size_t)a * g.tiles + tile) * (size_t)g.W;
  for (uint32_t e = threadIdx.x; e < (uint32_t)g.W; e += kDrawBlock) {
    uint32_t off = e, cnt = 0, stuck = 0;
    for (int step = 0; step < kDrawStartsMax && off < end; ++step) {
      const uint32_t l = s_len[off];
      if (l == 0) { stuck = kTabStuck; break; }
      off += l;
      ++cnt;
    }
    const uint32_t exit = off >= (uint32_t)kDrawTile ? off - (uint32_t)kDrawTile : 0u;   // < W: the last len is <= W
    row[e] = exit | (cnt << 12) | stuck;
  }
}

__global__ __launch_bounds__(kDrawBlock) void prerej_draws_compose_kernel(DrawArgs g, uint32_t *__restrict__ words, uint16_t *__restrict__ draws) {
  __shared__ uint32_t s_tab[kDrawChunkWords];
  __shared__ uint32_t s_state[3];   // entry, iterations so far, the problem's word
  const uint32_t a = blockIdx.x, W = (uint32_t)g.W, H = (uint32_t)g.H, per = max(1u, (uint32_t)kDrawChunkWords / W);
  const uint32_t *tab = g.tab + (size_t)a * g.tiles * W;
  uint32_t *ent = g.ent + (size_t)a * g.tiles * 2;
  if (threadIdx.x == 0) { s_state[0] = 0; s_state[1] = 0; s_state[2] = 0; }
  for (uint32_t t0 = 0; t0 < g.tiles; t0 += per) {
    const uint32_t nt = min(per, g.tiles - t0);
    __syncthreads();   // (the walk of the last chunk has read s_tab)
    for (uint32_t j = threadIdx.x; j < nt * W; j += kDrawBlock) s_tab[j] = tab[(size_t)t0 * W + j];
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t e = s_state[0], it = s_state[1], word = s_state[2];
      for (uint32_t t = 0; t < nt; ++t) {
        const bool live = e != kNoEntry && it < H;
        ent[2 * (size_t)(t0 + t)] = live ? e : kNoEntry;
        ent[2 * (size_t)(t0 + t) + 1] = it;
        if (!live) { e = kNoEntry; continue; }
        const uint32_t w = s_tab[t * W + e];
        it += (w >> 12) & 0xfffu;
        if ((w & kTabStuck) && it < H) { word |= kDrawOverflow; e = kNoEntry; continue; }   // iteration `it` is needed and too long
        e = w & 0xfffu;
      }
      s_state[0] = e; s_state[1] = it; s_state[2] = word;
    }
  }
  __syncthreads();
  uint32_t word = s_state[2];
  if (!(word & kDrawOverflow) && s_state[1] < H) word |= kDrawShort;
  if (threadIdx.x == 0) words[a] = word;
  // A problem that falls back leaves iterations the emit kernel never writes, and the buffer comes uncleared from the pool: all its
  // words become draw 0 | 0 << 12 (in range for every ns and K) here, before the emit kernel writes the iterations that do start,
  // so that whoever reads the slice before the host has drawn it again (the batch's first prerejection) reads valid indices.
  if (word) {
    uint16_t *slice = draws + (size_t)a * H * (size_t)g.S;
    for (size_t j = threadIdx.x; j < (size_t)H * (size_t)g.S; j += kDrawBlock) slice[j] = 0;
  }
}

__global__ __launch_bounds__(kDrawBlock) void prerej_draws_emit_kernel(DrawArgs g, uint16_t *__restrict__ draws) {
  __shared__ uint16_t s_len[kDrawTile];
  __shared__ uint16_t s_start[kDrawBlock];
  __shared__ uint32_t s_n;
  const uint32_t tile = blockIdx.x, a = blockIdx.y, base = tile * (uint32_t)kDrawTile, H = (uint32_t)g.H;
  const uint32_t entry = g.ent[2 * ((size_t)a * g.tiles + tile)], first = g.ent[2 * ((size_t)a * g.tiles + tile) + 1];
  if (entry == kNoEntry) return;   // (the whole block: nothing starts here)
  const uint64_t seed = g.seeds[a];
  tile_lengths(g, seed, base, s_len);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t end = min((uint32_t)kDrawTile, g.P - base);
    uint32_t off = entry, k = 0;
    while (k < (uint32_t)kDrawBlock && off < end && first + k < H) {
      const uint32_t l = s_len[off];
      if (l == 0) break;
      s_start[k++] = (uint16_t)off;
      off += l;
    }
    s_n = k;
  }
  __syncthreads();
  if (threadIdx.x < s_n) {
    const uint32_t it = first + threadIdx.x;   // < H by the walk
    draw_iteration<true>(lcg_at(seed, base + s_start[threadIdx.x]), g.ns, g.S, g.K, g.W, draws + ((size_t)a * H + it) * (size_t)g.S);
  }
}
static_assert(kDrawStartsMax <= kDrawBlock, "one lane of the emit kernel per start of a tile");

}  // namespace

hipError_t draws_device_launch(ope_ctx *ctx, CallTmp &tmp, const DrawPlan &plan, int ns, int S, int K, int H, const uint64_t *seeds, size_t n,
                               uint16_t *d_draws, uint32_t **d_words, int64_t *launches, int64_t *host_syncs) {
  const hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  const size_t tiles = (size_t)plan.tiles;
  auto *d_seeds = (uint64_t *)tmp.get(8 * n, e);
  auto *d_tab = (uint32_t *)tmp.get(4 * n * tiles * (size_t)plan.W, e);
  auto *d_ent = (uint32_t *)tmp.get(8 * n * tiles, e);
  *d_words = (uint32_t *)tmp.get(4 * n, e);
  if (e == hipSuccess) e = upload_staged(st, d_seeds, seeds, 8 * n, launches, host_syncs);
  if (e != hipSuccess) return e;
  const DrawArgs g{d_seeds, d_tab, d_ent, (uint32_t)plan.P, (uint32_t)tiles, ns, S, K, H, plan.W};
  STAGE_LAUNCH(ctx, *launches, prerej_draws_tables_kernel, 4.0 * (double)n * (double)tiles * plan.W, dim3((unsigned)tiles, (unsigned)n),
               dim3(kDrawBlock), 0, st, g);
  STAGE_LAUNCH(ctx, *launches, prerej_draws_compose_kernel, (4.0 * plan.W + 8.0) * (double)n * (double)tiles, dim3((unsigned)n), dim3(kDrawBlock), 0,
               st, g, *d_words, d_draws);
  STAGE_LAUNCH(ctx, *launches, prerej_draws_emit_kernel, 8.0 * (double)n * (double)tiles + 2.0 * (double)n * (double)H * S,
               dim3((unsigned)tiles, (unsigned)n), dim3(kDrawBlock), 0, st, g, d_draws);
  return hipGetLastError();
}

}  // namespace ope

using namespace ope;

extern "C" {

int ope_prerejective_set_draws(ope_ctx *ctx, int mode) {
  if (!ctx) return OPE_EINVAL;
  if (mode != OPE_DRAWS_HOST && mode != OPE_DRAWS_DEVICE)
    return set_err(ctx, OPE_EINVAL, "ope_prerejective_set_draws: the mode is OPE_DRAWS_HOST or OPE_DRAWS_DEVICE");
  ctx->draws_mode = mode;
  return OPE_OK;
}

int ope_prerejective_set_draws_limits(ope_ctx *ctx, int window, int64_t budget) {
  if (!ctx) return OPE_EINVAL;
  if (window && (window < 2 * 3 || window > kDrawWindowMax))
    return set_err(ctx, OPE_EINVAL, "ope_prerejective_set_draws_limits: window must be 0 or 6 .. 1024");
  if (budget < 0) return set_err(ctx, OPE_EINVAL, "ope_prerejective_set_draws_limits: budget must be >= 0");
  ctx->draws_window = window;
  ctx->draws_budget = budget;
  return OPE_OK;
}

int ope_prerejective_get_draws(const ope_ctx *ctx, int *mode) {
  if (!ctx || !mode) return OPE_EINVAL;
  *mode = ctx->draws_mode;
  return OPE_OK;
}

int ope_prerejective_draws_device(ope_ctx *ctx, int ns, int S, int K, int H, const uint64_t *seeds, size_t n, int window, int64_t budget,
                                  int32_t *samples, int32_t *picks, int64_t *stats) {
  static const char *who = "ope_prerejective_draws_device: ";
  if (!ctx) return OPE_EINVAL;
  if (n == 0) return OPE_OK;
  if (!seeds || !samples || !picks) return set_err(ctx, OPE_EINVAL, std::string(who) + "bad argument");
  ope_prerejective_params p;
  ope_prerejective_default_params(&p);
  p.nr_samples = S; p.k_correspondences = K; p.max_iterations = H;
  if (const int rc = prerej_check_params(ctx, who, p)) return rc;
  if (ns < S || ns > 4096) return set_err(ctx, OPE_EINVAL, std::string(who) + "ns must be nr_samples .. 4096 (a draw packs the index in 12 bits)");
  if (window && (window < 2 * S || window > kDrawWindowMax)) return set_err(ctx, OPE_EINVAL, std::string(who) + "window must be 0 or 2 * nr_samples .. 1024");
  if (budget < 0) return set_err(ctx, OPE_EINVAL, std::string(who) + "budget must be >= 0");
  if (n > 65535) return set_err(ctx, OPE_EINVAL, std::string(who) + "more than 65535 problems (one grid row each)");
  if ((unsigned long long)n * (unsigned long long)H > 0x7fffffffull) return set_err(ctx, OPE_EINVAL, std::string(who) + "problems x iterations above 2^31 - 1");
  if (const int rc = refuse_communicator(ctx, who)) return rc;

  OPE_HIP(ctx, hipSetDevice(ctx->device));
  const DrawPlan plan = draw_plan(ns, S, H, n, window, budget);
  int64_t *ds = ctx->draws_stats;
  draw_stats_begin(ds, OPE_DRAWS_DEVICE, plan, plan.fits);
  const size_t HS = (size_t)H * S;
  std::vector<size_t> again;
  if (!plan.fits) {
    for (size_t a = 0; a < n; ++a) again.push_back(a);
  } else {
    const hipStream_t st = ctx->stream;
    CallTmp tmp{st, {}};
    hipError_t e = hipSuccess;
    auto *d_draws = (uint16_t *)tmp.get(2 * n * HS, e);
    uint32_t *d_words = nullptr;
    int64_t syncs = 0;
    if (e == hipSuccess) e = draws_device_launch(ctx, tmp, plan, ns, S, K, H, seeds, n, d_draws, &d_words, &ds[kDsLaunches], &syncs);
    std::vector<uint16_t> packed(n * HS);
    std::vector<uint32_t> words(n);
    if (e == hipSuccess) e = hipMemcpyAsync(packed.data(), d_draws, 2 * n * HS, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(words.data(), d_words, 4 * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_err(ctx, OPE_EHIP, std::string(who) + hipGetErrorString(e));
    again = draw_fallbacks(words.data(), n, ds);
    for (size_t a = 0, f = 0; a < n; ++a) {
      if (f < again.size() && again[f] == a) { ++f; continue; }
      for (size_t j = a * HS; j < (a + 1) * HS; ++j) { samples[j] = (int32_t)(packed[j] & 0xfffu); picks[j] = (int32_t)(packed[j] >> 12); }
    }
  }
  for (const size_t a : again) prerej_draws(ns, S, K, H, seeds[a], samples + a * HS, picks + a * HS);
  if (stats) std::memcpy(stats, ds, sizeof ctx->draws_stats);
  return OPE_OK;
}

int ope_prerejective_draws_last_stats(const ope_ctx *ctx, int64_t out[8]) {
  if (!ctx || !out) return OPE_EINVAL;
  std::memcpy(out, ctx->draws_stats, sizeof ctx->draws_stats);
  return OPE_OK;
}

}  // extern "C"
