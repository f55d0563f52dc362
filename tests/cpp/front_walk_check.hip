// Stand-alone check of bvh_traverse_front<W> (csrc/bvh_traverse.hpp): every query through the walk for W = 2, 4, 8 lanes per
// query, with no hint, the true leaf and a deliberately wrong leaf as start, against a brute-force scan in this program.
// One more instantiation has its pending stack cut to 4 entries, so that the overflow path (the private trail) runs on every
// far query.  d2 must agree bit for bit; the index may differ only where d2 is equal; the leaf returned must hold the point
// returned; all W lanes must come back with the same answer.
//
// Targets: 3, 17, 1 000 and 20 000 points on a bumpy surface, and 20 000 coplanar points on a lattice (exact ties abound),
// each indexed by the library's own build_bvh_device (leaf size 16).  Queries: 4 096, half of them on the surface, half 5-20 cm
// away from it.  Prints one line per (target, walk, hint) with the mismatch counts and "front_walk_check: N mismatches" last;
// exit status 0 iff N == 0.  Built by tests/test_gpu_front_walk.py: hipcc --offload-arch=gfx950 against libope_hip.so.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bvh_traverse.hpp"

namespace ope {
hipError_t build_bvh_device(hipStream_t stream, const float4 *d_src, const float4 *d_src_nrm, size_t n, int leaf_size, const float bb_lo[3],
                            const float bb_hi[3], int *out_depth, float4 **d_nodes, float4 **d_pts, float4 **d_nrm, float4 **d_axis2, bool tmp_alloc);
}

using namespace ope;

#define CHECK(x)                                                                        \
  do {                                                                                  \
    const hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                             \
      std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return 2;                                                                         \
    }                                                                                   \
  } while (0)

constexpr int kBlock = 256;

// nearest point of the index by a scan of all its points, in index order (the first of equal distances wins)
__global__ void brute_kernel(BvhView t, const float4 *__restrict__ q, uint32_t nq, float *__restrict__ d2, uint32_t *__restrict__ pos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const float4 p = q[i];
  float best = INFINITY;
  uint32_t bp = kNoPos;
  for (uint32_t j = 0; j < t.n; ++j) {
    const float4 c = t.pts[j];
    const float d = sq_dist3(__fsub_rn(p.x, c.x), __fsub_rn(p.y, c.y), __fsub_rn(p.z, c.z));
    if (d < best) { best = d; bp = j; }
  }
  d2[i] = best;
  pos[i] = bp;
}

// W consecutive lanes carry query (global thread id) / W; lane 0 of the group reports, `differ` counts groups whose lanes disagree
template <int W, int CAP>
__global__ __launch_bounds__(kBlock) void front_kernel(BvhView t, const float4 *__restrict__ q, const uint32_t *__restrict__ hint, uint32_t nq,
                                                       float *__restrict__ d2, uint32_t *__restrict__ pos, uint32_t *__restrict__ leaf,
                                                       uint32_t *__restrict__ differ) {
  __shared__ float s_stk[kMaxDepth + 2][kBlock];
  const uint32_t tid = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t i = tid / W;
  if (i >= nq) return;   // (whole groups)
  const float4 p = q[i];
  NearestVisitor v{INFINITY, kNoPos, 0};
  bvh_traverse_front<W, CAP>(t, p.x, p.y, p.z, v, &s_stk[0][threadIdx.x & ~(W - 1)], kBlock, hint ? hint[i] : 0u);
  const int first = (int)((threadIdx.x & 63u) & ~(uint32_t)(W - 1));
  const bool same = __float_as_uint(v.best) == (uint32_t)__shfl((int)__float_as_uint(v.best), first, 64) &&
                    v.pos == (uint32_t)__shfl((int)v.pos, first, 64) && v.leaf == (uint32_t)__shfl((int)v.leaf, first, 64);
  if (!same) atomicAdd(differ, 1u);
  if ((threadIdx.x & (W - 1)) == 0) {
    d2[i] = v.best;
    pos[i] = v.pos;
    leaf[i] = v.leaf;
  }
}

struct Target {
  const char *name;
  std::vector<float4> pts;
};

static float4 surface_point(std::mt19937 &rng) {
  std::uniform_real_distribution<float> u(-0.15f, 0.15f);
  const float x = u(rng), y = u(rng);
  return make_float4(x, y, 0.03f * std::sin(20.f * x) * std::cos(17.f * y) + 0.4f * x * y, 0.f);
}

int main() {
  std::mt19937 rng(12345);
  std::vector<Target> targets;
  for (int n : {3, 17, 1000, 20000}) {
    Target t{n == 3 ? "surface_3" : n == 17 ? "surface_17" : n == 1000 ? "surface_1000" : "surface_20000", {}};
    for (int i = 0; i < n; ++i) t.pts.push_back(surface_point(rng));
    targets.push_back(t);
  }
  {
    // 200 x 100 lattice in the plane z = 0, spacing 1/512 (exact in fp32): a query above a cell's centre is equally far from four points
    Target t{"coplanar_20000", {}};
    for (int i = 0; i < 200; ++i)
      for (int j = 0; j < 100; ++j) t.pts.push_back(make_float4((float)(i - 100) / 512.f, (float)(j - 50) / 512.f, 0.f, 0.f));
    targets.push_back(t);
  }
  hipStream_t stream;
  CHECK(hipStreamCreate(&stream));
  constexpr uint32_t nq = 4096;
  unsigned long long total_bad = 0;
  for (Target &tg : targets) {
    const size_t n = tg.pts.size();
    for (size_t i = 0; i < n; ++i) { int idx = (int)i; std::memcpy(&tg.pts[i].w, &idx, 4); }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const float4 &p : tg.pts) {
      lo[0] = std::fmin(lo[0], p.x); lo[1] = std::fmin(lo[1], p.y); lo[2] = std::fmin(lo[2], p.z);
      hi[0] = std::fmax(hi[0], p.x); hi[1] = std::fmax(hi[1], p.y); hi[2] = std::fmax(hi[2], p.z);
    }
    float4 *d_src = nullptr, *d_nodes = nullptr, *d_pts = nullptr, *d_nrm = nullptr, *d_axis2 = nullptr;
    CHECK(hipMalloc((void **)&d_src, sizeof(float4) * n));
    CHECK(hipMemcpy(d_src, tg.pts.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    int D = 0;
    CHECK(build_bvh_device(stream, d_src, nullptr, n, 16, lo, hi, &D, &d_nodes, &d_pts, &d_nrm, &d_axis2, false));
    BvhView view{};
    view.nodes = d_nodes; view.pts = d_pts; view.nrm = nullptr; view.n = (uint32_t)n; view.depth = D; view.axis2 = d_axis2;
    std::vector<float4> ipts(n);
    CHECK(hipMemcpy(ipts.data(), d_pts, sizeof(float4) * n, hipMemcpyDeviceToHost));
    // leaf of every position of the index
    std::vector<uint32_t> leaf_of(n);
    for (uint32_t j = 0; j < (1u << D); ++j) {
      const uint32_t s = (uint32_t)(((unsigned long long)j * n) >> D), e = (uint32_t)(((unsigned long long)(j + 1) * n) >> D);
      for (uint32_t k = s; k < e; ++k) leaf_of[k] = (1u << D) + j;
    }
    // queries: even ones on the surface (a target point, nudged), odd ones 5-20 cm off it
    std::vector<float4> q(nq);
    std::uniform_int_distribution<size_t> pick(0, n - 1);
    std::uniform_real_distribution<float> far(0.05f, 0.20f), nudge(-2e-4f, 2e-4f), side(-0.02f, 0.02f);
    const bool lattice = std::strncmp(tg.name, "coplanar", 8) == 0;
    for (uint32_t i = 0; i < nq; ++i) {
      const float4 p = tg.pts[pick(rng)];
      if (lattice) {
        // above (or, on the surface, at) the centre of a lattice cell: four-way ties, exact
        const float cx = p.x + 1.f / 1024.f, cy = p.y + 1.f / 1024.f;
        q[i] = (i & 1u) ? make_float4(cx, cy, (float)(26 + (int)(i % 77)) / 512.f, 0.f) : make_float4(cx, cy, 0.f, 0.f);
      } else if (i & 1u) {
        q[i] = make_float4(p.x + side(rng), p.y + side(rng), p.z + ((i & 2u) ? 1.f : -1.f) * far(rng), 0.f);
      } else {
        q[i] = make_float4(p.x + nudge(rng), p.y + nudge(rng), p.z + nudge(rng), 0.f);
      }
    }
    float4 *d_q = nullptr;
    float *d_bd2 = nullptr, *d_d2 = nullptr;
    uint32_t *d_bpos = nullptr, *d_pos = nullptr, *d_leaf = nullptr, *d_hint = nullptr, *d_differ = nullptr;
    CHECK(hipMalloc((void **)&d_q, sizeof(float4) * nq));
    CHECK(hipMalloc((void **)&d_bd2, 4 * nq)); CHECK(hipMalloc((void **)&d_d2, 4 * nq));
    CHECK(hipMalloc((void **)&d_bpos, 4 * nq)); CHECK(hipMalloc((void **)&d_pos, 4 * nq));
    CHECK(hipMalloc((void **)&d_leaf, 4 * nq)); CHECK(hipMalloc((void **)&d_hint, 4 * nq));
    CHECK(hipMalloc((void **)&d_differ, 4));
    CHECK(hipMemcpy(d_q, q.data(), sizeof(float4) * nq, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(brute_kernel, dim3((nq + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, view, d_q, nq, d_bd2, d_bpos);
    CHECK(hipStreamSynchronize(stream));
    std::vector<float> bd2(nq), d2(nq);
    std::vector<uint32_t> bpos(nq), pos(nq), leaf(nq);
    CHECK(hipMemcpy(bd2.data(), d_bd2, 4 * nq, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bpos.data(), d_bpos, 4 * nq, hipMemcpyDeviceToHost));
    std::vector<uint32_t> hint_true(nq), hint_wrong(nq);
    for (uint32_t i = 0; i < nq; ++i) {
      hint_true[i] = leaf_of[bpos[i]];
      hint_wrong[i] = leaf_of[pick(rng)];
    }
    const char *hint_names[3] = {"none", "true", "wrong"};
    for (int h = 0; h < 3; ++h) {
      if (h == 1) CHECK(hipMemcpy(d_hint, hint_true.data(), 4 * nq, hipMemcpyHostToDevice));
      if (h == 2) CHECK(hipMemcpy(d_hint, hint_wrong.data(), 4 * nq, hipMemcpyHostToDevice));
      const uint32_t *hp = h == 0 ? nullptr : d_hint;
      for (int variant = 0; variant < 4; ++variant) {
        CHECK(hipMemset(d_differ, 0, 4));
        CHECK(hipMemset(d_d2, 0xff, 4 * nq)); CHECK(hipMemset(d_pos, 0xff, 4 * nq)); CHECK(hipMemset(d_leaf, 0, 4 * nq));
        const int W = variant == 0 ? 2 : variant == 3 ? 4 : 4 * variant;   // 2, 4, 8, and 4 with the stack cut
        const dim3 grid((nq * (uint32_t)W + kBlock - 1) / kBlock), block(kBlock);
        if (variant == 0) hipLaunchKernelGGL((front_kernel<2, 2 * (kMaxDepth + 1)>), grid, block, 0, stream, view, d_q, hp, nq, d_d2, d_pos, d_leaf, d_differ);
        if (variant == 1) hipLaunchKernelGGL((front_kernel<4, 4 * (kMaxDepth + 1)>), grid, block, 0, stream, view, d_q, hp, nq, d_d2, d_pos, d_leaf, d_differ);
        if (variant == 2) hipLaunchKernelGGL((front_kernel<8, 8 * (kMaxDepth + 1)>), grid, block, 0, stream, view, d_q, hp, nq, d_d2, d_pos, d_leaf, d_differ);
        if (variant == 3) hipLaunchKernelGGL((front_kernel<4, 4>), grid, block, 0, stream, view, d_q, hp, nq, d_d2, d_pos, d_leaf, d_differ);
        CHECK(hipStreamSynchronize(stream));
        uint32_t differ = 0;
        CHECK(hipMemcpy(&differ, d_differ, 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(d2.data(), d_d2, 4 * nq, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(pos.data(), d_pos, 4 * nq, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(leaf.data(), d_leaf, 4 * nq, hipMemcpyDeviceToHost));
        unsigned bad_d2 = 0, bad_pos = 0, bad_leaf = 0, other_index = 0;
        for (uint32_t i = 0; i < nq; ++i) {
          if (std::memcmp(&d2[i], &bd2[i], 4) != 0) { ++bad_d2; continue; }
          if (pos[i] >= n) { ++bad_pos; continue; }
          if (pos[i] != bpos[i]) {
            // allowed only where the distance is the same bits
            const float4 c = ipts[pos[i]];
            const float dx = q[i].x - c.x, dy = q[i].y - c.y, dz = q[i].z - c.z;
            volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            volatile float s1 = xx + yy;
            const float d = s1 + zz;
            if (std::memcmp(&d, &bd2[i], 4) != 0) ++bad_pos; else ++other_index;
          }
          if (leaf[i] != leaf_of[pos[i]]) ++bad_leaf;
        }
        std::printf("%-15s D=%2d W=%d cap=%-3d hint=%-5s  d2 %u  index %u  leaf %u  lanes %u  (other index of an equal d2: %u)\n", tg.name, D, W,
                    variant == 3 ? 4 : W * (kMaxDepth + 1), hint_names[h], bad_d2, bad_pos, bad_leaf, differ, other_index);
        total_bad += bad_d2 + bad_pos + bad_leaf + differ;
      }
    }
    for (void *p : {(void *)d_q, (void *)d_bd2, (void *)d_d2, (void *)d_bpos, (void *)d_pos, (void *)d_leaf, (void *)d_hint, (void *)d_differ, (void *)d_src,
                    (void *)d_nodes, (void *)d_pts, (void *)d_axis2})
      CHECK(hipFree(p));
  }
  CHECK(hipStreamDestroy(stream));
  std::printf("front_walk_check: %llu mismatches\n", total_bad);
  return total_bad == 0 ? 0 : 1;
}
