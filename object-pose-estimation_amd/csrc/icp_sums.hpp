// icp_sums.hpp — one query per lane -> the wave's 17 (44) ICP sums {n, Σs, Σt, Σ t sᵀ, Σd²} (+ 27 normal-equation sums of the
// point-to-plane estimator).  Shared by the accumulate kernels (icp_kernels.hip) and the batched kernel (icp_batch.hip), so the
// terms and the order of their additions inside a wave are the same wherever they are restated.
//
// Every term is formed in fp64 from fp32 values (differences and products of fp32 values are exact in fp64), so the sums do
// not depend, beyond 1e-16, on how queries are grouped into lanes, chunks, waves or ranks.
//
// The count n is a population count of the wave's `ok` ballot.  The 16 other terms are summed over the wave by a REDUCE-SCATTER
// of four stages: at each stage a lane keeps one half of its values and adds its partner's copy of that half, so the live
// values per lane go 16 -> 8 -> 4 -> 2 -> 1 and each of the 15 pairings is added once (a butterfly that leaves every lane with
// every total adds each of them 16 times over):
//   stage 1  halves of the wave  (v_permlane32_swap: lanes 32-63 of one register <-> lanes 0-31 of the other, then one add)
//   stage 2  neighbouring rows   (v_permlane16_swap: odd 16-lane rows of one register <-> even rows of the other, one add)
//   stage 3  lanes 8 apart       (DPP row_ror:8; the `old` operand and bank masks do the keep and the receive in one move)
//   stage 4  lanes 4 apart       (DPP row_shr:4 / row_shl:4, bank masks)
// Stages 1 and 2 are the gfx950 swaps: two registers in, two out, nothing computed twice and nothing selected.
// The stages are walked depth first: values 0 and 1 are paired as soon as both exist, their sum with that of 2 and 3, and so
// on, so at most four partial sums are live next to the pair being formed (stage by stage it would be eight), and an input
// that only the first values need is dead after them.  In that order the value a lane ends up with is the bit reversal of
// its quad's number: LANE l HOLDS VALUE rev4(l >> 2), summed over the 16 lanes of the wave congruent to l modulo 4 — the four
// lanes of a quad hold the four quarters of one value's wave total.  They are added into the value's LDS slot either by one
// ds_add_f64 from all 64 lanes (four lanes per address) or, where the caller wants a single writer per slot, after two
// quad_perm steps by the quad's first lane.
#pragma once

#include "bvh_traverse.hpp"

namespace ope {

typedef const __attribute__((address_space(3))) float *lds_cfloat_ptr;   // a pointer that stays an LDS pointer

// a (kept by lanes 0-31) and b (kept by lanes 32-63): own half + the other half-wave's copy of it
__device__ __forceinline__ double half_swap_add(double a, double b) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// a (kept by rows 0 and 2) and b (kept by rows 1 and 3): own + the neighbouring row's copy
__device__ __forceinline__ double row_swap_add(double a, double b) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// In the banks of KEEP_A (a mask of the row's four banks of four lanes) a lane keeps a and receives its partner's a; in the
// other banks it keeps b and receives b.  CTRL_A / CTRL_B: the DPP moves that bring the partner's value to the banks keeping a / b.
template <int CTRL_A, int CTRL_B, int KEEP_A>
__device__ __forceinline__ double bank_pair_add(double a, double b) {
  constexpr int KEEP_B = 0xf & ~KEEP_A;
  // u: own a where a is kept, the partner's b elsewhere; v: the partner's a where a is kept, own b elsewhere
  const int ulo = __builtin_amdgcn_update_dpp(__double2loint(a), __double2loint(b), CTRL_B, 0xf, KEEP_B, false);
  const int uhi = __builtin_amdgcn_update_dpp(__double2hiint(a), __double2hiint(b), CTRL_B, 0xf, KEEP_B, false);
  const int vlo = __builtin_amdgcn_update_dpp(__double2loint(b), __double2loint(a), CTRL_A, 0xf, KEEP_A, false);
  const int vhi = __builtin_amdgcn_update_dpp(__double2hiint(b), __double2hiint(a), CTRL_A, 0xf, KEEP_A, false);
  return __hiloint2double(uhi, ulo) + __hiloint2double(vhi, vlo);
}

// term(j), j = 0 .. 15: this lane's 16 values, asked for in that order.  Returns the wave's sum of value scattered_value(lane)
// over the lanes congruent to this one modulo 4.  Every lane of the wave must be here.
template <class F>
__device__ __forceinline__ double wave_reduce_scatter16(F term) {
  double y[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double x[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int j = 8 * i + 4 * k;
      const double w0 = half_swap_add(term(j), term(j + 1));       // lanes 0-31: value j, lanes 32-63: value j + 1
      const double w1 = half_swap_add(term(j + 2), term(j + 3));
      x[k] = row_swap_add(w0, w1);                                  // rows 1 and 3: value + 2
    }
    y[i] = bank_pair_add<0x128, 0x128, 0x3>(x[0], x[1]);           // row_ror:8.  Lanes 8-15 of a row: value + 4
  }
  return bank_pair_add<0x104, 0x114, 0x5>(y[0], y[1]);   // row_shl:4 into banks 0 and 2, row_shr:4 into banks 1 and 3: value + 8
}
// bit 5 of the lane (the half) selects bit 0 of the value, bit 4 (the row) bit 1, bit 3 bit 2 and bit 2 bit 3
__device__ __forceinline__ uint32_t scattered_value(uint32_t lane_id) { return __brev(lane_id >> 2) >> 28; }

// Adds r, the lane's result of wave_reduce_scatter16, into *slot: the slot of value scattered_value(lane), the same for the four
// lanes of a quad (write == false: the lane holds padding).
// ATOMIC: one ds_add_f64 from every lane; otherwise the quad is summed first and its first lane is the slot's only writer.
template <bool ATOMIC>
__device__ __forceinline__ void scatter_add(double *slot, uint32_t lane_id, double r, bool write = true) {
  if (ATOMIC) {
    if (write) unsafeAtomicAdd(slot, r);
  } else {
    r += dpp_move_f64<0xB1>(r);   // quad_perm [1,0,3,2]
    r += dpp_move_f64<0x4E>(r);   // quad_perm [2,3,0,1]
    if ((lane_id & 3u) == 0u && write) *slot += r;
  }
}

// The order in which the 16 terms are formed: j = 4 T + S is t_T s_S, with index 3 standing for "1": j = 3, 7, 11 are tx, ty, tz,
// j = 12, 13, 14 are sx, sy, sz, and j = 15 is d² — each t component is dead after its four values.  Where they go, as a slot of
// the sums {n, s[3], t[3], t sᵀ[9] by rows, d²}:
__host__ __device__ constexpr int sum_slot_of_term(int j) {
  const int T = j >> 2, S = j & 3;
  return T < 3 ? (S < 3 ? 7 + 3 * T + S : 4 + T) : (S < 3 ? 1 + S : 16);
}
// (the 16 slots less one, one nibble per value)
__host__ __device__ constexpr unsigned long long sum_slot_nibbles() {
  unsigned long long k = 0;
  for (int j = 0; j < 16; ++j) k |= (unsigned long long)(sum_slot_of_term(j) - 1) << (4 * j);
  return k;
}

// the 27 point-to-plane sums in their slot order: the upper triangle of AᵀA by rows, then Aᵀb; v[6] is the right-hand side
__host__ __device__ constexpr int p2p_sum_row(int j) {
  if (j >= 21) return j - 21;
  int r = 0;
  for (int n = 6; j >= n; --n) { j -= n; ++r; }
  return r;
}
__host__ __device__ constexpr int p2p_sum_col(int j) {
  if (j >= 21) return 6;
  int r = 0;
  for (int n = 6; j >= n; --n) { j -= n; ++r; }
  return r + j;
}

// The same sums, each term reduced on its own over its 16-lane row (row16_sum: two live registers, every row total computed 16
// times over), then one ds_add_f64 per row and sum.  What every accumulate kernel did before the reduce-scatter, kept for the
// normal-shooting instantiations: they sit at their register bound and gained registers or scratch with
// anything else here.
template <bool NRM>
__device__ __forceinline__ void add_query_sums_by_rows(double *acc, lds_cfloat_ptr cs2, uint32_t lane_id, bool ok, bool p2p, float x, float y, float z,
                                                       const float4 t, const float4 tn, float d2) {
  asm volatile("" : "+v"(cs2));
  const float psx = cs2[12], psy = cs2[13], psz = cs2[14];
  const double sx = (double)x - (double)psx, sy = (double)y - (double)psy, sz = (double)z - (double)psz;
  const double tx = (double)t.x - (double)psx, ty = (double)t.y - (double)psy, tz = (double)t.z - (double)psz;
  const double w = ok ? 1.0 : 0.0;
  double term[kNumSums];
  term[0] = w;
  term[1] = w * sx; term[2] = w * sy; term[3] = w * sz;
  term[4] = w * tx; term[5] = w * ty; term[6] = w * tz;
  term[7] = w * (tx * sx); term[8] = w * (tx * sy); term[9] = w * (tx * sz);
  term[10] = w * (ty * sx); term[11] = w * (ty * sy); term[12] = w * (ty * sz);
  term[13] = w * (tz * sx); term[14] = w * (tz * sy); term[15] = w * (tz * sz);
  term[16] = ok ? (double)d2 : 0.0;
#pragma unroll
  for (int k = 0; k < kNumSums; ++k) {
    const double r = row16_sum(term[k]);
    if ((lane_id & 15u) == 0u) unsafeAtomicAdd(acc + k, r);
  }
  if (NRM && p2p) {
    // TransformationEstimationPointToPlaneLLS (see add_query_sums): products in float, sums in double
    const float v0 = __fsub_rn(__fmul_rn(tn.z, y), __fmul_rn(tn.y, z));
    const float v1 = __fsub_rn(__fmul_rn(tn.x, z), __fmul_rn(tn.z, x));
    const float v2 = __fsub_rn(__fmul_rn(tn.y, x), __fmul_rn(tn.x, y));
    const float dd = __fsub_rn(__fsub_rn(__fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(tn.x, t.x), __fmul_rn(tn.y, t.y)), __fmul_rn(tn.z, t.z)),
                                                     __fmul_rn(tn.x, x)), __fmul_rn(tn.y, y)), __fmul_rn(tn.z, z));
    const double v[6] = {w * (double)v0, w * (double)v1, w * (double)v2, w * (double)tn.x, w * (double)tn.y, w * (double)tn.z};
    int slot = kNumSums;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        const double sum = row16_sum(v[r] * v[c]);
        if ((lane_id & 15u) == 0u) unsafeAtomicAdd(acc + slot, sum);
        ++slot;
      }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double sum = row16_sum(v[r] * (double)dd);
      if ((lane_id & 15u) == 0u) unsafeAtomicAdd(acc + slot, sum);
      ++slot;
    }
  }
}

// One query's contribution to the wave's running sums in `acc` (LDS; kNumSums slots, kNumSumsMax with the point-to-plane
// estimator).  t: the matched target point, tn: its normal (point-to-plane only); lanes with ok == false contribute zeros:
// their fp32 inputs are replaced (points by the pivot, the rest by zero) before anything is widened, so their terms are the
// zeros a 0/1 weight would make of them.
// Lane -> component: lane 0 adds n into acc[0]; lane l adds into acc[sum_slot_of_term(rev4(l >> 2))] — quads 0, 8, 4 (lanes 0-3,
// 32-35, 16-19) Σ tx s, quad 12 Σtx; quads 2, 10, 6 Σ ty s, quad 14 Σty; quads 1, 9, 5 Σ tz s, quad 13 Σtz; quads 3, 11, 7 Σs;
// quad 15 Σd².  The point-to-plane sums follow as two groups of 16, lane l adding sum rev4(l >> 2) and sum 16 + rev4(l >> 2).
// SCATTER == false (accumulate kernels only: it adds with LDS atomics): add_query_sums_by_rows instead.
template <bool NRM, bool ATOMIC, bool SCATTER = true>
__device__ __forceinline__ void add_query_sums(double *acc, lds_cfloat_ptr cs2, uint32_t lane_id, bool ok, bool p2p, float x, float y, float z,
                                               const float4 t, const float4 tn, float d2) {
  static_assert(ATOMIC || SCATTER, "row sums have four writers per slot of a wave's row");
  if (!SCATTER) return add_query_sums_by_rows<NRM>(acc, cs2, lane_id, ok, p2p, x, y, z, t, tn, d2);
  // (through values the optimiser cannot see through: what it could hoist out of the caller's loop — the pivot, the slot
  // addresses — it would hold in registers across the walks)
  asm volatile("" : "+v"(cs2), "+v"(lane_id));
  const float psx = cs2[12], psy = cs2[13], psz = cs2[14];
  const unsigned long long okm = __ballot(ok);
  const double n = (double)(int)(__popc((unsigned)okm) + __popc((unsigned)(okm >> 32)));   // (a small integer: exact)
  if (lane_id == 0u) {
    if (ATOMIC) unsafeAtomicAdd(acc, n);
    else acc[0] += n;
  }
  const float s32[3] = {ok ? x : psx, ok ? y : psy, ok ? z : psz};
  const float t32[3] = {ok ? t.x : psx, ok ? t.y : psy, ok ? t.z : psz};
  const float d32 = ok ? d2 : 0.f;
  const float ps[3] = {psx, psy, psz};
  const uint32_t jv = scattered_value(lane_id);
  const auto term = [&](int j) -> double {
    const int T = j >> 2, S = j & 3;
    if (j == 15) return (double)d32;
    if (T == 3) return (double)s32[S] - (double)ps[S];
    if (S == 3) return (double)t32[T] - (double)ps[T];
    return ((double)t32[T] - (double)ps[T]) * ((double)s32[S] - (double)ps[S]);
  };
  const double r = wave_reduce_scatter16(term);
  scatter_add<ATOMIC>(acc + 1 + (uint32_t)((sum_slot_nibbles() >> (4u * jv)) & 15ull), lane_id, r);
  if (NRM && p2p) {
    // TransformationEstimationPointToPlaneLLS: row v = (s x n, n), right-hand side d = n . (t - s);
    // the reference forms these products in float (operands are const float&), sums in double
    const float v0 = __fsub_rn(__fmul_rn(tn.z, y), __fmul_rn(tn.y, z));
    const float v1 = __fsub_rn(__fmul_rn(tn.x, z), __fmul_rn(tn.z, x));
    const float v2 = __fsub_rn(__fmul_rn(tn.y, x), __fmul_rn(tn.x, y));
    const float dd = __fsub_rn(__fsub_rn(__fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(tn.x, t.x), __fmul_rn(tn.y, t.y)), __fmul_rn(tn.z, t.z)),
                                                     __fmul_rn(tn.x, x)), __fmul_rn(tn.y, y)), __fmul_rn(tn.z, z));
    const double v[7] = {(double)(ok ? v0 : 0.f), (double)(ok ? v1 : 0.f), (double)(ok ? v2 : 0.f), (double)(ok ? tn.x : 0.f),
                         (double)(ok ? tn.y : 0.f), (double)(ok ? tn.z : 0.f), (double)(ok ? dd : 0.f)};
    constexpr int kP2p = kNumSumsMax - kNumSums;   // 27: one full group of 16, one of 11 padded with zeros
    const double r0 = wave_reduce_scatter16([&](int j) -> double { return v[p2p_sum_row(j)] * v[p2p_sum_col(j)]; });
    scatter_add<ATOMIC>(acc + kNumSums + jv, lane_id, r0);
    const double r1 = wave_reduce_scatter16([&](int j) -> double { return 16 + j < kP2p ? v[p2p_sum_row(16 + j)] * v[p2p_sum_col(16 + j)] : 0.0; });
    scatter_add<ATOMIC>(acc + kNumSums + 16 + jv, lane_id, r1, 16 + jv < (uint32_t)kP2p);
  }
}

}  // namespace ope
