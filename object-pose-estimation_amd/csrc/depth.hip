// depth.hip — the frame's ingest (gfx950, wave64): DataGrabber::rgbd2Pcl + depthToMeter (DetectAndLocalize/src/datagrabber.cpp:65-174)
// and, optionally, the workspace crop getPassThrough (rosinterface.cpp:212) on the 16-bit depth image.  DESIGN.md §4.12.
//
// The output order is the reference's loop order, columns outer and rows inner, over a ROW-major image.  Read naively that is a
// 2-byte load at a stride of one image row per lane.  Instead a workgroup of four waves takes a tile of 64 rows x 64 columns:
//   load      16 lanes read one tile row (128 B, 8 B each), 16 rows per step: whole cache lines;
//   transpose the tile lies in LDS with a pitch of 33 words, so the 64 lanes of a wave read ONE column (lane = row) from 64
//             different banks;
//   count     a wave takes 16 columns; per column __ballot gives the survivors of that (column, 64-row) segment, one count each;
//   scan      one exclusive scan over the segments in column-major order (5120 for 640 x 480) gives every segment's first
//             output position and the total;
//   scatter   the same tiles again: the points are recomputed (cheaper than keeping them), lane rank = mbcnt of the ballot, so
//             consecutive surviving lanes write consecutive points and pixel indices; the bounding box goes through ordered
//             integer keys (wave reduction, LDS, one atomic per block and word: min and max are exact in any order).
// One host synchronisation brings back the count and the boxes; morton_order_device then orders the cloud as ope_cloud_upload does.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

#include "ope_internal.hpp"

namespace ope {

namespace {

constexpr int kTile = 64;        // rows and columns of a tile; a wave's lanes are the tile's rows
constexpr int kTilePitch = 33;   // words per tile row in LDS: 32 hold the 64 samples, 1 pads (column reads hit 64 banks)
constexpr int kBgrPitch = 49;    // the colour tile: 48 words hold a row's 64 x 3 bytes, 1 pads (odd: a column read hits 64 banks)
constexpr int kDepthBlock = 256;
constexpr int kColsPerWave = kTile / (kDepthBlock / 64);
// What morton_order_device is booked as in ope_depth_stats: its key kernel, its one rocPRIM sort call (however many kernels
// that issues inside) and its gather, and its synchronisation.  Booked, not counted: an empty cloud orders nothing.
constexpr int kMortonLaunches = 3, kMortonSyncs = 1;

struct DepthJob {
  // the frame on the device, row_bytes per image row: pitch depth samples (pitch a multiple of kTile) and, for a coloured
  // frame, the row's pitch BGR pixels behind them (bgr_off = 2 * pitch; both parts start on a multiple of 64 bytes)
  const unsigned char *img;
  uint32_t rows, cols, pitch, row_tiles, col_tiles, row_bytes, bgr_off;
  float f_row, c_row, f_col, c_col, scale;
  double z_max;
  int crop;
  float lo[3], hi[3];
};

// words of the result block: the box and count of the valid pixels (count pass), the box and finite count of the kept ones (scatter pass)
enum { kValidLo = 0, kValidCount = 3, kValidHi = 4, kKeptLo = 8, kKeptFinite = 11, kKeptHi = 12, kResultWords = 16 };

__device__ __forceinline__ uint32_t ordered_key(float v) {
  const uint32_t u = (uint32_t)__float_as_int(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The box of the points a block has seen (ordered keys kept per lane) and a count: wave reduction, the block's waves through
// LDS, one atomic per block and word.
__device__ __forceinline__ void block_commit(uint32_t klo[3], uint32_t khi[3], uint32_t wave_count, bool with_box, uint32_t *__restrict__ res,
                                             int lo_word, int hi_word, int count_word) {
  __shared__ uint32_t s_lo[3][kDepthBlock / 64], s_hi[3][kDepthBlock / 64], s_cnt[kDepthBlock / 64];
  const int wave = threadIdx.x >> 6;
  if (with_box) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      uint32_t l = klo[d], h = khi[d];
      for (int off = 32; off >= 1; off >>= 1) {
        l = min(l, (uint32_t)__shfl_xor((int)l, off, 64));
        h = max(h, (uint32_t)__shfl_xor((int)h, off, 64));
      }
      if ((threadIdx.x & 63u) == 0) { s_lo[d][wave] = l; s_hi[d][wave] = h; }
    }
  }
  if ((threadIdx.x & 63u) == 0) s_cnt[wave] = wave_count;
  __syncthreads();
  if (threadIdx.x < 3 && with_box) {
    const int d = threadIdx.x;
    uint32_t l = s_lo[d][0], h = s_hi[d][0];
    for (int w = 1; w < kDepthBlock / 64; ++w) { l = min(l, s_lo[d][w]); h = max(h, s_hi[d][w]); }
    if (l <= h) { atomicMin(res + lo_word + d, l); atomicMax(res + hi_word + d, h); }
  } else if (threadIdx.x == 3) {
    uint32_t c = 0;
    for (int w = 0; w < kDepthBlock / 64; ++w) c += s_cnt[w];
    if (c) atomicAdd(res + count_word, c);
  }
}

// SCATTER = false: seg_count[col * row_tiles + row_tile] = survivors of that segment (and the valid pixels' count and, for a
// cropped call, their box: the Morton box of the uncropped cloud).  SCATTER = true: the points, their pixel indices, the kept
// points' box.
// RGB (scatter pass of ope_depth_to_cloud_rgb): the tile's 64 x 64 BGR pixels, 192 bytes per tile row, come in as 16-byte loads (12
// lanes read one tile row) and lie in LDS at an odd pitch of words; a wave reads the three bytes of (row = lane, one column) as the
// two words they can span, 64 different banks each, and shifts them out (the column, so the shift, is the same for the wave).
// rgb[o] = r << 16 | g << 8 | b beside the point (datagrabber.cpp:48-51: bytes 0, 1, 2 are b, g, r).
template <bool SCATTER, bool RGB>
__global__ __launch_bounds__(kDepthBlock) void depth_tile_kernel(DepthJob job, uint32_t *__restrict__ seg_count, const uint32_t *__restrict__ seg_off,
                                                                 float *__restrict__ raw, int32_t *__restrict__ pix, uint32_t *__restrict__ rgb,
                                                                 uint32_t *__restrict__ res) {
  static_assert(SCATTER || !RGB, "colours are written with the points");
  __shared__ uint32_t s_tile[kTile][kTilePitch];
  __shared__ uint32_t s_bgr[RGB ? kTile : 1][kBgrPitch];
  const uint32_t tr = blockIdx.x / job.col_tiles, tc = blockIdx.x - tr * job.col_tiles;
  {
    const uint32_t k = threadIdx.x & 15u, r0 = threadIdx.x >> 4;
#pragma unroll
    for (int step = 0; step < kTile / 16; ++step) {
      const uint32_t r = r0 + 16u * step, grow = tr * kTile + r;
      uint2 v = make_uint2(0u, 0u);   // rows past the image: depth 0, dropped
      if (grow < job.rows) v = *reinterpret_cast<const uint2 *>(job.img + (size_t)grow * job.row_bytes + (size_t)tc * (2 * kTile) + 8u * k);
      s_tile[r][2 * k] = v.x;
      s_tile[r][2 * k + 1] = v.y;
    }
  }
  if (RGB) {
    constexpr uint32_t kVecPerRow = 3 * kTile / 16;   // 12 loads of 16 bytes per tile row
    for (uint32_t i = threadIdx.x; i < kTile * kVecPerRow; i += kDepthBlock) {
      const uint32_t r = i / kVecPerRow, k = i - r * kVecPerRow, grow = tr * kTile + r;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);   // rows past the image: never read back (their depth is 0)
      if (grow < job.rows)
        v = *reinterpret_cast<const uint4 *>(job.img + (size_t)grow * job.row_bytes + job.bgr_off + (size_t)tc * (3 * kTile) + 16u * k);
      s_bgr[r][4 * k] = v.x; s_bgr[r][4 * k + 1] = v.y; s_bgr[r][4 * k + 2] = v.z; s_bgr[r][4 * k + 3] = v.w;
    }
    if (threadIdx.x < kTile) s_bgr[threadIdx.x][kBgrPitch - 1] = 0u;   // the pad word: read as the upper word of the last column, shifted out
  }
  if (!SCATTER && blockIdx.x == 0 && threadIdx.x == 0) seg_count[(size_t)job.cols * job.row_tiles] = 0u;   // the scan's last slot
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t row = tr * kTile + lane;
  const float row_off = __fsub_rn((float)row, job.c_row);
  const bool with_box = SCATTER || job.crop;
  uint32_t klo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, khi[3] = {0u, 0u, 0u};
  uint32_t wave_count = 0;
  for (int j = 0; j < kColsPerWave; ++j) {
    const uint32_t c_local = wave * kColsPerWave + j, col = tc * kTile + c_local;
    if (col >= job.cols) break;   // (the same for every lane of the wave)
    const uint32_t word = s_tile[lane][c_local >> 1];
    const uint32_t d = (c_local & 1u) ? (word >> 16) : (word & 0xffffu);
    // datagrabber.cpp:169-171, every operation rounded once
    const float z = __fdiv_rn((float)d, job.scale);
    const float y = __fdiv_rn(__fmul_rn(row_off, z), job.f_row);
    const float x = __fdiv_rn(__fmul_rn(__fsub_rn((float)col, job.c_col), z), job.f_col);
    const bool valid = d != 0u && !((double)z > job.z_max);
    const bool fin = isfinite(x) && isfinite(y) && isfinite(z);
    // passthrough.hpp: "if (value > max || value < min) -> removed"; a non-finite point never passes
    const bool keep = valid && (!job.crop || (fin && !(x > job.hi[0] || x < job.lo[0]) && !(y > job.hi[1] || y < job.lo[1]) &&
                                              !(z > job.hi[2] || z < job.lo[2])));
    const unsigned long long m = __ballot(keep);
    const uint32_t seg = col * job.row_tiles + tr;
    if (!SCATTER) {
      if (lane == 0) seg_count[seg] = (uint32_t)__popcll(m);
      wave_count += (uint32_t)__popcll(__ballot(valid));
      if (job.crop && valid && fin) {
        const float v[3] = {x, y, z};
#pragma unroll
        for (int a = 0; a < 3; ++a) { const uint32_t key = ordered_key(v[a]); klo[a] = min(klo[a], key); khi[a] = max(khi[a], key); }
      }
    } else {
      wave_count += (uint32_t)__popcll(__ballot(keep && fin));
      if (keep) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const size_t o = (size_t)seg_off[seg] + rank;
        raw[3 * o] = x; raw[3 * o + 1] = y; raw[3 * o + 2] = z;
        pix[o] = (int32_t)(row * job.cols + col);
        if (RGB) {
          const uint32_t byte = 3u * c_local, w = byte >> 2;
          const unsigned long long two = ((unsigned long long)s_bgr[lane][w + 1] << 32) | s_bgr[lane][w];
          rgb[o] = (uint32_t)(two >> (8u * (byte & 3u))) & 0x00ffffffu;
        }
        if (fin) {
          const float v[3] = {x, y, z};
#pragma unroll
          for (int a = 0; a < 3; ++a) { const uint32_t key = ordered_key(v[a]); klo[a] = min(klo[a], key); khi[a] = max(khi[a], key); }
        }
      }
    }
  }
  if (SCATTER) block_commit(klo, khi, wave_count, with_box, res, kKeptLo, kKeptHi, kKeptFinite);
  else block_commit(klo, khi, wave_count, with_box, res, kValidLo, kValidHi, kValidCount);
}

float unkey(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

}  // namespace
}  // namespace ope

using namespace ope;

extern "C" int ope_depth_sensor_params(int sensor, ope_depth_params *p) {
  if (!p) return OPE_EINVAL;
  float fx, fy, cx, cy;
  switch (sensor) {   // datagrabber.cpp:133-136, :146-149, :159-162
    case OPE_SENSOR_EUCLID: fx = 306.178f; fy = 306.929f; cx = 158.523f; cy = 122.747f; break;
    case OPE_SENSOR_KINECT: fx = 525.0f; fy = 525.0f; cx = 319.5f; cy = 239.5f; break;
    case OPE_SENSOR_ASTRA: fx = 570.342f; fy = 570.342f; cx = 314.5f; cy = 235.5f; break;
    default: return OPE_EINVAL;
  }
  // the row is depthToMeter's p_FeatX (:86,170), the column its p_FeatY (:171)
  p->f_row = fx; p->c_row = cx;
  p->f_col = fy; p->c_col = cy;
  p->scale = 1000.0f;
  p->z_max = 2.0;
  return OPE_OK;
}

extern "C" int ope_depth_last_stats(const ope_ctx *ctx, ope_depth_stats *out) {
  if (!ctx || !out) return OPE_EINVAL;
  *out = ctx->depth_stats;
  return OPE_OK;
}

// ope_depth_to_cloud (bgr == nullptr) and ope_depth_to_cloud_rgb: one path.  A coloured frame differs in the bytes of a staged row
// (2 + 3 per padded pixel instead of 2), in the scatter pass's instantiation and in the colour stream of the Morton gather.
static int depth_to_cloud_impl(ope_ctx *ctx, const char *fn, const uint16_t *depth, size_t rows, size_t cols, size_t row_stride_bytes,
                               const unsigned char *bgr, size_t bgr_stride_bytes, const ope_depth_params *params, const float lo[3],
                               const float hi[3], ope_cloud **out, int32_t *out_pixel, size_t *n_out) {
  const std::string who = std::string(fn) + ": ";
  // (a NULL ctx is refused last: every other case is then told apart by its message without a context, ope_last_error(NULL))
  if (!depth || !params || !out) return set_err(ctx, OPE_EINVAL, who + "bad argument");
  if (rows == 0 || cols == 0 || rows > (size_t)0x7fffffff || cols > (size_t)0x7fffffff || rows * cols > (size_t)0x7fffffff)
    return set_err(ctx, OPE_EINVAL, who + "rows * cols must be 1 .. 2^31 - 1");
  if (row_stride_bytes < 2 * cols || (row_stride_bytes & 1u)) return set_err(ctx, OPE_EINVAL, who + "row_stride_bytes must be even and >= 2 * cols");
  if (!positive_finite(params->scale) || !positive_finite(params->f_row) || !positive_finite(params->f_col))
    return set_err(ctx, OPE_EINVAL, who + "scale, f_row and f_col must be positive and finite");
  if (!std::isfinite(params->c_row) || !std::isfinite(params->c_col))   // (no point would be finite: n_valid < n)
    return set_err(ctx, OPE_EINVAL, who + "c_row and c_col must be finite");
  const size_t px_bytes = bgr ? 5 : 2;   // of a staged pixel: the depth sample and, for a coloured frame, its three colour bytes
  if (px_bytes * ((cols + kTile - 1) / kTile * kTile) > kStageChunk) return set_err(ctx, OPE_EINVAL, who + "one padded image row must fit the 32 MB staging block");
  if ((lo == nullptr) != (hi == nullptr)) return set_err(ctx, OPE_EINVAL, who + "give both lo and hi, or neither");
  if (!ctx) return set_err(ctx, OPE_EINVAL, who + "bad argument: ctx is NULL");
  *out = nullptr;
  if (n_out) *n_out = 0;
  OPE_HIP(ctx, hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  ope_depth_stats &S = ctx->depth_stats;
  S = ope_depth_stats{};
  S.pixels = (int64_t)(rows * cols);

  DepthJob job{};
  job.rows = (uint32_t)rows;
  job.cols = (uint32_t)cols;
  job.col_tiles = (uint32_t)((cols + kTile - 1) / kTile);
  job.row_tiles = (uint32_t)((rows + kTile - 1) / kTile);
  job.pitch = job.col_tiles * kTile;
  job.f_row = params->f_row; job.c_row = params->c_row;
  job.f_col = params->f_col; job.c_col = params->c_col;
  job.scale = params->scale;
  job.z_max = params->z_max;
  job.crop = lo != nullptr;
  for (int d = 0; d < 3; ++d) { job.lo[d] = lo ? lo[d] : 0.f; job.hi[d] = hi ? hi[d] : 0.f; }
  const size_t n_pix = rows * cols, n_seg = cols * (size_t)job.row_tiles, row_bytes = px_bytes * (size_t)job.pitch;
  job.row_bytes = (uint32_t)row_bytes;
  job.bgr_off = 2 * job.pitch;
  const unsigned n_tiles = job.row_tiles * job.col_tiles;

  unsigned char *d_img = nullptr;
  uint32_t *d_cnt = nullptr, *d_off = nullptr, *d_res = nullptr, *d_rgb_raw = nullptr;
  float *d_raw = nullptr;
  int32_t *d_pix = nullptr, *d_perm = nullptr;
  void *d_tmp = nullptr;
  size_t tb = 0;
  ope_cloud *c = nullptr;
  uint32_t res[kResultWords], total = 0;
  hipError_t e = tmp_malloc(st, (void **)&d_img, row_bytes * rows);
  if (e == hipSuccess) e = tmp_malloc(st, (void **)&d_cnt, 4 * (n_seg + 1));
  if (e == hipSuccess) e = tmp_malloc(st, (void **)&d_off, 4 * (n_seg + 1));
  if (e == hipSuccess) e = tmp_malloc(st, (void **)&d_res, sizeof res);
  if (e == hipSuccess) e = tmp_malloc(st, (void **)&d_raw, 12 * n_pix);
  if (e == hipSuccess) e = tmp_malloc(st, (void **)&d_pix, 4 * n_pix);
  if (e == hipSuccess && bgr) e = tmp_malloc(st, (void **)&d_rgb_raw, 4 * n_pix);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb, d_cnt, d_off, 0u, n_seg + 1, rocprim::plus<uint32_t>(), st);
  if (e == hipSuccess) e = tmp_malloc(st, &d_tmp, std::max<size_t>(tb, 16));
  // the image, 2 bytes per pixel: its rows packed at the device pitch into the pinned block, one copy (images of more than the
  // block's 32 MB: one copy and one synchronisation per block, the block is refilled next).  A coloured frame travels the same
  // way at 5 bytes per pixel: every staged row is the depth row followed by its colour row, so the two images share the
  // block, the copy and, above 32 MB, the blocks (6.7 M pixels per block instead of 16.7 M).
  {
    unsigned char *blk = nullptr;
    size_t cap = 0;
    if (e == hipSuccess) e = stage_block(row_bytes * rows, &blk, &cap);
    if (e == hipSuccess && cap < row_bytes) e = hipErrorInvalidValue;   // (cannot happen: refused above)
    const size_t rows_per_block = e == hipSuccess ? cap / row_bytes : 1;
    for (size_t r0 = 0; e == hipSuccess && r0 < rows; r0 += rows_per_block) {
      const size_t cnt = std::min(rows_per_block, rows - r0);
      if (r0) { e = hipStreamSynchronize(st); ++S.host_syncs; }
      for (size_t r = 0; e == hipSuccess && r < cnt; ++r)
        std::memcpy(blk + r * row_bytes, reinterpret_cast<const unsigned char *>(depth) + (r0 + r) * row_stride_bytes, 2 * cols);
      for (size_t r = 0; bgr && e == hipSuccess && r < cnt; ++r)
        std::memcpy(blk + r * row_bytes + job.bgr_off, bgr + (r0 + r) * bgr_stride_bytes, 3 * cols);
      if (e == hipSuccess) e = hipMemcpyAsync(d_img + r0 * row_bytes, blk, cnt * row_bytes, hipMemcpyHostToDevice, st);
      ++S.launches;
    }
  }
  if (e == hipSuccess) {
    for (int w = 0; w < kResultWords; ++w) res[w] = 0u;
    for (int d = 0; d < 3; ++d) res[kValidLo + d] = res[kKeptLo + d] = 0xffffffffu;
    e = h2d_copy(st, d_res, res, sizeof res);
    ++S.launches;
  }
  if (e == hipSuccess) {
    job.img = d_img;
    hipLaunchKernelGGL((depth_tile_kernel<false, false>), dim3(n_tiles), dim3(kDepthBlock), 0, st, job, d_cnt, (const uint32_t *)nullptr, (float *)nullptr,
                       (int32_t *)nullptr, (uint32_t *)nullptr, d_res);
    e = hipGetLastError();
    size_t t1 = std::max<size_t>(tb, 16);
    if (e == hipSuccess) e = rocprim::exclusive_scan(d_tmp, t1, d_cnt, d_off, 0u, n_seg + 1, rocprim::plus<uint32_t>(), st);
    S.launches += 2;
  }
  if (e == hipSuccess) {
    if (bgr)
      hipLaunchKernelGGL((depth_tile_kernel<true, true>), dim3(n_tiles), dim3(kDepthBlock), 0, st, job, (uint32_t *)nullptr, d_off, d_raw, d_pix, d_rgb_raw, d_res);
    else
      hipLaunchKernelGGL((depth_tile_kernel<true, false>), dim3(n_tiles), dim3(kDepthBlock), 0, st, job, (uint32_t *)nullptr, d_off, d_raw, d_pix,
                         (uint32_t *)nullptr, d_res);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d_off + n_seg, 4, hipMemcpyDeviceToHost, st);
    S.launches += 3;
  }
  if (e == hipSuccess || S.launches) {   // (also after a failure: no copy into this frame may be left in flight)
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    ++S.host_syncs;
  }
  if (e == hipSuccess) {
    S.valid = res[kValidCount];
    S.kept = total;
    c = new ope_cloud();
    c->ctx = ctx;
    c->n = total;
    c->n_valid = res[kKeptFinite];
    c->host_valid = false;
    e = hipMalloc((void **)&c->d_xyzw, sizeof(float4) * std::max<size_t>(total, 1));
    if (e == hipSuccess && bgr) e = hipMalloc((void **)&c->d_rgb, 4 * std::max<size_t>(total, 1));   // (an empty cloud has colours too)
  }
  if (e == hipSuccess) {
    if (c->n_valid > 0)
      for (int d = 0; d < 3; ++d) { c->bb_lo[d] = unkey(res[kKeptLo + d]); c->bb_hi[d] = unkey(res[kKeptHi + d]); }
    // The Morton box: the cloud's own, as ope_cloud_upload takes it; for a cropped call the UNCROPPED cloud's, because
    // ope_pass_through_cloud leaves its survivors in the order they had along the parent's curve (compact_cloud_device)
    // and the order of a cropped call is that one.
    float mlo[3] = {0.f, 0.f, 0.f}, mhi[3] = {0.f, 0.f, 0.f}, inv[3];
    const int lw = job.crop ? kValidLo : kKeptLo, hw = job.crop ? kValidHi : kKeptHi;
    if (res[lw] <= res[hw])
      for (int d = 0; d < 3; ++d) { mlo[d] = unkey(res[lw + d]); mhi[d] = unkey(res[hw + d]); }
    for (int d = 0; d < 3; ++d) inv[d] = (mhi[d] > mlo[d]) ? 1023.999f / (mhi[d] - mlo[d]) : 0.f;
    if (total) e = tmp_malloc(st, (void **)&d_perm, 4 * (size_t)total);
    if (e == hipSuccess && total && out_pixel) e = hipMemcpyAsync(out_pixel, d_pix, 4 * (size_t)total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && total) e = morton_order_device(st, d_raw, total, mlo, inv, c->d_xyzw, d_perm, d_rgb_raw, c->d_rgb);   // (synchronises)
    else if (total) (void)hipStreamSynchronize(st);
    S.launches += kMortonLaunches + (out_pixel ? 1 : 0);
    S.host_syncs += kMortonSyncs;
  }
  for (void *p : {(void *)d_img, (void *)d_cnt, (void *)d_off, (void *)d_res, (void *)d_raw, (void *)d_pix, (void *)d_perm, (void *)d_rgb_raw, d_tmp}) tmp_free(st, p);
  if (e != hipSuccess) {
    if (c) ope_cloud_free(c);
    return set_err(ctx, OPE_EHIP, who + hipGetErrorString(e));
  }
  *out = c;
  if (n_out) *n_out = total;
  return OPE_OK;
}

extern "C" int ope_depth_to_cloud(ope_ctx *ctx, const uint16_t *depth, size_t rows, size_t cols, size_t row_stride_bytes,
                                  const ope_depth_params *params, const float lo[3], const float hi[3], ope_cloud **out, int32_t *out_pixel,
                                  size_t *n_out) {
  return depth_to_cloud_impl(ctx, "ope_depth_to_cloud", depth, rows, cols, row_stride_bytes, nullptr, 0, params, lo, hi, out, out_pixel, n_out);
}

extern "C" int ope_depth_to_cloud_rgb(ope_ctx *ctx, const uint16_t *depth, size_t rows, size_t cols, size_t depth_stride_bytes,
                                      const unsigned char *bgr, size_t bgr_stride_bytes, const ope_depth_params *params, const float lo[3],
                                      const float hi[3], ope_cloud **out, int32_t *out_pixel, size_t *n_out) {
  // the colour image's own cases first: they need no context (the message goes where ope_last_error(NULL) finds it)
  if (!bgr) return set_err(ctx, OPE_EINVAL, "ope_depth_to_cloud_rgb: bgr is NULL");
  if (cols <= (size_t)0x7fffffff && bgr_stride_bytes < 3 * cols) return set_err(ctx, OPE_EINVAL, "ope_depth_to_cloud_rgb: bgr_stride_bytes must be >= 3 * cols");
  return depth_to_cloud_impl(ctx, "ope_depth_to_cloud_rgb", depth, rows, cols, depth_stride_bytes, bgr, bgr_stride_bytes, params, lo, hi, out, out_pixel,
                             n_out);
}
