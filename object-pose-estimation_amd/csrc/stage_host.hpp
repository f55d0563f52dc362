// stage_host.hpp — the host-side plumbing the stage files share (coarse aligners, segmentation, filters): the launch grid, the timed
// and counted launch, the identity, the communicator refusal, the staged upload and the two-phase select.  Host code only.
#pragma once

#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

#include "ope_internal.hpp"

namespace ope {

// blocks of `block` threads over n items, at least one
inline unsigned grid_of(size_t n, int block) { return (unsigned)std::max<size_t>((n + block - 1) / block, 1); }

constexpr float kIdentity4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // column-major 4x4

// One kernel launch under a KernelTimer (label, algorithmic bytes); the arguments after `bytes` are hipLaunchKernelGGL's after the
// kernel.  STAGE_LAUNCH_AS adds one to `counter` (the entry point's launch statistic) and takes the label, STAGE_LAUNCH labels the
// launch with the kernel's name, STAGE_LAUNCH_TIMED counts nothing.
#define STAGE_LAUNCH_TIMED(ctx, name, label, bytes, ...) \
  do {                                                   \
    KernelTimer kt_((ctx), label, (double)(bytes));      \
    hipLaunchKernelGGL(name, __VA_ARGS__);               \
  } while (0)
#define STAGE_LAUNCH_AS(ctx, counter, name, label, bytes, ...)     \
  do {                                                             \
    STAGE_LAUNCH_TIMED(ctx, name, label, bytes, __VA_ARGS__);      \
    ++(counter);                                                   \
  } while (0)
#define STAGE_LAUNCH(ctx, counter, name, bytes, ...) STAGE_LAUNCH_AS(ctx, counter, name, #name, bytes, __VA_ARGS__)
// One library call that enqueues launches (a rocPRIM primitive), timed and counted the same way, skipped once `e` holds an error.
#define STAGE_PRIM(ctx, counter, e, label, call) \
  do {                                           \
    if ((e) == hipSuccess) {                     \
      KernelTimer kt_((ctx), label, 0.0);        \
      (e) = (call);                              \
      ++(counter);                               \
    }                                            \
  } while (0)

// the aligners run on one device: OPE_OK, or the refusal of a context that carries a communicator
inline int refuse_communicator(ope_ctx *ctx, const char *who) {
  if (ctx->nccl_comm != nullptr || ctx->p2p_ok || ctx->p2p_broken)
    return set_err(ctx, OPE_EINVAL, std::string(who) + "the context carries a communicator (one device runs a whole alignment)");
  return OPE_OK;
}

// Host ranges back to back into one device block in stream order.  Up to the size of the pinned staging block this is one copy
// that does not synchronise (the caller synchronises before it stages again); beyond it, one h2d_copy per range, whose synchronising
// pieces are added to *syncs.  *copies grows by the copies made: one, or one per range.
struct HostRange { const void *p; size_t bytes; };
inline hipError_t upload_staged(hipStream_t stream, void *dst, const HostRange *parts, int n_parts, int64_t *copies, int64_t *syncs) {
  size_t total = 0;
  for (int i = 0; i < n_parts; ++i) total += parts[i].bytes;
  unsigned char *blk = nullptr;
  size_t cap = 0;
  hipError_t e = stage_block(total, &blk, &cap);
  if (e != hipSuccess) return e;
  size_t off = 0;
  if (total > cap) {
    for (int i = 0; i < n_parts && e == hipSuccess; off += parts[i++].bytes) {
      ++*copies;
      e = h2d_copy(stream, static_cast<unsigned char *>(dst) + off, parts[i].p, parts[i].bytes, syncs);
    }
    return e;
  }
  for (int i = 0; i < n_parts; off += parts[i++].bytes) std::memcpy(blk + off, parts[i].p, parts[i].bytes);
  ++*copies;
  return hipMemcpyAsync(dst, blk, total, hipMemcpyHostToDevice, stream);
}
inline hipError_t upload_staged(hipStream_t stream, void *dst, const void *src, size_t bytes, int64_t *copies, int64_t *syncs) {
  const HostRange all{src, bytes};
  return upload_staged(stream, dst, &all, 1, copies, syncs);
}

// The positions of the set flags among n, in order, and their number: rocprim::select over a counting iterator of the output's
// type.  select_flagged_bytes is the size query (no launch); select_flagged runs it in d_tmp under a KernelTimer and counts one launch.
template <class Index>
hipError_t select_flagged_bytes(hipStream_t stream, uint8_t *d_flags, Index *d_out, uint32_t *d_count, size_t n, size_t *tmp_bytes) {
  return rocprim::select(nullptr, *tmp_bytes, rocprim::counting_iterator<Index>(0), d_flags, d_out, d_count, n, stream);
}
template <class Index>
hipError_t select_flagged(ope_ctx *ctx, const char *label, double bytes, int64_t *launches, void *d_tmp, size_t tmp_bytes, uint8_t *d_flags,
                          Index *d_out, uint32_t *d_count, size_t n) {
  KernelTimer kt(ctx, label, bytes);
  ++*launches;
  return rocprim::select(d_tmp, tmp_bytes, rocprim::counting_iterator<Index>(0), d_flags, d_out, d_count, n, ctx->stream);
}

}  // namespace ope
