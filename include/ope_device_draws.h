/* ope_device_draws.h - the draws of the batched prerejective aligner made on the device (prerejective_draws.hip).
 * Part of the C ABI of ope.h, which includes this file after its own declarations: include ope.h, not this file alone.
 *
 * ope_prerejective_pose_batch and ope_final_pose_batch_prerejective draw, per active cluster, max_iterations iterations of
 * ope_prerejective's LCG stream on the host (nr_samples distinct indices, redrawn while they repeat, then nr_samples picks).  The
 * entry points below produce the same draws, entry for entry, on the device: the stream is cut into tiles of T positions, every
 * position computes the length of the iteration that would start there, the tiles' exit tables are composed in order, and every
 * iteration that really starts is emitted from its own position by a jump of the LCG.  An iteration longer than the window W, or a
 * problem that does not finish max_iterations iterations inside its stream budget P, is drawn by the host loop instead (the
 * outputs are the same; only the statistics tell). */
#ifndef OPE_DEVICE_DRAWS_H
#define OPE_DEVICE_DRAWS_H
#ifndef OPE_H
#error "include ope.h: it declares the types these entry points take and includes this header itself"
#endif

enum {
  OPE_DRAWS_HOST = 0,   /* the default: the host loop and one packed upload */
  OPE_DRAWS_DEVICE = 1
};

/* Where ope_prerejective_pose_batch and ope_final_pose_batch_prerejective make their draws from now on (context state, like the
 * list of global rejectors).  With OPE_DRAWS_DEVICE their step (b) is one small seed upload and three launches that write the packed
 * draws in place; a call then enqueues 12 launches instead of 9, still a constant that depends on neither clusters, iterations,
 * survivors nor points, and keeps its 3 host synchronisations.  A problem that falls back costs the call one upload and one synchronisation
 * of its own, and the call a second prerejection (4 launches, 1 synchronisation), all counted in ope_prerejective_batch_last_stats; a
 * call whose tile tables would exceed 256 MiB draws on the host as with OPE_DRAWS_HOST.  Results, statuses, seeds and the kept
 * hypotheses are byte for byte those of OPE_DRAWS_HOST.
 * The single ope_prerejective ignores the mode: its host needs the samples before the feature search, so device draws would add a
 * round trip.  ope_track_pose, the SAC-IA and the correspondence batches draw differently and are not affected.
 * OPE_EINVAL: a mode other than the two. */
int ope_prerejective_set_draws(ope_ctx *ctx, int mode);
int ope_prerejective_get_draws(const ope_ctx *ctx, int *mode);
/* The window W and the stream budget P the two batched calls draw with under OPE_DRAWS_DEVICE (context state; 0 = the defaults of
 * ope_prerejective_draws_device below).  Smaller values only send more problems back to the host loop, never change a result: this is
 * how the batch's fallback path is reached on purpose.  OPE_EINVAL: a non-zero window outside 6 .. 1024, a negative budget; a batched
 * call in device mode refuses a window below 2 * nr_samples. */
int ope_prerejective_set_draws_limits(ope_ctx *ctx, int window, int64_t budget);

/* The draws alone, for n problems that share ns (source key points), S (nr_samples), K (k_correspondences) and H (max_iterations)
 * and differ in their seed: samples / picks (n * H * S each, problem-major, then iteration-major) are what ope_prerejective draws
 * for that seed.  window / budget: 0 selects the defaults (W = 256 positions per iteration; P = ceil(H (2 S + E) + 8 sqrt(H V) + W)
 * stream positions, E and V the mean and the variance of an iteration's redraws); other values override W and P.  Problems the
 * device could not finish inside W or P are drawn on the host; stats (8 values, may be NULL) is what
 * ope_prerejective_draws_last_stats reports afterwards.  One synchronisation.  n = 0 does nothing.
 * OPE_EINVAL, nothing launched: H outside 1 .. 2^20, S outside 3 .. 8, K outside 1 .. 8, ns outside S .. 4096 (a draw is packed in
 * 12 + 3 bits), a non-zero window outside 2 S .. 1024, a negative budget, n * H above 2^31 - 1, a NULL seeds / samples / picks, a
 * context with a communicator. */
int ope_prerejective_draws_device(ope_ctx *ctx, int ns, int S, int K, int H, const uint64_t *seeds, size_t n, int window, int64_t budget,
                                  int32_t *samples, int32_t *picks, int64_t *stats);

/* The draw stage of the last ope_prerejective_draws_device, ope_prerejective_pose_batch or ope_final_pose_batch_prerejective on
 * the context: [0] the mode used (OPE_DRAWS_*), [1] problems drawn on the device, [2] problems that fell back because an iteration
 * outgrew the window, [3] problems that fell back because the budget ended first, [4] 1 if the whole call drew on the host because
 * of its size, [5] stream positions per problem P, [6] tile size T, [7] launches of the draw stage (the seed upload and the three
 * kernels; 0 on the host). */
int ope_prerejective_draws_last_stats(const ope_ctx *ctx, int64_t out[8]);

#endif /* OPE_DEVICE_DRAWS_H */
