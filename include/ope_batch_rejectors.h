/* ope_batch_rejectors.h - the batched ICP entry points that take a list of global correspondence rejectors as an argument
 * (icp_batch.hip: the staged instantiations; final_batch.hip).  Part of the C ABI of ope.h, which includes this file after its own
 * declarations: include ope.h, not this file alone.  The rules of the three rejectors, ope_global_rejector and
 * ope_global_rejector_stats are stated in ope.h ("Global correspondence rejectors"). */
#ifndef OPE_BATCH_REJECTORS_H
#define OPE_BATCH_REJECTORS_H
#ifndef OPE_H
#error "include ope.h: it declares the types these entry points take and includes this header itself"
#endif

/* ope_icp_run_batch with a list of global rejectors applied inside every problem's workgroup (icp_batch.hip, the staged
 * instantiations): per iteration the search pass with its fused pointwise rejectors stores the pairs, the list runs over them in
 * order by the rules of ope.h (median: an exact selection over the fp32 bit patterns; one to one: 64-bit integer minima per target
 * point; var trimmed: a sort of the keys), and a second pass adds the survivors' 17 sums for the same update step.  No kernel
 * boundary, no floating-point atomics, nothing that depends on scheduling: every output of a problem is bit-reproducible and
 * independent of the rest of the batch.  With an empty list the staged kernel returns what ope_icp_run_batch returns, byte for byte.
 *   stats (n * n_list, problem-major; may be NULL): rejector k of problem i as the last iteration that searched applied it;
 *       launches = 0 (the stage dispatches nothing of its own).
 *   index_match / distance (sum of src[i]->n entries each, problem i's from the sum of the earlier src[j]->n, addressed by
 *       ORIGINAL source index; each may be NULL): the ORIGINAL target index and the distance field of the pair that survived the
 *       last iteration that searched, or -1 and 0.
 * n_list = 0 and no pair output: ope_icp_run_batch itself.  n_list = 0 with a pair output: the staged kernel with an empty list.
 * OPE_EINVAL, nothing launched: everything ope_icp_run_batch refuses (a list set on the CONTEXT included); with a list or a pair
 * output also an estimator other than OPE_EST_SVD, reciprocal correspondences, more than OPE_GREJ_MAX rejectors, a rejector
 * parameter out of range.  The source limit is ope_icp_run_batch's (65536 valid points): up to 8192 valid source points the
 * var-trimmed keys sort in LDS, and up to 5376 target points the one-to-one words live there; larger problems use their slice of
 * the call's temporary block. */
int ope_icp_run_batch_rejectors(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                                const ope_icp_params *params, const ope_global_rejector *list, size_t n_list, double fitness_max_range,
                                ope_icp_batch_result *out, ope_global_rejector_stats *stats, int32_t *index_match, float *distance);

/* ope_final_pose_batch (SAC-IA coarse stage) whose fine ICP runs the list of global rejectors: ope_icp_run_batch_rejectors on the
 * same fine inputs (ope_final_batch_inputs reports them).  n_list = 0 is ope_final_pose_batch.  Refusals: ope_final_pose_batch's
 * and the list's (ope_icp_run_batch_rejectors); params->icp.estimator must be OPE_EST_SVD.  The prerejective and correspondences
 * variants and ope_track_pose take no list. */
int ope_final_pose_batch_rejectors(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                   const ope_final_params *params, const ope_global_rejector *list, size_t n_list, const uint64_t *seeds,
                                   ope_final_batch_result *out, int32_t *selected);

#endif /* OPE_BATCH_REJECTORS_H */
