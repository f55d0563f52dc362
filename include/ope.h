/*
 * ope.h — C ABI of libope_hip.so, the MI355X-native (gfx950) replacement for the
 * registration hot path of gopi-erabati/Object-Pose-Estimation (DetectAndLocalize).
 *
 * The reference has no FFI of its own: its operator API is the PCL class-template
 * protocol.  Each entry point below names the reference call it replaces
 * (paths relative to the reference root; vPCL = the vendored include/pcl/registration/ headers).
 * The C++ façade include/ope/pcl_compat.hpp re-creates those PCL call shapes on
 * top of this ABI; INTEGRATION.md shows the re-pointing of poseestimator.cpp.
 *
 * Conventions
 *  - every function returns OPE_OK (0) or a negative OPE_E* code; no exceptions
 *    cross the ABI; ope_last_error(ctx) gives the message of the last failure.
 *  - 4x4 transforms are COLUMN-MAJOR float[16] (Eigen::Matrix4f memory layout,
 *    translation in [12..14]; reference: rosinterface.cpp:435-437).
 *  - host buffers are only read/written during the call; device copies are owned
 *    by the ope_cloud / ope_index handles.  Handles are not thread-safe; calls on
 *    one ope_ctx must be externally serialised (reference: one PoseEstimator per
 *    process, rosinterface.h:54).
 *  - this library is GPU-only.  There is no CPU fallback: ope_ctx_create fails
 *    with OPE_ENODEV when no HIP device is present.
 */
#ifndef OPE_H
#define OPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPE_ABI_VERSION 5

enum {
  OPE_OK = 0,
  OPE_EINVAL = -1,  /* bad argument (NULL handle, n == 0 where forbidden, …) */
  OPE_ENODEV = -2,  /* no HIP device / bad ordinal */
  OPE_EHIP = -3,    /* a HIP runtime call failed */
  OPE_ENOMEM = -4,
  OPE_ESTATE = -5,  /* call out of sequence (e.g. ope_icp_step without begin) */
  OPE_ECOMM = -6,   /* RCCL failure */
  OPE_EEMPTY = -7,  /* empty target cloud (registration_mod.hpp:60-64) */
  OPE_ERANGE = -8   /* voxel index would overflow 32 bits: PCL warns "leaf size is too small" and returns its input */
};

typedef struct ope_ctx ope_ctx;
typedef struct ope_cloud ope_cloud;
typedef struct ope_index ope_index;

/* ---------------- context ---------------- */
int ope_abi_version(void);
int ope_device_count(void);
/* One context per GPU (one process per GPU in multi-GPU runs). */
int ope_ctx_create(ope_ctx **out, int device_ordinal);
void ope_ctx_destroy(ope_ctx *ctx);
/* Run on an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream. */
int ope_ctx_set_stream(ope_ctx *ctx, void *hip_stream);
int ope_ctx_sync(ope_ctx *ctx);
/* Named roctx ranges (rocprofv3 --marker-trace) around the host side of the path: icp_iter {nn, reduce}, normals,
 * fpfh_spfh, fpfh_weight, sacia, prerejective, index_build, uniform_sampling.  Off by default.  The reference's own instrumentation is
 * pcl::ScopeTime("Initial Alignment" / "Final Alignment") (poseestimator.cpp:61,349): the facade keeps those names. */
int ope_ctx_set_tracing(ope_ctx *ctx, int on);
/* Bound of every device-side wait of the overlapped update launches (ope_icp_params.update_launch), seconds, 0 .. 40; default 2.
 * A launch whose partner has not reported within the bound gives up and the run resumes in line at the next ope_icp_poll /
 * ope_icp_end (nothing is lost but the time waited; the context launches in line from then on).  Raise it for launches that
 * legitimately take longer than the bound (a source of hundreds of millions of points); a process that shares its GPU with other
 * work it cannot predict should rather ask for OPE_UPDATE_IN_LINE.  A bound of a microsecond makes every overlapped update give up at once
 * (how the test of the recovery path forces it). */
int ope_ctx_set_wait_limit(ope_ctx *ctx, double seconds);
const char *ope_last_error(const ope_ctx *ctx);

/* Measurement hook for the coarse-stage and filter kernels (normals_kernel, spfh_kernel, fpfh_kernel, feature_knn_kernel,
 * sacia_error_kernel, sor_mean_distance_kernel): while on, every launch is bracketed by HIP events on the launch stream and
 * recorded with its ALGORITHMIC bytes (normals N(12+12k+16); SPFH N(24+24m+132); FPFH N(136m+132); SAC-IA
 * 24 N_s per hypothesis; SOR N(12+12k+4)).  ope_profile_kernels_read synchronises and returns one record per kernel name,
 * summed over its launches since ope_profile_kernels(ctx, 1). */
typedef struct {
  char name[32];
  double ms;
  int launches;
  double algorithmic_bytes;
} ope_kernel_time;
int ope_profile_kernels(ope_ctx *ctx, int on);
int ope_profile_kernels_read(ope_ctx *ctx, ope_kernel_time *out, size_t cap, size_t *n_out);

/* ---------------- clouds ---------------- */
/* Upload n points from an array of structs: xyz floats at base + i*stride + xyz_off,
 * optional normal floats at normal_off (pass -1 for none).  Works directly on
 * pcl::PointXYZ (stride 16, xyz_off 0), pcl::PointXYZRGBNormal (stride 48,
 * normal_off 16) or packed float[3] (stride 12).  Replaces setInputSource /
 * setInputCloud (registration_mod.h:197-201; poseestimator.cpp:121,155,312).
 * Points are re-ordered on the device along a Morton curve (the permutation is
 * kept; all outputs are reported in ORIGINAL indices).  Non-finite points are
 * kept in the index space but never produce correspondences (icp_mod.hpp:71-72). */
int ope_cloud_upload(ope_ctx *ctx, const void *base, size_t n, size_t stride_bytes, size_t xyz_off,
                     ptrdiff_t normal_off, ope_cloud **out);
/* Attach / replace normals (n*3 packed floats, original order). */
int ope_cloud_set_normals(ope_ctx *ctx, ope_cloud *cloud, const float *normals_xyz);
/* The normals attached to a cloud (ope_cloud_set_normals, ope_normals, ope_mls_smooth_cloud with compute_normals), in ORIGINAL
 * order: out_normals n*3 floats, out_curvature n floats (the fourth component the device keeps beside a normal: 0 after
 * ope_cloud_set_normals); either may be NULL.  OPE_EINVAL when the cloud carries none. */
int ope_cloud_download_normals(ope_ctx *ctx, const ope_cloud *cloud, float *out_normals, float *out_curvature);
/* The colour payload of a cloud: one word per point, the 32 bits of pcl::PointXYZRGB::rgb (r << 16 | g << 8 | b, top byte as
 * given), kept on the device beside the points.  ope_cloud_set_rgb attaches / replaces it from n words in ORIGINAL order; NULL
 * detaches it (the cloud is then what it was before: nothing else about a cloud depends on its colours).  ope_cloud_has_rgb: 1 or
 * 0 (0 for NULL).  ope_cloud_download_rgb: the n words in ORIGINAL order; OPE_EINVAL when the cloud has no colours.
 * CARRIED: every entry point that makes a cloud from clouds hands the payload on with the points, in the launches that move the
 * points (no further launch or synchronisation): ope_cloud_select (repeats and any order), ope_cloud_concat (below), the _cloud
 * forms of the filters (ope_remove_nan_cloud, ope_pass_through_cloud, ope_statistical_outlier_removal_cloud,
 * ope_uniform_sampling_cloud: the chosen point's colour), plane / not_plane of ope_plane_segment and ope_tabletop_segment, out of
 * ope_prism_extract, the clusters of ope_euclidean_clusters_cloud, ope_mls_smooth_cloud, and ope_depth_to_cloud_rgb makes it.  An empty cloud made from a
 * coloured one has colours.  NOT carried: *aligned of ope_track_pose (the moved model; the tracker reads no colours). */
int ope_cloud_set_rgb(ope_ctx *ctx, ope_cloud *cloud, const uint32_t *rgb);
int ope_cloud_has_rgb(const ope_cloud *cloud);
int ope_cloud_download_rgb(ope_ctx *ctx, const ope_cloud *cloud, uint32_t *out);
/* pcl::transformPointCloud(a, ., T_a) followed by operator+= (BuildModel regmeshpcd.cpp:203,254: cloudTemp = aligned + target),
 * built on the device: out holds T_a * a (T_a may be NULL: identity) followed by b, ORIGINAL indices a's then b's.  Neither
 * input travels through the host; normals are not carried (re-estimated per pair in the reference, :72-90).  Colours are
 * carried when BOTH a and b have them (operator+= keeps rgb; T_a does not touch them): a's words, then b's.  With colours on
 * one side only the result has none. */
int ope_cloud_concat(ope_ctx *ctx, const ope_cloud *a, const float T_a[16], const ope_cloud *b, ope_cloud **out);
/* xyz of a cloud in ORIGINAL order (n*3 floats): the way out for clouds made by ope_cloud_concat. */
int ope_cloud_download(ope_ctx *ctx, const ope_cloud *cloud, float *out_xyz);
/* A new cloud from n ORIGINAL indices of `cloud` (host array, any order, repeats allowed), gathered on the device: the new
 * cloud's original order is the order of idx; normals and colours attached to `cloud` are carried.  What `cloud[idx]` would be after an
 * upload, without the trip through the host (the hand-over between the stages in front of the path:
 * rosinterface.cpp:212-213 -> poseestimator.cpp:141-156). */
int ope_cloud_select(ope_ctx *ctx, const ope_cloud *cloud, const int32_t *idx, size_t n, ope_cloud **out);
size_t ope_cloud_size(const ope_cloud *cloud);
void ope_cloud_free(ope_cloud *cloud);

/* ---------------- search index over a target cloud ---------------- */
typedef struct {
  int leaf_size; /* max points per leaf bucket of the OBB tree (default 16) */
  int grid;      /* 1 (default): 1-NN ICP runs also use a uniform grid over the points ("radix-bucketed" search): queries
                    whose previous match is close are answered from a few cell runs, all others by the tree.  A run whose
                    source turns out to hold more than 3 % of queries far from the target (measured on the device after
                    the first iterations) continues on the tree-only kernel, which is faster for that mix.
                    0: tree only.  2: grid kernel always. */
  float grid_fill;      /* target number of points per occupied grid cell (0 = default) */
  int grid_max_cells;   /* upper bound on the number of grid cells, 4 B each (0 = default: the table must stay L2-resident) */
} ope_index_params;
void ope_index_default_params(ope_index_params *p);
/* Replaces the kd-tree build of Registration::initCompute (registration_mod.hpp:80-84)
 * / pcl::search::KdTree::setInputCloud (poseestimator.cpp:151-152).
 * Returns OPE_EEMPTY for an empty (or all-non-finite) target. */
int ope_index_build(ope_ctx *ctx, const ope_cloud *target, const ope_index_params *params, ope_index **out);
void ope_index_free(ope_index *index);

/* Exact searches, results in ORIGINAL target indices, squared L2 distances
 * (pcl::search::KdTree::nearestKSearch / radiusSearch semantics).  `T` (optional)
 * is applied to the queries first (float math).  Host output buffers.
 *   nn:     out_idx[nq], out_d2[nq]; idx = -1, d2 = +inf for non-finite queries.
 *   knn:    out_idx[nq*k], out_d2[nq*k], ascending d2, -1/+inf padded.
 *   radius: counts[nq] always; if out_idx/out_d2 non-NULL, up to max_nn per query
 *           at stride max_nn (ascending d2). */
int ope_nn_search(ope_ctx *ctx, const ope_cloud *queries, const ope_index *index, const float *T,
                  int32_t *out_idx, float *out_d2);
int ope_knn_search(ope_ctx *ctx, const ope_cloud *queries, const ope_index *index, const float *T, int k,
                   int32_t *out_idx, float *out_d2);
int ope_radius_search(ope_ctx *ctx, const ope_cloud *queries, const ope_index *index, float radius, int max_nn,
                      int32_t *counts, int32_t *out_idx, float *out_d2);

/* ---------------- ICP ---------------- */
enum { /* DefaultConvergenceCriteria::ConvergenceState, default_convergence_criteria_mod.h:73-81 */
  OPE_CONV_NOT_CONVERGED = 0,
  OPE_CONV_ITERATIONS = 1,
  OPE_CONV_TRANSFORM = 2,
  OPE_CONV_ABS_MSE = 3,
  OPE_CONV_REL_MSE = 4,
  OPE_CONV_NO_CORRESPONDENCES = 5
};

enum { OPE_CORR_NEAREST = 0, OPE_CORR_NORMAL_SHOOTING = 1 };
/* transformation estimation: SVD/Umeyama (poseestimator.cpp:306,341), or the linearised point-to-plane
 * estimator that IterativeClosestPointWithNormals defaults to (icp_mod.h:352-357; needs TARGET normals).
 * OPE_EST_POINT_TO_PLANE_LM: pcl::registration::TransformationEstimationPointToPlane, the Levenberg-Marquardt estimator
 * BuildModel installs (regmeshpcd.cpp:162,193): same cost, minimised over (t, quaternion) with Eigen's LM logic on a
 * forward-difference Jacobian and float tolerances.  The residual is linear in the warp matrix, so one device pass per ICP
 * iteration reduces the 91 sums every functor evaluation is a quadratic form of, and the minimisation runs in the launch
 * that also updates the transform: nothing synchronises the host (ope_icp_run / ope_icp_iterate only — the step-wise
 * accumulate / update pair exchanges 17 or 44 sums, not these; needs TARGET normals). */
enum { OPE_EST_SVD = 0, OPE_EST_POINT_TO_PLANE_LLS = 1, OPE_EST_POINT_TO_PLANE_LM = 2 };
#define OPE_NUM_SUMS 17     /* {n, Σs, Σt, Σ t sᵀ, Σd²} */
#define OPE_NUM_SUMS_MAX 44 /* + upper triangle of AᵀA (21) and Aᵀb (6) for point-to-plane */

typedef struct {
  /* Registration defaults, registration_mod.h:106-118 */
  int max_iterations;               /* 10 */
  double transformation_epsilon;    /* 0 */
  double euclidean_fitness_epsilon; /* -DBL_MAX */
  double max_corr_dist;             /* sqrt(DBL_MAX) */
  int min_correspondences;          /* 3 */
  int use_reciprocal;               /* 0 */
  /* correspondence estimation: 1-NN (correspondence_estimation_mod.hpp:127-213) or
   * normal shooting over the k nearest (…normal_shooting_weighted.hpp:107-145) */
  int corr_mode;
  int k_normal_shooting; /* 20 (poseestimator.cpp:246) */
  /* rejectors, applied in this order (poseestimator.cpp:334-337) */
  int use_surface_normal_rej;  /* CorrespondenceRejectorSurfaceNormal, score correspondence_rejection_mod.h:368-376 */
  double surface_normal_thr;   /* 0.7 (poseestimator.cpp:272) */
  int use_self_occluded_rej;   /* correspondence_rejection_mod.h:382-391; opt-in, see SURVEY Q3 */
  double self_occluded_thr;    /* 0.6 (poseestimator.cpp:291) */
  /* DefaultConvergenceCriteria knobs reachable through getConvergeCriteria() */
  double mse_threshold_absolute; /* 1e-12; negative disables (fixed-length throughput runs) */
  int failure_after_max_iter;    /* 0 */
  /* host polling period for the on-device convergence flag (iterations); 0 = only at the end */
  int check_every;
  int estimator; /* OPE_EST_* */
  /* 0 (default): every block adds its partial sums into the run's sums with fp64 atomics: the addition order, and with
   * it the last bit of the sums (~1e-9 in the final transform after 100 iterations), varies from run to run.
   * 1: one row of partial sums per block and a fixed-tree reduction, the tree kernel with its chunks in natural order (no
   * cost-sorted schedule, no grid kernel: both follow measured times): bit-reproducible from run to run on one GPU model,
   * at the price of the schedule (launches that fill the GPU take longer). */
  int deterministic_sums;
  /* Which walk the OBB-tree kernel uses for the 64-query chunks of a 1-NN run.  OPE_WALK_AUTO (0, default): launches that
   * fill the GPU take one packet walk per coherent chunk and private per-lane walks for the rest, smaller launches
   * per-lane walks only.  OPE_WALK_LANE (1) / OPE_WALK_PACKET (2) force the instantiation (every walk is exact: the choice
   * moves time, and lets a test pin each kernel by name, see ope_icp_kernel_launches). */
  int tree_walk;
  /* How the per-iteration update step (Umeyama / Cholesky lane + convergence test) is launched in ope_icp_run /
   * ope_icp_iterate.  OPE_UPDATE_OVERLAPPED (0, default): on a stream of its own next to the accumulate launch it follows,
   * waiting on the device for that launch's blocks, while the next accumulate launch is already being dispatched and its
   * blocks wait for the update's word: one kernel boundary per iteration instead of two around a 64-thread launch.  Taken by
   * plain 1-NN runs of one rank (not: normal shooting, reciprocal, deterministic_sums, the LM estimator, fixed correspondences,
   * sharded runs), the others launch in line whatever this says.  Every device-side wait is bounded (2 s); a run that hits
   * the bound (the GPU's block slots held by other work, a tool that serialises dispatches) resumes in line at the next
   * ope_icp_poll / ope_icp_end with nothing lost but the time, and the context stays in line from then on; a process under a
   * counter-collecting profiler (rocprofv3 --pmc: ROCPROF_COUNTER_COLLECTION in the environment) launches in line from the start.
   * OPE_UPDATE_IN_LINE (1): accumulate -> update -> accumulate on the one stream, as in rounds 1-2 (a profiler that
   * serialises dispatches, e.g. rocprofv3 --pmc, wants this).  Same arithmetic either way. */
  int update_launch;
  /* Skip certificates of the plain 1-NN search (what CorrespondenceEstimation::determineCorrespondences,
   * impl/correspondence_estimation_mod.hpp:165-177, recomputes from scratch every iteration).  Late in a run a query's nearest
   * neighbour rarely changes, and that can be PROVEN without a search.  A certificate is the outcome of one 6-nearest walk from
   * where the query was then (q_ref): its five nearest target points and a lower bound L — the sixth's distance — on its distance
   * to every other one.  Wherever the query is later, every non-candidate is at least L - |q - q_ref| away; while the nearest of
   * the five candidates, re-measured from where the query is now, stays strictly below that (past every fp32 rounding) and
   * strictly below the other four, it is the unique nearest neighbour: same index, same d2, bit for bit, and no walk.  Every
   * launch still writes every correspondence and adds every term of the sums.
   * OPE_CERT_AUTO (0, default): launches keep certificates from the iteration on whose update moves no scene point by more than
   * 1/24 of the target's point spacing (1/512 for a run that starts on the tree kernel because more than 3 % of its queries lie
   * far outside the target: clutter, whose walks set the pace until it can hold certificates too); decided on the device, no host
   * round trip.  A query builds one when the slack it can expect — read off its previous distance — is worth 24 launches of the
   * scene's current displacement.
   * OPE_CERT_OFF (1): never.  OPE_CERT_ALWAYS (2): from the first launch (tests).  Plain 1-NN runs, tree and grid kernel
   * (not: reciprocal, normal shooting, deterministic_sums); exact in every mode — the choice moves time only. */
  int skip_certificates;
} ope_icp_params;
enum { OPE_WALK_AUTO = 0, OPE_WALK_LANE = 1, OPE_WALK_PACKET = 2 };
enum { OPE_UPDATE_OVERLAPPED = 0, OPE_UPDATE_IN_LINE = 1 };
enum { OPE_CERT_AUTO = 0, OPE_CERT_OFF = 1, OPE_CERT_ALWAYS = 2 };

typedef struct {
  int iterations;        /* nr_iterations_ */
  int converged;         /* hasConverged() */
  int state;             /* OPE_CONV_* */
  double last_mse;       /* correspondences_cur_mse_ */
  int64_t n_corr;        /* post-rejection correspondences of the last iteration */
  double align_strength; /* getAlignStrength(): n_corr / (N_src + N_tgt), icp_mod.h:249-260
                            (N_src = the full source size set with ope_icp_set_global_sizes in sharded runs) */
} ope_icp_result;

void ope_icp_default_params(ope_icp_params *p);

/* IterativeClosestPoint::setFixedCorrespondences (vPCL icp_mod.h:268; getFixedCorrespondences :276, clearCorrespondences
 * :281) — the reference's injection of given pairs into every iteration, unused by its own programs.  index_query /
 * index_match: ORIGINAL indices into `src` and into the cloud the target index was built from; n = 0 clears.  They stay set
 * for every later run over the same source cloud and a target of the same size, and take part as the reference has them:
 * 1-NN estimation lists every given pair in front of the searched ones whatever its distance, with the distance field
 * (squared distance) * 1e10 — which therefore also enters the MSE of the convergence test — (correspondence_estimation_mod.hpp:
 * 134-162); normal shooting lists none (…normal_shooting_weighted.hpp:81-101); listed pairs pass the rejectors like any
 * other; then the FIRST rejector alone is applied to the given pairs and the survivors are appended, a second time for those
 * already listed (icp_mod.hpp:210-224; only when a rejector is installed; with both rejectors of ope_icp_params on, "the first"
 * is the surface-normal one — the params fix the order the reference's programs add them in, poseestimator.cpp:334-336).  SVD estimator only; not with reciprocal
 * correspondences; in a sharded run set them on exactly ONE rank (indices into that rank's shard): every rank that holds
 * pairs adds them to the sums that are then summed over the ranks.  ope_icp_correspondences lists the searched pairs only.  Runs with fixed
 * correspondences launch their update in line. */
int ope_icp_set_fixed_correspondences(ope_ctx *ctx, const ope_cloud *src, const ope_cloud *tgt_cloud, const int32_t *index_query,
                                      const int32_t *index_match, size_t n);
/* The given pairs as the LAST iteration of the last run saw them, in the order they were given (any output may be NULL;
 * *n = number of pairs set): distance[f] = the value the reference writes back into the caller's list through the pointer,
 * every iteration (impl/correspondence_estimation_mod.hpp:150-161: squared distance * 1e10 as float; under normal shooting the
 * squared distance to the source normal's line, impl/correspondence_estimation_normal_shooting_weighted.hpp:81-101);
 * listed[f] = 1 if the pair stands in the final correspondence list in front of the searched pairs (1-NN estimation, through
 * every rejector); appended[f] = 1 if it stands behind them once more (first rejector alone, impl/icp_mod.hpp:210-224).
 * The reference's correspondences_ = listed pairs, ope_icp_correspondences' pairs, appended pairs. */
int ope_icp_fixed_correspondences(ope_ctx *ctx, float *distance, int32_t *listed, int32_t *appended, size_t cap, size_t *n);

/* How many accumulate launches of the current (or last) run each search kernel served: the bucketed grid kernel, the
 * OBB-tree kernel in its per-lane and in its packet instantiation, the k-NN (normal shooting) kernel.  A run may move
 * between kernels (ope_index_params.grid = 1); tests use this to assert which kernel their comparison exercised. */
enum { OPE_KERNEL_GRID = 0, OPE_KERNEL_TREE_LANE = 1, OPE_KERNEL_TREE_PACKET = 2, OPE_KERNEL_KNN = 3, OPE_KERNEL_KINDS = 4 };
int ope_icp_kernel_launches(const ope_ctx *ctx, int64_t counts[OPE_KERNEL_KINDS]);
/* How many update steps of the current (or last) run were launched overlapped (ope_icp_params.update_launch). */
int64_t ope_icp_overlapped_updates(const ope_ctx *ctx);
/* How many runs of this context had an overlapped update launch give up its bounded wait (ope_ctx_set_wait_limit) and were
 * resumed in line on the same pose (0 unless the GPU was held up by something else for that long).  Results are unaffected;
 * TIMINGS are not: the launches enqueued behind the launch that gave up return at once and their iterations are enqueued
 * again, in line, by the next ope_icp_poll / ope_icp_end — a benchmark that brackets ope_icp_iterate with stream
 * synchronisation alone must check this counter (bench.py does, and measures again). */
int ope_icp_update_fallbacks(const ope_ctx *ctx);
/* Skip certificates of the run in progress (ope_icp_params.skip_certificates; synchronises the stream): out[0] = queries answered
 * from their certificate, summed over the run's launches; out[1] = accumulate launches that kept certificates; out[2] = 1 if the
 * run has reached the stage where it keeps them; out[3] = the last update's largest scene displacement in nanometres (what the
 * automatic mode compares with 1/24 of the target's point spacing). */
int ope_icp_certificate_stats(ope_ctx *ctx, int64_t out[4]);

/* Registration::align(output, guess) -> IterativeClosestPoint::computeTransformation
 * (registration_mod.hpp:176-219, icp_mod.hpp:119-272).  guess may be NULL (identity).
 * out_T receives getFinalTransformation(). */
int ope_icp_run(ope_ctx *ctx, const ope_cloud *src, const ope_index *tgt, const float *guess,
                const ope_icp_params *params, float out_T[16], ope_icp_result *result);

/* Batched ICP: n independent registrations in ONE launch, one workgroup per problem running its whole loop (search,
 * rejectors, sums, the update step and PCL's convergence rule of ope_icp_run) with no host round trip between iterations.
 * For many small problems, e.g. checking candidate clusters in order (rosinterface.cpp:243-262) or refining several
 * hypotheses.  Problem i registers src[i] to the target of tgt[i] from guesses[16*i .. 16*i+15] (column-major; guesses NULL =
 * identity for all).  One params for all problems; every run starts from the state ope_icp_begin would give it.
 * fitness_max_range >= 0: getFitnessScore(fitness_max_range) of each final transform (registration_mod.hpp:131-165; what
 * ope_fitness computes) in the same launch; < 0: no fitness pass (fitness = DBL_MAX, fitness_n = -1).  Synchronous, on the
 * context's stream; the state of the context's single run (ope_icp_correspondences, ope_icp_current_transform, the step-wise
 * calls) is left as it was.
 * Each problem's sums are added in a fixed order inside its workgroup: its result is bit-reproducible and does not depend on
 * the other problems of the batch or its position among them.  deterministic_sums, tree_walk, update_launch,
 * skip_certificates and check_every are ignored.
 * OPE_EINVAL, nothing launched: reciprocal correspondences, OPE_EST_POINT_TO_PLANE_LM, normal shooting or a rejector without
 * source normals, point-to-plane or the surface-normal rejector without target normals, k_normal_shooting outside 1..32 (normal
 * shooting), a source of more than 65536 valid points (use ope_icp_run), fixed correspondences set for one of the source
 * clouds, a context with a communicator.  OPE_EEMPTY: a NULL target.  n = 0 does nothing.  An empty or all-non-finite source,
 * or fewer than min_correspondences pairs, ends that problem with OPE_CONV_NO_CORRESPONDENCES; the others are unaffected. */
typedef struct {
  ope_icp_result result; /* as ope_icp_run reports it (align_strength from the problem's own cloud sizes) */
  float T[16];           /* final transformation, column-major */
  double fitness;        /* getFitnessScore(fitness_max_range) of T; DBL_MAX if no point is in range */
  int64_t fitness_n;     /* points that entered it */
} ope_icp_batch_result;
int ope_icp_run_batch(ope_ctx *ctx, size_t n, const ope_cloud *const *src, const ope_index *const *tgt, const float *guesses,
                      const ope_icp_params *params, double fitness_max_range, ope_icp_batch_result *out);

/* Step-wise form of the same loop, for one-process-per-GPU drivers that put a
 * collective between the local reduction and the transform update:
 *   begin -> { accumulate -> [all-reduce 17 doubles at ope_icp_sums_device()] -> update } * -> end
 * All launches go to the context stream; nothing synchronises the host except
 * ope_icp_poll / ope_icp_end. */
int ope_icp_begin(ope_ctx *ctx, const ope_cloud *src, const ope_index *tgt, const float *guess,
                  const ope_icp_params *params);
int ope_icp_accumulate(ope_ctx *ctx);
/* Device pointer to the fp64 sums {n, Σs[3], Σt[3], Σ t sᵀ[9], Σd²} (about the index pivot), followed for the
 * point-to-plane estimator by 21 + 6 normal-equation sums: all-reduce OPE_NUM_SUMS doubles (OPE_NUM_SUMS_MAX with
 * OPE_EST_POINT_TO_PLANE_LLS); the library reads and writes exactly that many. */
void *ope_icp_sums_device(ope_ctx *ctx);
int ope_icp_update(ope_ctx *ctx);
/* Use a caller-owned device buffer for the sums (e.g. a torch tensor that torch.distributed all-reduces):
 * OPE_NUM_SUMS doubles, OPE_NUM_SUMS_MAX for runs with OPE_EST_POINT_TO_PLANE_LLS; NULL restores the internal buffer. */
int ope_icp_set_sums_buffer(ope_ctx *ctx, void *device_ptr);
/* Enqueue n whole iterations (accumulate -> [RCCL all-reduce if ope_comm_init_rank was called] -> update)
 * without synchronising the host.  The accumulate launches ADD into the sums and ope_icp_update leaves them at
 * zero: in the stepwise form every ope_icp_accumulate must be followed by one ope_icp_update. */
int ope_icp_iterate(ope_ctx *ctx, int n_iterations);
int ope_icp_poll(ope_ctx *ctx, ope_icp_result *result); /* syncs the stream */
/* getFinalTransformation() of a run in progress (polls the device state): the transform after the iterations
 * enqueued so far. */
int ope_icp_current_transform(ope_ctx *ctx, float out_T[16]);
int ope_icp_end(ope_ctx *ctx, float out_T[16], ope_icp_result *result);
/* In sharded runs: the sizes getAlignStrength divides by (defaults: local sizes). */
int ope_icp_set_global_sizes(ope_ctx *ctx, int64_t n_src_total, int64_t n_tgt_total);

/* Measurement hook: bracket up to max_launches launches of the accumulate kernel (the dominant
 * kernel) with HIP events on the launch stream; 0 disables.  ope_icp_profile_read synchronises and
 * returns the summed kernel time and the number of launches timed since ope_icp_profile. */
int ope_icp_profile(ope_ctx *ctx, int max_launches);
int ope_icp_profile_read(ope_ctx *ctx, double *total_ms, int *n_launches);
/* The same per launch: ms[i] = duration of the i-th timed launch (at most cap of them), *n_out their number. */
int ope_icp_profile_launches(ope_ctx *ctx, float *ms, size_t cap, size_t *n_out);

/* Last iteration's post-rejection correspondences, compacted in query order
 * (pcl::Correspondences: index_query, index_match, distance = squared L2).  OPE_ESTATE when there is no finished
 * run on this context, or its source cloud has been freed since. */
int ope_icp_correspondences(ope_ctx *ctx, int32_t *index_query, int32_t *index_match, float *distance, size_t cap,
                            size_t *n);

/* getLastIncrementalTransformation() (transformation_, registration_mod.h): the incremental transform of the last
 * iteration of the run that ope_icp_end / ope_icp_poll last read back. */
int ope_icp_last_incremental(ope_ctx *ctx, float out_T[16]);

/* CorrespondenceRejector::getRemainingCorrespondences for n GIVEN correspondences (stand-alone use; inside the ICP loop the
 * same predicates are fused into the search kernel).  a, b: n packed float triples.
 *   OPE_REJ_SURFACE_NORMAL: a = source normal, b = matched target normal; keep iff a . b > threshold
 *                           (correspondence_rejection_mod.h:368-376)
 *   OPE_REJ_SELF_OCCLUDED:  a = source normal, b = source point; keep iff a . (-b / |b|) > threshold (:382-391) */
enum { OPE_REJ_SURFACE_NORMAL = 0, OPE_REJ_SELF_OCCLUDED = 1 };
int ope_reject_pairs(ope_ctx *ctx, int kind, const float *a, const float *b, size_t n, double threshold, unsigned char *keep);

/* ---- Global correspondence rejectors (global_rejectors.hip): the three of estimateFinePose's list (poseestimator.cpp:250-292,
 * blocks 3.1, 3.2, 3.5) that need ALL of an iteration's pairs before they can decide about one, as PCL 1.7.2 applies them without
 * a data container.  d_i = a pair's `distance` field (squared distance, fp32), m = the pairs that reach the rejector; every
 * comparison is made in fp64 on the widened value.  tests/global_rejectors_ref.py is the restatement the kernels are pinned to.
 *   OPE_GREJ_MEDIAN_DISTANCE  (correspondence_rejection_median_distance.cpp) median = the element at position m / 2 of the
 *       ascending d_i; keep iff d_i <= median * factor.  m = 0 keeps nothing (threshold NaN).
 *   OPE_GREJ_ONE_TO_ONE       (correspondence_rejection_one_to_one.cpp) among the pairs with one index_match keep the smallest
 *       d_i, on equal d_i the smallest index_query (PCL's std::sort leaves the tie open).  Stand-alone, pairs with
 *       index_match < 0 are dropped.  The pairs STAY IN QUERY ORDER: PCL's output is in match order, nothing downstream reads it.
 *   OPE_GREJ_VAR_TRIMMED      (correspondence_rejection_var_trimmed.cpp, lambda 3) s = the d_i ascending, lo = floor(min_ratio m),
 *       hi = floor(max_ratio m), L = s[0] + ... + s[lo-1]; for j in [lo, hi): FRMS_j = (1 / r^3)^2 (1 / (j+1)) (s[j] + L) with
 *       r = (j+1) / m (PCL's expression as written: L is the head only); best = the first j of the smallest FRMS;
 *       ratio = float(best) / float(m) (fp32); idx = int(double(m) * double(ratio)); keep iff d_i < s[idx] (strict).
 *       hi <= lo (PCL: undefined): every pair is kept, ratio = 1, threshold NaN.
 * A list applies its rejectors in order, each over the survivors of the one before.
 *
 * Inside the ICP loop the list is context state (like the fixed correspondences): it runs after the search kernel with its fused
 * pointwise rejectors and before the min_correspondences test (icp_mod.hpp:195-240); the update step reads the 17 sums of the
 * survivors alone (count, cross-covariance, sum of d^2 -> the MSE of the convergence rule), and n_corr, align_strength and
 * ope_icp_correspondences report the survivors.  A run with a list launches its update in line, adds the survivor sums in a fixed
 * order (bit-reproducible whatever deterministic_sums says), synchronises nothing and allocates nothing between iterations, and
 * its launches per iteration depend on the list alone.  ope_icp_begin answers OPE_EINVAL, nothing launched, while a list is set
 * and the run asks for reciprocal correspondences, an estimator other than OPE_EST_SVD, fixed correspondences or a context with a
 * communicator; ope_icp_run_batch, the ope_final_pose_batch* family and ope_track_pose answer OPE_EINVAL while a list is set.
 * The batched runs take a list as an ARGUMENT instead: ope_icp_run_batch_rejectors, ope_final_pose_batch_rejectors
 * (ope_batch_rejectors.h, included at the end of this header).
 * OPE_EINVAL for a parameter out of range: factor not finite or < 0, a ratio outside [0, 1], min_ratio > max_ratio, an unknown
 * kind, more than OPE_GREJ_MAX rejectors. */
enum { OPE_GREJ_MEDIAN_DISTANCE = 0, OPE_GREJ_ONE_TO_ONE = 1, OPE_GREJ_VAR_TRIMMED = 2 };
#define OPE_GREJ_MAX 4
typedef struct {
  int kind;
  double factor;                /* median distance: 1.0 (the reference's block uses 0.8) */
  double min_ratio, max_ratio;  /* var trimmed: 0.05, 0.95 (the reference's block uses min_ratio 0.3) */
} ope_global_rejector;
typedef struct {
  int64_t n_in, n_out;
  double threshold;   /* the median or the trimmed distance; NaN for one-to-one */
  double ratio;       /* var trimmed: the ratio chosen; else NaN */
  int64_t launches;   /* dispatches this rejector books per application: its own kernels, and one for the rocPRIM sort of var
                         trimmed whatever that launches inside; a function of the kind alone */
} ope_global_rejector_stats;
void ope_global_rejector_defaults(int kind, ope_global_rejector *r);
/* n <= OPE_GREJ_MAX; n = 0 (or list NULL) clears.  Holds for every later run of the context: ope_icp_begin takes a copy, so a run
 * in progress keeps the list it began with. */
int ope_icp_set_global_rejectors(ope_ctx *ctx, const ope_global_rejector *list, size_t n);
/* Rejector `which` of the list as the last iteration of the last run applied it.  OPE_ESTATE: no such run; OPE_EINVAL: which. */
int ope_icp_global_rejector_stats(ope_ctx *ctx, size_t which, ope_global_rejector_stats *out);
/* getRemainingCorrespondences of one rejector on n GIVEN pairs (the same kernels as in the loop): keep[i] = 1 for the survivors,
 * in the order given.  index_query / index_match are read by one-to-one only and may be NULL for the other kinds. */
int ope_reject_correspondences(ope_ctx *ctx, const ope_global_rejector *r, const int32_t *index_query, const int32_t *index_match,
                               const float *distance, size_t n, unsigned char *keep, ope_global_rejector_stats *stats);

/* Registration::getFitnessScore(max_range), registration_mod.hpp:131-165.
 * sum_out/n_out (optional) expose the partial sums for sharded runs. */
int ope_fitness(ope_ctx *ctx, const ope_cloud *src, const ope_index *tgt, const float T[16], double max_range,
                double *score, double *sum_out, int64_t *n_out);

/* registration::TransformationEstimationSVD::estimateRigidTransformation(src, tgt, correspondences, T)
 * (called stand-alone at poseestimator.cpp:429-435 with identity correspondences over the model).
 * src_xyz / tgt_xyz: n already-paired points, packed float[3] each.  Needs n >= 1. */
int ope_rigid_transform_svd(ope_ctx *ctx, const float *src_xyz, const float *tgt_xyz, size_t n, float out_T[16]);

/* pcl::transformPointCloud on the host copy of a result (float math): out = T * in. */
int ope_transform_cloud(ope_ctx *ctx, const ope_cloud *cloud, const float T[16], float *out_xyz);

/* ---------------- native RCCL path (optional; torch.distributed drivers use the step-wise API) ---------------- */
#define OPE_COMM_ID_BYTES 128
int ope_comm_get_unique_id(char id[OPE_COMM_ID_BYTES]);
int ope_comm_init_rank(ope_ctx *ctx, const char id[OPE_COMM_ID_BYTES], int nranks, int rank);
int ope_comm_destroy(ope_ctx *ctx);
/* How the 17 (44) sums of an iteration travel between the ranks of one node.
 *   OPE_COMM_AUTO (default): peer-to-peer slots if every rank could set them up and exchange a test pattern, else RCCL
 *   OPE_COMM_RCCL: ncclAllReduce on the run's stream, then the update kernel
 *   OPE_COMM_P2P:  peer-to-peer slots or an error — every rank stores its sums into a slot it owns in each peer's
 *                  fine-grained buffer (opened through hipIpc handles; 8-byte words {32 data bits, 32-bit sequence number},
 *                  so a word is valid the moment its number matches: no fence between data and flag), reads its own slots
 *                  in rank order and runs the update step in the same launch.  At most 8 ranks.
 * To be called with the same value on every rank, after ope_comm_init_rank and outside a run.
 * ope_comm_transport returns what iterations will use: OPE_COMM_RCCL or OPE_COMM_P2P (0 without a communicator). */
enum { OPE_COMM_AUTO = 0, OPE_COMM_RCCL = 1, OPE_COMM_P2P = 2 };
int ope_comm_set_transport(ope_ctx *ctx, int transport);
int ope_comm_transport(const ope_ctx *ctx);
/* The peer-to-peer slots WITHOUT an RCCL communicator, for drivers that have their own way of passing 64 bytes around
 * (torch.distributed with any backend, MPI, a file): every rank calls ope_comm_p2p_open and publishes the handle it gets;
 * every rank then calls ope_comm_p2p_connect with all handles in rank order.  connect is collective: it maps the peers'
 * buffers and runs the test exchange (up to 10 s); OPE_ECOMM on any rank means no rank may use the communicator — agree
 * on the return codes before iterating.  Such a communicator carries every estimator (17 / 44 sums per iteration, the LM
 * estimator's 17 + 91).  After an exchange has timed out (OPE_ECOMM from ope_icp_poll / ope_icp_end) the ranks' sequence
 * numbers no longer agree: ope_icp_begin refuses further runs until the communicator has been re-created
 * (ope_comm_destroy, then ope_comm_p2p_open / connect or ope_comm_init_rank again, on every rank). */
#define OPE_P2P_HANDLE_BYTES 64
int ope_comm_p2p_open(ope_ctx *ctx, char handle[OPE_P2P_HANDLE_BYTES]);
int ope_comm_p2p_connect(ope_ctx *ctx, const char *handles /* nranks * OPE_P2P_HANDLE_BYTES */, int nranks, int rank);

/* ---------------- features (coarse stage) ---------------- */
/* pcl::NormalEstimation::compute with setKSearch(k) and viewpoint vp (poseestimator.cpp:151-156).
 * out_normals n*3, out_curvature n (optional), ORIGINAL order; NaN where fewer than 3 neighbours.
 * The normals are also attached to `cloud` on the device; with both outputs NULL nothing is copied back. */
int ope_normals(ope_ctx *ctx, ope_cloud *cloud, int k, const float vp[3], float *out_normals, float *out_curvature);
/* The same with the neighbourhoods taken from another cloud's index: NormalEstimation::setSearchSurface
 * (pcl/features/feature.h), used here to shard the normals of one big cloud over ranks — every rank searches the whole
 * cloud's index for its own slice of the points. */
int ope_normals_from(ope_ctx *ctx, ope_cloud *queries, const ope_index *index, int k, const float vp[3], float *out_normals,
                     float *out_curvature);
/* pcl::FPFHEstimation::compute with setRadiusSearch(radius) on a cloud that carries
 * normals (poseestimator.cpp:121-125).  out33 n*33 floats, ORIGINAL order.
 * A point's neighbourhood is every finite point within the radius, squared distance <= radius * radius in float (a point at
 * exactly the radius is in), itself included.  A non-finite point is in no neighbourhood and gets a NaN row; a finite point
 * with nothing else in range gets a zero row; every other group of 11 bins sums to 100.
 * Duplicates: a point at distance 0 that is another point by index is a neighbour: it counts in the bin increment
 * 100 / (neighbours - 1), its pair is rejected (computePairFeatures: f4 == 0), and the weighted pass leaves out every
 * neighbour at distance 0, the point itself and its duplicates.
 * NaN normals (fewer than 3 neighbours, or a collinear neighbourhood: ope_normals) reject nothing and swap nothing, as in PCL,
 * whose tests are comparisons; a feature that comes out non-finite goes to bin 0 of its own group, feature by feature (PCL's
 * (int)floor(NaN) followed by its clamp).  The rows stay finite.  tests/fpfh_ref.py states all of it in fp64. */
int ope_fpfh(ope_ctx *ctx, const ope_cloud *cloud, float radius, float *out33);
/* pcl::UniformSampling::compute(PointCloud<int>&) with setRadiusSearch(leaf)
 * (poseestimator.cpp:141-145); survivors in ascending voxel-key order. */
int ope_uniform_sampling(ope_ctx *ctx, const ope_cloud *cloud, float leaf, int32_t *out_idx, size_t *n_out);


/* ---------------- filters either side of the path ---------------- */
/* pcl::removeNaNFromPointCloud (poseestimator.cpp:192-194): ORIGINAL indices of the finite points, ascending.
 * out_idx has room for every point of the cloud. */
int ope_remove_nan(ope_ctx *ctx, const ope_cloud *cloud, int32_t *out_idx, size_t *n_out);
/* pcl::PassThrough::filter on "z", then "y", then "x" with setFilterLimits(lo, hi) each
 * (BuildModel processingpcd.cpp:8-36): a finite point survives iff lo[d] <= p[d] <= hi[d] for d = x, y, z
 * (limits inclusive; use -/+FLT_MAX for an unfiltered field).  ORIGINAL indices, ascending. */
int ope_pass_through(ope_ctx *ctx, const ope_cloud *cloud, const float lo[3], const float hi[3], int32_t *out_idx,
                     size_t *n_out);
/* pcl::VoxelGrid::filter with setLeafSize(leaf[0], leaf[1], leaf[2]) (BuildModel processingpcd.cpp:39-52):
 * one centroid per occupied voxel, in ascending voxel index (PCL's output order); xyz only (ope_voxel_grid_rgb
 * carries the colours).  out_xyz has room for 3 floats per finite input point.  OPE_ERANGE where PCL would warn
 * "Leaf size is too small for the input dataset" and return the input unchanged. */
int ope_voxel_grid(ope_ctx *ctx, const ope_cloud *cloud, const float leaf[3], float *out_xyz, size_t *n_out);
/* pcl::VoxelGrid<PointXYZRGB>::filter as ProcessingPcd::getDownSampled runs it (BuildModel processingpcd.cpp:44-59,
 * downsample_all_data_ = true): besides the centroid, the packed colour is averaged channel by channel in float and
 * re-packed by truncation, alpha byte 0 (voxel_grid.hpp, "RGB special case").  rgb: the 32 bits of PointXYZRGB::rgb of
 * every input point, ORIGINAL order; out_rgb: one word per centroid.  rgb == NULL: ope_voxel_grid. */
int ope_voxel_grid_rgb(ope_ctx *ctx, const ope_cloud *cloud, const float leaf[3], const uint32_t *rgb, float *out_xyz,
                       uint32_t *out_rgb, size_t *n_out);
/* pcl::StatisticalOutlierRemoval::filter with setMeanK(mean_k) and setStddevMulThresh(stddev_mul)
 * (ProcessingPcd::getOutlierRemove, DetectAndLocalize processingpcd.cpp:62-77: meanK 30): a point is removed iff its mean
 * distance to its mean_k nearest neighbours exceeds mean + stddev_mul * stddev over the cloud.  ORIGINAL indices of the
 * inliers, ascending (out_idx has room for every point); non-finite points pass, as in PCL.  1 <= mean_k <= 31.
 * out_mean_dist (optional, n floats, ORIGINAL order): the per-point mean distances. */
int ope_statistical_outlier_removal(ope_ctx *ctx, const ope_cloud *cloud, int mean_k, double stddev_mul, int32_t *out_idx,
                                    size_t *n_out, float *out_mean_dist);
/* pcl::ConditionalRemoval with a ConditionAnd of six PackedRGBComparison (ProcessingPcd::getFilterRgb, BuildModel
 * processingpcd.cpp:112-141: "r" GT lo[0], "r" LT hi[0], then "g" and "b" alike): a point survives iff lo[c] < channel_c < hi[c]
 * for c = r, g, b of its colour word (ope_cloud_set_rgb; the top byte plays no part).  Strict integer comparisons, as
 * PackedRGBComparison compares the uint8 with the value.  The coordinates play no part: a non-finite point passes or fails by its
 * colour like any other.  ORIGINAL indices, ascending (out_idx has room for every point).  OPE_EINVAL for a cloud without
 * colours. */
int ope_color_filter(ope_ctx *ctx, const ope_cloud *cloud, const int32_t lo[3], const int32_t hi[3], int32_t *out_idx, size_t *n_out);

/* Device-resident forms of the filters above: the survivors are handed on as a new cloud (*out, as ope_cloud_select of the
 * indices the host form returns would build it), so that crop -> outlier removal -> key points -> normals -> FPFH -> SAC-IA
 * runs without a host round trip per stage.  out_idx (optional, room for every point) receives the same ORIGINAL indices
 * as the host form; n_out (optional) their number. */
int ope_remove_nan_cloud(ope_ctx *ctx, const ope_cloud *cloud, ope_cloud **out, int32_t *out_idx, size_t *n_out);
int ope_pass_through_cloud(ope_ctx *ctx, const ope_cloud *cloud, const float lo[3], const float hi[3], ope_cloud **out, int32_t *out_idx,
                           size_t *n_out);
int ope_statistical_outlier_removal_cloud(ope_ctx *ctx, const ope_cloud *cloud, int mean_k, double stddev_mul, ope_cloud **out,
                                          int32_t *out_idx, size_t *n_out);
int ope_uniform_sampling_cloud(ope_ctx *ctx, const ope_cloud *cloud, float leaf, ope_cloud **out, int32_t *out_idx, size_t *n_out);
int ope_color_filter_cloud(ope_ctx *ctx, const ope_cloud *cloud, const int32_t lo[3], const int32_t hi[3], ope_cloud **out, int32_t *out_idx,
                           size_t *n_out);

typedef struct {
  int max_iterations;      /* 400  (poseestimator.cpp:55) */
  int nr_samples;          /* 5    (:56) */
  int k_correspondences;   /* 5    (:57) */
  double max_corr_dist;    /* 0.05 (:58) */
  float min_sample_dist;   /* 0.01 (:59) */
  uint64_t seed;           /* PCL uses unseeded rand(); here an explicit LCG stream */
} ope_sacia_params;
void ope_sacia_default_params(ope_sacia_params *p);
/* pcl::SampleConsensusInitialAlignment::align (poseestimator.cpp:50-64).
 * src_feat/tgt_feat: n*33 floats in ORIGINAL order.  forced_samples (optional):
 * max_iterations*nr_samples source indices then as many target indices.
 * A hypothesis with a drawn sample whose descriptor matches nothing (a NaN row, as ope_fpfh writes
 * it for a non-finite point) or with a fit that is not finite is void: it scores |source| and its
 * transform is the identity.  The call goes on and returns OPE_OK. */
int ope_sacia(ope_ctx *ctx, const ope_cloud *src, const float *src_feat33, const ope_cloud *tgt,
              const ope_index *tgt_index, const float *tgt_feat33, const ope_sacia_params *params,
              const int32_t *forced_samples, float out_T[16], double *best_error, int32_t *best_iteration);

/* ---------------- prerejective coarse alignment ---------------- */
/* pcl::SampleConsensusPrerejective::align with the parameters of the block the reference keeps commented out
 * (BuildModel/src/poseestimator.cpp:90-108), the initial guess the identity.  Every iteration is drawn up front, tested by
 * CorrespondenceRejectorPoly in one launch, and the survivors are fitted and scored together. */
typedef struct {
  int32_t max_iterations;      /* 50000 (:97); 1 .. 2^20 */
  int32_t nr_samples;          /* 3     (:98); 3 .. 8 */
  int32_t k_correspondences;   /* 5     (:99) setCorrespondenceRandomness; 1 .. 8 */
  float similarity_threshold;  /* 0.8   (:100); [0, 1) */
  double max_corr_dist;        /* 0.15  (:101) the inlier distance; > 0 */
  float inlier_fraction;       /* 0.25  (:102); [0, 1] */
  uint64_t seed;               /* 1: the LCG stream of ope_sacia */
} ope_prerejective_params;
void ope_prerejective_default_params(ope_prerejective_params *p);
typedef struct {
  float T[16];             /* column-major; the identity without a winner */
  double error;            /* the winner's mean squared inlier distance; FLT_MAX without a winner */
  int32_t best_iteration;  /* -1 without a winner */
  int32_t inliers;
  int32_t converged;
} ope_prerejective_result;
typedef struct {
  int64_t iterations;   /* hypotheses drawn (max_iterations) */
  int64_t survivors;    /* hypotheses the polygon test let through */
  int64_t launches;     /* kernel launches and copies to the device enqueued (a rocPRIM select counts as one) */
  int64_t host_syncs;
  int64_t nr_samples;   /* of that call: what ope_prerejective_last_hypotheses writes per iteration into samples and targets */
} ope_prerejective_stats;
/* src_feat33 / tgt_feat33: n * 33 floats in ORIGINAL order.  Per iteration the host draws nr_samples distinct source indices
 * int(ns * next()) and then nr_samples picks int(k * next()); the target of a sample is the pick-th of the k nearest target
 * descriptors of its source descriptor.  forced_samples (optional): max_iterations * nr_samples source indices then as many target
 * indices, taken instead of the draws and the feature search (the features may then be NULL).
 * An iteration survives iff every edge i -> (i + 1) mod nr_samples has min(ds, dt) / max(ds, dt) >= similarity_threshold^2 (squared
 * lengths in the source and in the target, float; a NaN ratio fails).  A survivor's transform is Umeyama without scaling over its
 * pairs (fp64).  Its inliers are the finite source points whose moved image has a nearest target point at a squared distance
 * (float, widened) < max_corr_dist^2; its error is the fp64 sum of those squared distances over their number (FLT_MAX for
 * none).  In iteration order a survivor is accepted iff (float)inliers / (float)|source| >= inlier_fraction and its error is below
 * the lowest so far.  out_inliers (optional, room for every source point): the winner's inliers, ORIGINAL indices ascending,
 * out->inliers of them.  No winner: OPE_OK, converged = 0.
 * params may be NULL: the defaults of ope_prerejective_default_params (as ope_sacia takes a NULL params).
 * OPE_EINVAL, nothing launched: a NULL ctx, src, tgt, tgt_index or out (or features, without forced_samples); a parameter outside
 * the ranges above; fewer source points than nr_samples; an empty target (a cloud without a finite point, or an index over none);
 * k_correspondences above the number of target points; a forced index out of range; a context with a communicator.  OPE_EINVAL
 * after the feature search, nothing more launched: a sampled source descriptor without a single finite distance to a target
 * descriptor (NaN rows).
 * Launches and synchronisations depend on neither the iterations, the survivors nor the points (ope_prerejective_last_stats). */
int ope_prerejective(ope_ctx *ctx, const ope_cloud *src, const float *src_feat33, const ope_cloud *tgt, const ope_index *tgt_index,
                     const float *tgt_feat33, const ope_prerejective_params *params, const int32_t *forced_samples,
                     ope_prerejective_result *out, int32_t *out_inliers);
int ope_prerejective_last_stats(const ope_ctx *ctx, ope_prerejective_stats *out);
/* The iterations of the last ope_prerejective in drawing order: samples and targets (ope_prerejective_stats.nr_samples ORIGINAL
 * indices each, cap * nr_samples entries of room), survived (1 / 0), T (16 floats, column-major), inliers and error; an iteration
 * that did not survive has the identity, 0 and FLT_MAX.  Any output may be NULL; at most cap iterations are written, *n_out = how
 * many there were. */
int ope_prerejective_last_hypotheses(const ope_ctx *ctx, int32_t *samples, int32_t *targets, uint8_t *survived, float *T,
                                     int32_t *inliers, double *error, size_t cap, size_t *n_out);

/* ---------------- feature matches filtered by RANSAC ---------------- */
/* The third coarse aligner of estimateCoarsePose, which the reference keeps commented out (BuildModel/src/poseestimator.cpp:43-60,
 * :111-113): pcl::registration::CorrespondenceEstimation over FPFH rows, CorrespondenceRejectorSampleConsensus over the matches,
 * TransformationEstimationSVD over the matches that remain (tests/corr_sac_ref.py is the specification).
 *
 * ope_feature_correspondences: source row i (ORIGINAL order, n * 33 floats) is matched to the target row with the smallest squared
 * L2 distance (float, component after component), the lowest index on a tie; out_dist (optional) is that squared distance.  A row
 * without a finite distance (NaN or infinite everywhere) gives no match: *n_out matches are written, in source order (the outputs
 * have room for n_src), and n_src - *n_out rows were dropped.  No rows on either side: no matches, nothing launched.
 * OPE_EINVAL, nothing launched: a NULL ctx, output or feature array; more than 2^31 - 1 rows. */
int ope_feature_correspondences(ope_ctx *ctx, const float *src_feat33, size_t n_src, const float *tgt_feat33, size_t n_tgt,
                                int32_t *out_src_idx, int32_t *out_tgt_idx, float *out_dist, size_t *n_out);
typedef struct {
  double inlier_threshold;   /* 0.05, CorrespondenceRejectorSampleConsensus's default (the reference sets 0.08); > 0 */
  int32_t max_iterations;    /* 1000; 1 .. 2^20 */
  double probability;        /* 0.99; inside (0, 1) */
  uint64_t seed;             /* 12345: std::mt19937 takes its low 32 bits */
} ope_corr_sac_params;
void ope_corr_sac_default_params(ope_corr_sac_params *p);
typedef struct {
  float T_best[16];     /* getBestTransformation: the winning hypothesis, column-major; the identity without a model */
  float T_svd[16];      /* TransformationEstimationSVD over the remaining matches (all of them without a model) */
  int32_t inliers;      /* remaining matches */
  int32_t best;         /* the winning hypothesis in drawing order; -1 without a model */
  int32_t iterations;   /* RandomSampleConsensus::iterations_ */
  int32_t found;
} ope_corr_sac_result;
typedef struct {
  int64_t hypotheses;   /* samples drawn (or forced) and scored */
  int64_t iterations;
  int64_t launches;     /* kernel launches, fills and copies to the device enqueued */
  int64_t host_syncs;
  double sample_dist_thresh;   /* as the draws used it */
} ope_corr_sac_stats;
/* Match i pairs ORIGINAL point src_idx[i] of src with tgt_idx[i] of tgt.  The model is SampleConsensusModelRegistration:
 * sample_dist_thresh from the eigenvalues of the matched source points' float covariance; a sample is three matches (positions in
 * 0 .. n - 1) drawn by drawIndexSample with std::mt19937 (seed), redrawn up to 1000 times until every squared edge of its source
 * triangle is above the threshold; its transform is Umeyama without scaling over the three pairs (fp64, cast to float); a match is
 * within the distance iff |T s - t|^2 (float, widened) < inlier_threshold^2.  Every sample RandomSampleConsensus::computeModel can
 * reach (max_iterations + 1) is drawn and scored, and the loop is replayed from the counts.  forced_samples (optional): n_forced
 * triples of match positions taken instead of the draws (isSampleGood is not asked).
 * With a model: out_inlier_pos (optional, room for n) receives the positions of the matches within the distance of the winner,
 * ascending, out->inliers of them.  Without one (fewer than 3 matches, or no good sample in 1000 draws): OPE_OK, found = 0, best = -1,
 * the identity as T_best, every match remains (positions 0 .. n - 1) and T_svd is fitted over all of them.  n == 0: both the identity,
 * nothing launched.  refineModel is not built.
 * params may be NULL: the defaults of ope_corr_sac_default_params.
 * OPE_EINVAL, nothing launched: a NULL ctx, src, tgt or out (or index arrays with n > 0, or forced_samples with n_forced > 0);
 * max_iterations outside 1 .. 2^20, inlier_threshold <= 0 or not finite, probability outside (0, 1); more than OPE_COARSE_MAX_KEYS
 * matches; more than 2^20 + 1 forced samples; a match index out of range; a source index in two matches (PCL's index map would keep
 * the last); a match on a non-finite point; a forced position out of range; a context with a communicator.
 * Launches and synchronisations depend on neither the hypotheses, the matches (n >= 1), the iteration the loop stops at nor the
 * inliers (ope_corr_sac_last_stats). */
int ope_corr_sac(ope_ctx *ctx, const ope_cloud *src, const ope_cloud *tgt, const int32_t *src_idx, const int32_t *tgt_idx, size_t n,
                 const ope_corr_sac_params *params, const int32_t *forced_samples, size_t n_forced, ope_corr_sac_result *out,
                 int32_t *out_inlier_pos);
int ope_corr_sac_last_stats(const ope_ctx *ctx, ope_corr_sac_stats *out);
/* The hypotheses of the last ope_corr_sac in drawing order: samples (3 match positions), T (16 floats, column-major) and counts.
 * Any output may be NULL; at most cap hypotheses are written, *n_out = how many there were. */
int ope_corr_sac_last_hypotheses(const ope_ctx *ctx, int32_t *samples, float *T, int32_t *counts, size_t cap, size_t *n_out);

/* ---------------- batched coarse stage ---------------- */
/* estimateCoarsePose (poseestimator.cpp:16-73) of one model against n candidate clusters in one call: the coarse half of the
 * reference's candidate loop (rosinterface.cpp:243-262).  Each cloud is uniformly sampled at key_leaf, gets k-NN normals and
 * FPFH on its key points, and SAC-IA aligns the model's key points (source) to each cluster's (target). */
typedef struct {
  float key_leaf;          /* UniformSampling radius, 0.01 (poseestimator.cpp:116) */
  int normals_k;           /* 30 (:153) */
  float viewpoint[3];      /* NormalEstimation's default, 0 0 0 */
  float fpfh_radius;       /* 0.03 (:122) */
  ope_sacia_params sacia;  /* 400 / 5 / 5 / 0.05 / 0.01, seed 1 */
} ope_coarse_params;
void ope_coarse_default_params(ope_coarse_params *p);

/* Limits of one batch: points of one cloud (model or cluster), and key points of one cloud after sampling (each cloud's key
 * points are staged in LDS).  Larger clouds go through the single-cloud calls.  The limits are inclusive: a cloud of exactly
 * OPE_COARSE_MAX_KEYS key points is accepted (its FPFH launch holds 2 x 4096 float4 and the histograms, 148 KB of the 160 KB of
 * LDS), one more key point is refused.  The batch's FPFH follows ope_fpfh's rules; duplicates never reach it, uniform sampling
 * keeps one point per voxel. */
#define OPE_COARSE_MAX_POINTS 65536
#define OPE_COARSE_MAX_KEYS 4096

enum { OPE_COARSE_OK = 0, OPE_COARSE_EMPTY_TARGET = 1, OPE_COARSE_FEW_TARGET_FEATURES = 2 };
typedef struct {
  float T[16];             /* coarse pose, column-major; identity unless status == OPE_COARSE_OK */
  double best_error;       /* computeErrorMetric of the winning hypothesis */
  int32_t best_iteration;  /* -1 unless OK */
  int32_t n_src_keys;      /* model key points after UniformSampling */
  int32_t n_tgt_keys;      /* this cluster's key points */
  int32_t status;
} ope_coarse_batch_result;

/* Synchronous, on the context's stream; the single-run state of the context is untouched; n == 0 does nothing.
 * Cluster i draws with seeds[i], or with params->sacia.seed + i when seeds is NULL (the i-th coarse call of an estimator).
 * An empty cluster gives OPE_COARSE_EMPTY_TARGET, fewer than 10 cluster key points OPE_COARSE_FEW_TARGET_FEATURES (:40-45);
 * both keep the identity.  The model's features are computed once per call.  Each cluster's result is byte-identical whatever
 * else is in the batch and wherever it sits.  The number of kernel launches and host synchronisations does not depend on n.
 * OPE_EINVAL, nothing launched: a model with fewer than sacia.nr_samples key points, normals_k outside 1..32,
 * k_correspondences outside 1..8, key_leaf or fpfh_radius <= 0, a cloud of more than OPE_COARSE_MAX_POINTS points or more than
 * OPE_COARSE_MAX_KEYS key points.  (Key points are counted on the host before anything is launched.) */
int ope_coarse_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                          const ope_coarse_params *params, const uint64_t *seeds, ope_coarse_batch_result *out);
/* Key points (ORIGINAL indices into that cloud), normals (n*3) and FPFH rows (n*33) the last ope_coarse_pose_batch (or
 * ope_prerejective_pose_batch, ope_final_pose_batch_prerejective, ope_corr_sac_pose_batch, ope_final_pose_batch_correspondences: the front end is the same code) computed for `which` (-1 = the model, 0..n-1 = cluster), in key-point order; any output may be NULL.  *n_out = the key points; at
 * most cap rows are written.  Like ope_icp_correspondences for the single run. */
int ope_coarse_batch_features(ope_ctx *ctx, int which, int32_t *key_idx, float *normals, float *fpfh33, size_t cap,
                              size_t *n_out);

/* ---------------- batched final pose: the reference's first-frame candidate loop ---------------- */
/* PoseEstimator::estimateFinalPose(model, cluster) (poseestimator.cpp:383-448) of one model against n candidate clusters in one
 * call, as the reference's first frame runs it cluster by cluster (rosinterface.cpp:243-262): the coarse stage of
 * ope_coarse_pose_batch, then the fine stage's preparation (:186-223) and its ICP (:229-363) with getFitnessScore, for every
 * cluster at once.  The composite coarse * fine and the re-anchoring (rigidmodelPose) stay with the caller. */
typedef struct {
  ope_coarse_params coarse;  /* ope_coarse_default_params */
  float fine_leaf;           /* UniformSampling radius of the fine clouds, 0.008 (poseestimator.cpp:196-216) */
  int fine_normals_k;        /* 30 */
  int min_fine_points;       /* 100 (:218-223): fewer fine target points and the fine pose is the identity */
  ope_icp_params icp;        /* the fine stage: 100 iterations, 1e-8, 1e-8, normal shooting k = 20, surface-normal rejector 0.7 */
  double fitness_max_range;  /* getFitnessScore's default: DBL_MAX */
  double accept_fitness;     /* the loop stops at fitness < 1e-4 (rosinterface.cpp:256) */
  double accept_strength;    /* ... or align strength > 0.4 */
} ope_final_params;
void ope_final_default_params(ope_final_params *p);

/* ope_final_batch_result.status */
enum {
  OPE_FINAL_OK = 0,                  /* coarse pose found, fine ICP ran */
  OPE_FINAL_EMPTY_TARGET = 1,        /* an empty cluster: the loop skips it (nothing ran) */
  OPE_FINAL_FEW_TARGET_FEATURES = 2, /* fewer than 10 coarse key points: coarse pose = identity, fine ICP ran from the model
                                        (only with min_fine_points lowered: < 10 cm-voxels hold < 100 fine points) */
  OPE_FINAL_FEW_FINE_POINTS = 3      /* fewer than min_fine_points fine target points: fine pose = identity, no ICP */
};
typedef struct {
  ope_coarse_batch_result coarse; /* as ope_coarse_pose_batch reports it */
  uint64_t seed;                  /* the SAC-IA stream this cluster drew with; 0 if it did not reach SAC-IA */
  ope_icp_batch_result fine;      /* the fine ICP from the identity (T, result, fitness, fitness_n); identity and zeros without ICP */
  int32_t n_fine_src;             /* fine key points (after the NaN-normal drop) of the moved model */
  int32_t n_fine_tgt;             /* ... and of the cluster */
  int32_t status;                 /* OPE_FINAL_* */
  int32_t accepted;               /* ICP ran and fitness < accept_fitness || align_strength > accept_strength */
} ope_final_batch_result;

/* Synchronous, on the context's stream; n == 0 does nothing.  Cluster i is what estimateFinalPose does on a fresh estimator:
 *   coarse: ope_coarse_pose_batch's result, except that without seeds cluster i draws with coarse.sacia.seed + (the clusters
 *           before it that reached SAC-IA): empty clusters and clusters with fewer than 10 key points use up no seed
 *           (the estimator's coarse-call counter); seeds[i] if seeds is given;
 *   fine source: the model moved by the coarse pose (pcl::transformPointCloud's float arithmetic, non-finite points left as they
 *           are; identity unless the coarse status is OK), NaNs removed, UniformSampling(fine_leaf), k-NN normals
 *           (fine_normals_k, coarse.viewpoint), rows with a non-finite normal dropped (withNormals);
 *   fine target: the same preparation of the cluster;
 *   fine ICP: ope_icp_run_batch of the two from the identity, the target indexed as ope_index_build indexes it (default leaf size),
 *           with getFitnessScore(fitness_max_range).
 * *selected = the first accepted cluster, or -1.  The launches and host synchronisations do not depend on n; each cluster's
 * result is byte-identical whatever else is in the batch.  For ONE cluster the single-run calls are faster: one workgroup runs
 * the whole fine ICP here (ope_icp_run_batch), so at C1 size one cluster takes ~1.3x one estimateFinalPose chain, while 8
 * clusters take 3.4x less than 8 chains.
 * OPE_EINVAL, nothing launched: what ope_coarse_pose_batch or ope_icp_run_batch refuses (LM, reciprocal correspondences, a context
 * with a communicator, ...), fine_leaf <= 0, fine_normals_k outside 1..32, a cluster of more than OPE_COARSE_MAX_KEYS fine key
 * points.  OPE_EINVAL after sampling (the moved model is only known there), nothing more launched and the context usable: a
 * moved model with more than OPE_COARSE_MAX_KEYS fine key points, or a fine_leaf too small for it. */
int ope_final_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters, const ope_final_params *params,
                         const uint64_t *seeds, ope_final_batch_result *out, int32_t *selected);
/* The fine inputs the last ope_final_pose_batch prepared: cluster `which`, side 0 = the moved model (source), 1 = the cluster
 * (target); xyz (n*3) and normals (n*3) in key-point order, as they would be handed to ope_cloud_upload; either may be NULL.
 * *n_out = the points; at most cap rows are written. */
int ope_final_batch_inputs(ope_ctx *ctx, int which, int side, float *xyz, float *normals, size_t cap, size_t *n_out);

/* ---------------- batched prerejective coarse stage ---------------- */
/* estimateCoarsePose with the prerejective aligner (ope_prerejective) of one model against n candidate clusters in one call:
 * the front end of ope_coarse_pose_batch (key points, normals, FPFH of every cloud), then every active cluster's draws, polygon
 * tests, fits and scores together.  The model's key points are the source, a cluster's the target. */
enum { OPE_PREREJ_OK = 0, OPE_PREREJ_EMPTY_TARGET = 1, OPE_PREREJ_FEW_TARGET_FEATURES = 2, OPE_PREREJ_NAN_FEATURES = 3 };
typedef struct {
  float T[16];             /* column-major; identity unless converged */
  double error;            /* the winner's mean squared inlier distance; FLT_MAX without a winner */
  int32_t best_iteration;  /* -1 without a winner */
  int32_t inliers;
  int32_t converged;
  int32_t survivors;       /* of this cluster's polygon test */
  int32_t n_src_keys;      /* model key points after UniformSampling */
  int32_t n_tgt_keys;      /* this cluster's key points */
  int32_t status;          /* OPE_PREREJ_* */
  uint64_t seed;           /* the stream this cluster drew with; 0 unless status == OPE_PREREJ_OK */
} ope_prerejective_batch_result;
typedef struct {
  int64_t clusters;     /* n */
  int64_t active;       /* clusters that drew (>= 10 key points) */
  int64_t iterations;   /* per active cluster (max_iterations) */
  int64_t survivors;    /* of all clusters */
  int64_t launches;     /* kernel launches and copies to the device enqueued after the front end (a rocPRIM select counts as one) */
  int64_t host_syncs;   /* of the whole call, the front end's one included */
  int64_t nr_samples;
} ope_prerejective_batch_stats;
/* Synchronous, on the context's stream; n == 0 does nothing.  front gives key_leaf, normals_k, viewpoint and fpfh_radius
 * (front->sacia is ignored; NULL: ope_coarse_default_params), params everything else (NULL: ope_prerejective_default_params).
 * Cluster i draws with seeds[i], or with params->seed + i.  Per cluster the result is what ope_prerejective gives for the
 * model's key points and FPFH rows against the cluster's (ope_coarse_batch_features reports both), n_src = the model's key
 * points: the same draws, targets, survival flags, transforms and inlier counts; the error sums the same squared distances in
 * KEY-POINT order (256 key points per partial sum, the partials in order), so it can differ from the single call's, which sums
 * along its cloud's stored order, in the last bits.
 * Status: an empty cluster OPE_PREREJ_EMPTY_TARGET; fewer than 10 cluster key points OPE_PREREJ_FEW_TARGET_FEATURES; a cluster in
 * which a sampled model descriptor has no finite distance to any descriptor (where ope_prerejective answers OPE_EINVAL)
 * OPE_PREREJ_NAN_FEATURES.  All three keep the identity, report seed 0 and leave the other clusters' results untouched.  No
 * winner: OPE_PREREJ_OK with converged = 0, the identity and best_iteration = -1.  Each cluster's result is byte-identical
 * whatever else is in the batch and wherever it sits.  Launches and host synchronisations depend on neither n, the iterations,
 * the survivors nor the points, as long as the packed draws (2 bytes each) of all active clusters fit the 32 MiB staging block;
 * beyond it the upload goes in synchronising pieces, which ope_prerejective_batch_last_stats counts.
 * keep_hypotheses != 0 keeps every iteration of every active cluster for ope_prerejective_batch_hypotheses (3.2 MB per cluster
 * at the defaults).
 * OPE_EINVAL, nothing launched: a NULL ctx, model, clusters, a cluster or out; n > 65535; n * max_iterations above 2^31 - 1;
 * key_leaf or fpfh_radius <= 0; normals_k outside 1..32; a parameter outside ope_prerejective's ranges (max_iterations 1..2^20,
 * nr_samples 3..8, k_correspondences 1..8, similarity_threshold [0, 1), inlier_fraction [0, 1], max_corr_dist > 0 and finite);
 * a cloud of more than OPE_COARSE_MAX_POINTS points or more than OPE_COARSE_MAX_KEYS key points; a model with fewer key points
 * than nr_samples; a context with a communicator. */
int ope_prerejective_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                const ope_coarse_params *front, const ope_prerejective_params *params, const uint64_t *seeds,
                                int keep_hypotheses, ope_prerejective_batch_result *out);
int ope_prerejective_batch_last_stats(const ope_ctx *ctx, ope_prerejective_batch_stats *out);
/* The iterations of cluster `which` of the last ope_prerejective_pose_batch with keep_hypotheses, in the shape of
 * ope_prerejective_last_hypotheses (samples: model key points, targets: the cluster's key points, both in key-point order).
 * *n_out = the iterations: 0 for a cluster that did not draw.  OPE_EINVAL: no such call yet, or `which` out of range. */
int ope_prerejective_batch_hypotheses(const ope_ctx *ctx, int which, int32_t *samples, int32_t *targets, uint8_t *survived, float *T,
                                      int32_t *inliers, double *error, size_t cap, size_t *n_out);
/* ope_final_pose_batch with ope_prerejective_pose_batch as its coarse stage (params->coarse is its front; prerejective NULL: the
 * defaults).  out[i].coarse: T, best_error = error, best_iteration, the key counts, status OPE_COARSE_* (OPE_PREREJ_NAN_FEATURES
 * reads OPE_COARSE_FEW_TARGET_FEATURES); a cluster without a winner stays OPE_COARSE_OK with the identity, which is what
 * PoseEstimator's prerejective coarse stage leaves (an identity pose and a counted coarse call).  Without seeds cluster i draws
 * with prerejective->seed + (the clusters before it that drew), the estimator's coarse-call counter; out[i].seed as above.
 * Everything after the coarse stage, *selected and the refusals are ope_final_pose_batch's; ope_final_batch_inputs reports its
 * fine inputs. */
int ope_final_pose_batch_prerejective(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                      const ope_final_params *params, const ope_prerejective_params *prerejective, const uint64_t *seeds,
                                      ope_final_batch_result *out, int32_t *selected);

/* ---------------- batched correspondence coarse stage ---------------- */
/* estimateCoarsePose with the third aligner (ope_feature_correspondences + ope_corr_sac) of one model against n candidate clusters
 * in one call: the front end of ope_coarse_pose_batch (key points, normals, FPFH of every cloud), then every active cluster's
 * matches, threshold, fits, counts, inliers and pose together.  The model's key points are the source, a cluster's
 * the target; every index is in KEY-POINT order (ope_coarse_batch_features reports the key points and rows). */
enum { OPE_CORRSAC_OK = 0, OPE_CORRSAC_EMPTY_TARGET = 1, OPE_CORRSAC_FEW_TARGET_FEATURES = 2 };
typedef struct {
  float T_svd[16];            /* the coarse pose: TransformationEstimationSVD over the remaining matches; identity unless OK and matches > 0 */
  float T_best[16];           /* the winning hypothesis; identity without a model */
  double sample_dist_thresh;  /* as this cluster's draws used it */
  uint64_t seed;              /* the stream it drew with; 0 unless status == OK */
  int32_t matches;            /* model rows with a finite match in this cluster */
  int32_t inliers;            /* remaining matches (= matches without a model) */
  int32_t best, iterations, found;   /* as ope_corr_sac_result */
  int32_t n_src_keys, n_tgt_keys, status;
} ope_corr_sac_batch_result;   /* 176 bytes */
typedef struct {
  int64_t clusters;     /* n */
  int64_t active;       /* clusters that reached the matcher (>= 10 key points) */
  int64_t hypotheses;   /* scored, all clusters */
  int64_t draw_lists;   /* sample lists drawn and uploaded: clusters with the same seed and the same matched model rows share one */
  int64_t launches;     /* kernel launches, fills and copies to the device enqueued after the front end */
  int64_t host_syncs;   /* of the whole call, the front end's one included */
} ope_corr_sac_batch_stats;
/* Synchronous, on the context's stream; n == 0 does nothing.  front gives key_leaf, normals_k, viewpoint and fpfh_radius
 * (front->sacia is ignored; NULL: ope_coarse_default_params), params everything else (NULL: ope_corr_sac_default_params).
 * Cluster i draws with seeds[i]; without seeds every cluster draws with params->seed (the reference's rejector is a new object per
 * call and never reseeds).  Per cluster the result is what ope_feature_correspondences + ope_corr_sac give for the model's key
 * points and FPFH rows against the cluster's: the same matches, distances, threshold, samples, transforms, counts, winner,
 * iterations, inlier positions and T_svd, bit for bit.
 * Status: an empty cluster OPE_CORRSAC_EMPTY_TARGET; fewer than 10 cluster key points OPE_CORRSAC_FEW_TARGET_FEATURES; both keep
 * the identities, report seed 0 and leave the other clusters untouched.  Within OPE_CORRSAC_OK: model rows without a finite
 * distance are dropped; fewer than 3 matches or no good sample: found = 0, best = -1, T_best the identity, T_svd over all matches;
 * no match at all: both the identity.  Each cluster's result is byte-identical whatever else is in the batch and wherever it sits.
 * 12 launches and copies after the front end and 4 synchronisations, whatever n, the hypotheses, the matches, the inliers or the
 * iteration a loop stops at, as long as the packed samples (6 bytes each) of all draw lists fit the 32 MiB staging block; beyond
 * it the upload goes in synchronising pieces, which ope_corr_sac_batch_last_stats counts.  When no cluster reaches the matcher
 * (every one empty or below 10 key points) the call ends after the front end: 0 launches and 2 synchronisations.
 * keep_hypotheses != 0 keeps every hypothesis of every active cluster for ope_corr_sac_batch_hypotheses (80 bytes each).
 * OPE_EINVAL, nothing launched: a NULL ctx, model, clusters, a cluster or out; n > 65535; n * (max_iterations + 1) above 2^31 - 1;
 * a parameter outside ope_corr_sac's ranges; key_leaf or fpfh_radius <= 0; normals_k outside 1..32; a cloud of more than
 * OPE_COARSE_MAX_POINTS points or more than OPE_COARSE_MAX_KEYS key points; a model with fewer than 3 key points; a context with a
 * communicator. */
int ope_corr_sac_pose_batch(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                            const ope_coarse_params *front, const ope_corr_sac_params *params, const uint64_t *seeds,
                            int keep_hypotheses, ope_corr_sac_batch_result *out);
int ope_corr_sac_batch_last_stats(const ope_ctx *ctx, ope_corr_sac_batch_stats *out);
/* Cluster `which` of the last ope_corr_sac_pose_batch.  Its matches in model key order (model key, cluster key, squared descriptor
 * distance); the remaining matches (ascending positions in the match list and the pair of keys of each); with keep_hypotheses its
 * hypotheses in drawing order (3 match positions, T column-major, count), otherwise *n_out = 0.  Any output may be NULL; at most cap
 * entries are written, *n_out = how many there were (0 for a cluster that did not reach the matcher).  OPE_EINVAL: no such call
 * yet, or `which` out of range. */
int ope_corr_sac_batch_matches(const ope_ctx *ctx, int which, int32_t *src_key, int32_t *tgt_key, float *dist, size_t cap, size_t *n_out);
int ope_corr_sac_batch_inliers(const ope_ctx *ctx, int which, int32_t *pos, int32_t *src_key, int32_t *tgt_key, size_t cap, size_t *n_out);
int ope_corr_sac_batch_hypotheses(const ope_ctx *ctx, int which, int32_t *samples, float *T, int32_t *counts, size_t cap, size_t *n_out);
/* ope_final_pose_batch with ope_corr_sac_pose_batch as its coarse stage (params->coarse is its front; corr_sac NULL: the defaults;
 * seeds as above).  out[i].coarse: T = T_svd, best_error = 0 (the pipeline has no error metric), best_iteration = best, the key
 * counts, status OPE_COARSE_OK for every cluster that reached the matcher, with or without a model (a counted coarse call);
 * out[i].seed the seed used.  Everything after the coarse stage, *selected and the refusals are ope_final_pose_batch's. */
int ope_final_pose_batch_correspondences(ope_ctx *ctx, const ope_cloud *model, size_t n, const ope_cloud *const *clusters,
                                         const ope_final_params *params, const ope_corr_sac_params *corr_sac, const uint64_t *seeds,
                                         ope_final_batch_result *out, int32_t *selected);

/* ---------------- tracking: the reference's later frames ---------------- */
/* Every frame after the first (rosinterface.cpp:264-313): the centroid of each cluster and of the source (the model as the
 * previous frame aligned it) by pcl::compute3DCentroid, the first non-empty cluster within gate_distance gets
 * estimateFinalPose(source, cluster); when none did and the LAST distance computed exceeds gate_distance, the candidate loop
 * runs again from the original model. */
enum {
  OPE_TRACK_NO_CLUSTERS = 0,  /* no clusters: nothing runs */
  OPE_TRACK_GATED = 1,        /* gate.selected is the first non-empty cluster with distance < gate_distance */
  OPE_TRACK_REALIGN_ALL = 2,  /* no cluster gated and the last distance > gate_distance: the candidate loop from the model */
  OPE_TRACK_NOTHING = 3,      /* no cluster gated and the last distance <= gate_distance (an empty last cluster, say): nothing */
  OPE_TRACK_REALIGN_LOOP = 4  /* ope_track_pose only: REALIGN_ALL with fitness_fine <= coarse_fitness on entry, so the loop's
                                 coarse stages would be skipped; nothing ran and the caller runs the loop one call at a time */
};
#define OPE_TRACK_COARSE_SKIPPED (-1) /* ope_track_result.coarse_status: fitness_fine <= coarse_fitness on entry */
typedef struct {
  double gate_distance;   /* 0.05: "distance < 0.05" (rosinterface.cpp:279), "distance > 0.05" (:304), float against double */
  double coarse_fitness;  /* 1e-4: the coarse stage runs while fitnessScoreFine > 1e-4 (poseestimator.cpp:399) */
  ope_final_params final; /* ope_final_default_params: the stages; accept_fitness 1e-4 / accept_strength 0.4 for the re-align */
} ope_track_params;
void ope_track_default_params(ope_track_params *p);
typedef struct {
  float centroid[3]; /* pcl::compute3DCentroid: the sequential float sum in the cloud's own order / count; 0 0 0 if count == 0 */
  int32_t count;     /* points summed: all of a cluster's (is_dense), the source's finite ones (!is_dense) */
  float distance;    /* (centroid - source centroid).lpNorm<2>() in float; 0 for the source itself */
} ope_track_centroid;
typedef struct {
  int32_t branch;     /* OPE_TRACK_* */
  int32_t selected;   /* the gated cluster, -1 unless GATED */
  ope_track_centroid source;
} ope_track_gate_result;
/* The gate alone, synchronous on the context's stream.  Three launches and one synchronisation whatever n is (none for n == 0:
 * NO_CLUSTERS).  centroids (n, may be NULL): each cluster's centroid, count and distance.  Clouds of any size. */
int ope_track_gate(ope_ctx *ctx, const ope_cloud *source, size_t n, const ope_cloud *const *clusters, const ope_track_params *params,
                   ope_track_gate_result *out, ope_track_centroid *centroids);

typedef struct {
  ope_track_gate_result gate; /* the branch taken (REALIGN_LOOP included) */
  int32_t selected;           /* GATED: the gated cluster; REALIGN_ALL: ope_final_pose_batch's selected; -1 otherwise */
  int32_t coarse_status;      /* GATED: OPE_COARSE_* of the coarse stage, or OPE_TRACK_COARSE_SKIPPED */
  uint64_t seed;              /* GATED: the SAC-IA stream it drew with (0: SAC-IA did not run) */
  float coarse[16];           /* GATED, column-major: coarsePose, finePose, rigidmodelPose and finalPose = rigid * (coarse * fine) */
  float fine[16];
  float rigid[16];
  float final_pose[16];
  ope_icp_result icp;         /* GATED: the fine ICP (iterations, align_strength, ...); zeros without ICP */
  double fitness;             /* GATED: getFitnessScore(final.fitness_max_range) of the fine pose; DBL_MAX without ICP */
  int64_t fitness_n;
  int32_t n_fine_src;         /* GATED: fine key points of the (moved) source and of the cluster */
  int32_t n_fine_tgt;
  int32_t status;             /* GATED: OPE_FINAL_* (OPE_FINAL_OK when the coarse stage was skipped and ICP ran) */
  int32_t reserved;
} ope_track_result;
/* One later frame of the reference, synchronous on the context's stream.  model = the original model (the estimator's cloudModel),
 * source = cloudSource (the model as the previous frame aligned it), fitness_fine / coarse_calls = the estimator's
 * fitnessScoreFine and SAC-IA calls so far (the k-th call draws with final.coarse.sacia.seed + k).
 *   GATED: estimateFinalPose(source, cluster): the coarse stage of ope_coarse_pose_batch when fitness_fine > coarse_fitness, the
 *          fine preparation of ope_final_pose_batch (the source as it is when the coarse stage is skipped), the single-problem ICP
 *          of ope_icp_run with getFitnessScore, the re-anchoring SVD fit of model to source over identity pairs; *aligned = a new
 *          cloud (free it with ope_cloud_free): the source moved by the coarse, then the fine pose (pcl::transformPointCloud's
 *          float arithmetic), the next frame's source.
 *   REALIGN_ALL: ope_final_pose_batch(model, clusters) with the estimator's seeds; realign (n) receives its results.
 *   REALIGN_LOOP, NOTHING, NO_CLUSTERS: nothing beyond the gate runs.
 * centroids (n) may be NULL; realign is required for n > 0.  OPE_EINVAL, nothing launched: what ope_final_pose_batch refuses for
 * (model, clusters) and, with fitness_fine > coarse_fitness, what the coarse stage refuses for (source, clusters); a model or
 * source of more than OPE_COARSE_MAX_POINTS points. */
int ope_track_pose(ope_ctx *ctx, const ope_cloud *model, const ope_cloud *source, double fitness_fine, int64_t coarse_calls, size_t n,
                   const ope_cloud *const *clusters, const ope_track_params *params, ope_track_result *out, ope_track_centroid *centroids,
                   ope_final_batch_result *realign, ope_cloud **aligned);

/* ---------------- segmentation: Euclidean cluster extraction ---------------- */
/* ObjectSegmentationPlane::getClusters (DetectAndLocalize/src/objectsegmentationplane.cpp:79-93): pcl::EuclideanClusterExtraction
 * of the non-plane cloud, the cloudClusterVector rosinterface.cpp:243-320 loops over. */
typedef struct {
  double tolerance; /* setClusterTolerance: 0.05 (objectsegmentationplane.cpp:85) */
  int32_t min_size; /* setMinClusterSize: 300 (:86) */
  int32_t max_size; /* setMaxClusterSize(1e5): 100000 (:87) */
} ope_cluster_params;
void ope_cluster_default_params(ope_cluster_params *p);
/* What EuclideanClusterExtraction::extract returns (PCL 1.7/1.8 extract_clusters.hpp): the connected components of the graph
 * that joins two finite points iff d2 <= r2, with d2 = (dx*dx + dy*dy) + dz*dz in float (FLANN's order, no contraction) and
 * r2 = (float)((double)(float)tolerance * (double)(float)tolerance) (PCL casts the tolerance to float, KdTreeFLANN squares it
 * in double).
 *  - a non-finite point is a component of its own (PCL's tree does not hold it): kept only when min_size <= 1;
 *  - a component with fewer than min_size or more than max_size points is dropped whole;
 *  - the points of a cluster are ORIGINAL indices, ascending;
 *  - clusters come by size, descending, then by their smallest index, ascending.  This is PCL's order (std::sort of
 *    comparePointClusters over reverse iterators) for up to 16 clusters, where libstdc++'s insertion sort is stable; beyond 16,
 *    PCL's order among equal sizes is implementation-defined and this rule is kept;
 *  - unlike PCL, two exact duplicates with no other neighbour are one cluster (PCL's search skips the first sorted radius
 *    result as if it were the query, so such a pair can come out as two singletons).
 * *n_clusters = the full count; the first min(count, max_clusters) clusters are written: cluster k is
 * out_idx[out_offsets[k] .. out_offsets[k + 1]) (out_idx: room for every point; out_offsets: max_clusters + 1).  out_label
 * (optional, n, ORIGINAL order): the rank of the written cluster holding the point, -1 for every other point.
 * Synchronous; kernel launches and host synchronisations do not depend on the number of clusters (one synchronisation).
 * An empty cloud gives 0 clusters.  OPE_EINVAL, nothing launched: tolerance <= 0 (or not finite), min_size < 1,
 * max_size < min_size, more than 2^31 - 1 points.  OPE_ERANGE, nothing launched: a cloud whose grid of cells of edge
 * 0.999 x tolerance / sqrt(3) over its finite points would have 2^36 cells or more along one axis (40 000 km at a 1 mm
 * tolerance) or 2^62 or more in all (a cube of 960 m at 1 mm); grids of more than 2^32 cells are fine. */
int ope_euclidean_clusters(ope_ctx *ctx, const ope_cloud *cloud, const ope_cluster_params *params, size_t max_clusters, size_t *n_clusters,
                           int32_t *out_idx, int32_t *out_offsets, int32_t *out_label);
/* The same, with each written cluster also as a new device cloud: out_clouds[k] is exactly what ope_cloud_select(cloud,
 * indices of cluster k) builds (its original order the cluster's ascending indices, normals carried, the Morton order of
 * ope_cloud_upload over its own box), made for all clusters at once in batched launches; free each with ope_cloud_free.
 * out_clouds: max_clusters entries; out_idx / out_offsets optional (as above).  Two synchronisations. */
int ope_euclidean_clusters_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_cluster_params *params, size_t max_clusters, size_t *n_clusters,
                                 ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets);
/* What the last ope_euclidean_clusters* call of this context did: kernel launches enqueued (a rocPRIM sort or scan counts as
 * one), host synchronisations, occupied grid cells, and cell pairs whose points were compared. */
typedef struct {
  int64_t launches;
  int64_t host_syncs;
  int64_t cells;
  int64_t pairs_tested;
} ope_cluster_stats;
int ope_cluster_last_stats(const ope_ctx *ctx, ope_cluster_stats *out);

/* ---------------- segmentation: smoothness-constrained region growing ---------------- */
/* SegmentationRegionGrow::getSegmentRegGrow (segmentationregiongrow.cpp:9-82): pcl::RegionGrowing over normals, the reference's
 * answer to a frame without a table whose objects no plane model separates. */
typedef struct {
  int32_t number_of_neighbours;   /* setNumberOfNeighbours: 15 (segmentationregiongrow.cpp:31) */
  int32_t normals_k;              /* setKSearch of the NormalEstimation: 30 (:25); used only when no normals are passed */
  double smoothness_threshold;    /* setSmoothnessThreshold: 10.0 / 180.0 * M_PI (:35) */
  double curvature_threshold;     /* setCurvatureThreshold: 1.0 (:36) */
  int32_t min_size, max_size;     /* setMinClusterSize / setMaxClusterSize: 500, 1000000 (:28-29) */
} ope_region_params;
void ope_region_default_params(ope_region_params *p);
/* What RegionGrowing::extract returns (PCL 1.7/1.8 region_growing.hpp, smooth mode, residual test off) while no curvature exceeds
 * the threshold, restated so that it runs in parallel:
 *   N(u) = the number_of_neighbours nearest finite points of u, u included: the list ope_knn_search returns;
 *   u -> v  iff  v is in N(u) and !(fabsf(n_v . n_u) < c), the dot product (x*x' + y*y') + z*z' in float without contraction and
 *            c = (float)cos((double)(float)smoothness_threshold); a NaN product is not < c: a NaN normal passes, as in PCL;
 *   rank: by curvature ascending, equal curvatures by ORIGINAL index ascending (PCL's std::sort leaves that order
 *            implementation-defined), a NaN curvature after every other;
 *   region(v) = the point of smallest rank among those that reach v along the edges, v included: PCL's sequential flood from
 *            the lowest-ranked unlabelled seed, which with the reference's threshold (1.0 >= every curvature) refuses no seed.
 *  - a non-finite point is in no region;
 *  - a region with fewer than min_size or more than max_size points is dropped whole;
 *  - regions come in seed order (the rank of their seed), NOT by size; the points of a region are ORIGINAL indices, ascending.
 * normals (n x 3) / curvature (n): host arrays in ORIGINAL order, both or neither.  Passed: used as given (setInputNormals), the
 * cloud's own are left alone.  Neither: the call runs ope_normals(cloud, normals_k, viewpoint 0 0 0) and leaves its result attached
 * to the cloud, as that call does.
 * *n_clusters, out_idx, out_offsets, out_label: the conventions of ope_euclidean_clusters.  An empty cloud gives 0 clusters.
 * A point with curvature > (float)curvature_threshold makes PCL's flood depend on which points end up as seeds; that rule is not
 * built: the call counts such points in the launch that reads the curvatures and, if there is one, returns OPE_EINVAL with
 * *n_clusters = 0 and out_idx, out_offsets, out_label (and out_clouds) untouched.
 * OPE_EINVAL, nothing launched: number_of_neighbours outside 1..32; normals_k outside 3..32 when no normals are passed; a threshold
 * that is not finite or a negative smoothness_threshold; min_size < 1; max_size < min_size; only one of normals / curvature;
 * more than (2^31 - 1) / 32 points.
 * Synchronous.  Kernel launches booked: 19 + 5 per batch of four propagation sweeps (batches go out until a sweep changes nothing),
 * + 1 with normals passed in; host synchronisations: 2 + 1 per batch (+ the staged upload of passed normals).  Not booked: the
 * build of the cloud's own search tree and, when the call estimates the normals, ope_normals with its one synchronisation.
 * Neither count depends on the number of regions. */
int ope_region_grow(ope_ctx *ctx, ope_cloud *cloud, const ope_region_params *params, const float *normals, const float *curvature,
                    size_t max_clusters, size_t *n_clusters, int32_t *out_idx, int32_t *out_offsets, int32_t *out_label);
/* The same, with each written region also as a new device cloud, exactly what ope_cloud_select(cloud, indices of region k)
 * builds, normals (the cloud's own) and colours carried: the batched path of ope_euclidean_clusters_cloud (4 more launches, one
 * more synchronisation).  out_clouds: max_clusters entries; out_idx / out_offsets optional. */
int ope_region_grow_cloud(ope_ctx *ctx, ope_cloud *cloud, const ope_region_params *params, const float *normals, const float *curvature,
                          size_t max_clusters, size_t *n_clusters, ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets);
/* What the last ope_region_grow* call of this context did. */
typedef struct {
  int64_t launches;                    /* kernel launches enqueued (a rocPRIM sort or scan, a memset and a copy count as one) */
  int64_t host_syncs;
  int64_t sweeps;                      /* propagation rounds until one changed nothing (that one included) */
  int64_t one_way_edges;               /* edges u -> v without v -> u */
  int64_t regions_before_size_filter;
  int64_t refused_curvature;           /* points with curvature > curvature_threshold (non-zero: the call was refused) */
} ope_region_stats;
int ope_region_last_stats(const ope_ctx *ctx, ope_region_stats *out);

/* ---------------- segmentation: colour-based region growing ---------------- */
/* SegmentationRegionGrow::getSegmentRegGrowRgb (segmentationregiongrow.cpp:85-151): pcl::RegionGrowingRGB, the reference's answer to
 * objects that neither a plane nor surface normals separate from what they touch. */
typedef struct {
  int32_t region_neighbour_number;  /* PCL's region_neighbour_number_, which the reference never changes: 100; 1..128 */
  double distance_threshold;        /* setDistanceThreshold (0.1) (segmentationregiongrow.cpp:100) */
  double point_color_threshold;     /* setPointColorThreshold (10) (:101) */
  double region_color_threshold;    /* setRegionColorThreshold (10) (:102) */
  int32_t min_size, max_size;       /* setMinClusterSize (700) (:103); PCL's default maximum, INT32_MAX */
} ope_region_rgb_params;
void ope_region_rgb_default_params(ope_region_rgb_params *p);
/* What RegionGrowingRGB::extract returns (PCL 1.7/1.8 region_growing_rgb.hpp; normal, curvature and residual tests off, as its
 * constructor leaves them) for a cloud with colours (ope_cloud_set_rgb).  With K = region_neighbour_number, N(u) the K nearest finite
 * points of u (u included), cd the sum of the squared channel differences, and every threshold squared in float:
 *  - point edges u -> v iff v is in N(u), v != u and !(cd(u, v) > point_color_threshold^2); segment(v) = the smallest ORIGINAL index
 *    among the points that reach v, v included; segments are numbered by seed;
 *  - a segment's colour is the truncated float mean of each channel; its neighbours are the K segments t nearest by
 *    (min d2 over its own points' lists, t);
 *  - merge A joins a segment to the first earlier segment that keeps it within distance_threshold^2 and whose colour differs by
 *    less than region_color_threshold^2; merge B moves every region below min_size into the region of its nearest neighbour, in
 *    order; regions are reordered by PCL's two-pointer pass over the empty ones, and those outside min_size..max_size are dropped.
 * DESIGN.md 4.19 has the whole restatement.  A non-finite point is in no region.  out_idx, out_offsets, out_label, *n_clusters and
 * max_clusters as ope_euclidean_clusters.  OPE_EINVAL, nothing launched: a cloud without colours, region_neighbour_number outside
 * 1..128, a threshold that is negative or not finite, min_size < 1, max_size < min_size, more than (2^31 - 1) / 128 points.  An
 * empty cloud gives 0 clusters.
 * Kernel launches booked: 27 + 5 per batch of four sweeps (+ 5 for the _cloud form); host synchronisations: 4 + 1 per batch (+ 1
 * for the _cloud form).  Neither count depends on the number of points, segments or regions. */
int ope_region_grow_rgb(ope_ctx *ctx, const ope_cloud *cloud, const ope_region_rgb_params *params, size_t max_clusters, size_t *n_clusters,
                        int32_t *out_idx, int32_t *out_offsets, int32_t *out_label);
/* The same, with each written region also as a new device cloud, exactly what ope_cloud_select(cloud, indices of region k)
 * builds (colours and normals carried); the caller frees them.  out_idx / out_offsets are optional here. */
int ope_region_grow_rgb_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_region_rgb_params *params, size_t max_clusters, size_t *n_clusters,
                              ope_cloud **out_clouds, int32_t *out_idx, int32_t *out_offsets);
/* What the last ope_region_grow_rgb* call of this context did. */
typedef struct {
  int64_t launches;
  int64_t host_syncs;
  int64_t sweeps;
  int64_t one_way_edges;
  int64_t segments;                    /* S */
  int64_t segment_pairs;               /* directed pairs (s, t) with a distance, before the cut to the K nearest */
  int64_t homogeneous_regions;         /* H, after merge A */
  int64_t regions_absorbed;            /* merge B */
  int64_t regions_before_size_filter;  /* non-empty regions after merge B */
} ope_region_rgb_stats;
int ope_region_rgb_last_stats(const ope_ctx *ctx, ope_region_rgb_stats *out);

/* ---------------- segmentation: RANSAC plane fit, polygonal prism, table-top ---------------- */
/* pcl::SACSegmentation with SACMODEL_PLANE, SAC_RANSAC (getPlaneIndicesAndCoeffSAC, objectsegmentationplane.cpp:36-55).
 * The reference also calls setAxis / setEpsAngle (:44-45); they have no effect on SACMODEL_PLANE in PCL (only the
 * PERPENDICULAR / PARALLEL plane models read them) and have no parameter here. */
typedef struct {
  double distance_threshold;      /* 0.01 (objectsegmentationplane.cpp:43) */
  double probability;             /* 0.99 (SACSegmentation's default) */
  int32_t max_iterations;         /* 50 (SACSegmentation's default); at most OPE_PLANE_MAX_ITERATIONS */
  int32_t optimize_coefficients;  /* 1 (:39) */
  uint64_t seed;                  /* 12345: std::mt19937's seed in PCL when `random` is false */
} ope_plane_params;
#define OPE_PLANE_MAX_ITERATIONS 1023
void ope_plane_default_params(ope_plane_params *p);
/* What the last ope_plane_segment of this context did (for ope_tabletop_segment: its SECOND fit, with the launches and
 * synchronisations of the whole call). */
typedef struct {
  int64_t iterations;   /* iterations RandomSampleConsensus::computeModel would have run */
  int64_t hypotheses;   /* hypotheses drawn and scored (max_iterations + 1 unless the draws ran dry) */
  int64_t launches;     /* kernel launches enqueued (a rocPRIM scan counts as one) */
  int64_t host_syncs;
  int32_t best;         /* the winning hypothesis, -1 without a model */
  int32_t found;        /* 1: a model was found; 0: none (the façade leaves ModelCoefficients::values empty) */
} ope_plane_stats;
/* The plane of a cloud: every one of the max_iterations + 1 samples RANSAC can reach is drawn on the device
 * (SampleConsensusModel::drawIndexSample over ALL points in ORIGINAL order, isSampleGood, computeModelCoefficients), all
 * are scored in ONE pass over the cloud (countWithinDistance), the counts come back and the loop of
 * RandomSampleConsensus::computeModel is replayed on the host; then selectWithinDistance, optimizeModelCoefficients
 * (optimize_coefficients) and selectWithinDistance again.  DESIGN 4.11 has the float order of every step.
 *   samples (optional, n_samples triples of ORIGINAL indices): taken instead of the draws, unchecked, n_samples <= max_iterations + 1;
 *   coeff: a b c d;  out_idx (room for every point) / *n_inliers: the inliers, ORIGINAL indices ascending;
 *   plane / not_plane (optional): new device clouds, exactly ope_cloud_select(cloud, inliers) and ope_cloud_select(cloud, the
 *   other indices, ascending) (ExtractIndices, negative false / true).
 * No model (fewer than 3 points, or no good sample): OPE_OK, *n_inliers = 0, coeff untouched, stats.found = 0, the clouds as
 * for an empty inlier list.  Launches and synchronisations do not depend on the number of points or of iterations.
 * out_idx is written as one copy of the whole index buffer, before the host knows the count: its entries from *n_inliers on
 * are unspecified (the same holds for every index output of ope_prism_extract and ope_tabletop_segment past its count).
 * In the stats a cloud selection (each output cloud, and the prism's cloud inside ope_tabletop_segment) is BOOKED as 4 launches
 * and 1 synchronisation (2 when the cloud carries normals), not counted: it is ope_cloud_select's device path, whose launches
 * depend on neither the points nor the iterations either (an empty selection launches nothing and is booked all the same). */
int ope_plane_segment(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *params, const int32_t *samples, size_t n_samples,
                      float coeff[4], int32_t *out_idx, size_t *n_inliers, ope_cloud **plane, ope_cloud **not_plane);
int ope_plane_last_stats(const ope_ctx *ctx, ope_plane_stats *out);
/* The hypotheses of the last ope_plane_segment: samples (3 ORIGINAL indices each), coefficients (4 floats each) and inlier
 * counts, in drawing order; any output may be NULL; at most cap are written, *n_out = how many there were. */
int ope_plane_last_hypotheses(const ope_ctx *ctx, int32_t *samples, float *coeffs, int32_t *counts, size_t cap, size_t *n_out);

/* pcl::ExtractPolygonalPrismData::segment with PCL's defaults (height limits 0 .. FLT_MAX unless given, viewpoint 0 0 0): the
 * plane of the hull's m >= 3 vertices (computeMeanAndCovarianceMatrix, eigen33, flipped towards the viewpoint and then
 * re-anchored on vertex 0), and per point the signed distance against the limits, the projection into that plane and the
 * crossing test against the hull with the normal's dominant axis dropped.  hull: m x 3 floats (host).
 * out_idx (optional, room for every point) / *n_out: the survivors, ORIGINAL indices ascending; out (optional): the survivors
 * as ope_cloud_select builds them.  hull_coeff (optional): the hull's plane. */
int ope_prism_extract(ope_ctx *ctx, const ope_cloud *cloud, const float *hull, size_t m, double height_min, double height_max,
                      int32_t *out_idx, size_t *n_out, ope_cloud **out, float hull_coeff[4]);

enum {
  OPE_TABLETOP_OK = 0,
  OPE_TABLETOP_NO_PLANE_FIRST = 1,    /* the first fit found no model (objectsegmentationplane.cpp:156-159: false, the input back) */
  OPE_TABLETOP_NO_PLANE_SECOND = 2    /* the fit on the prism's points found none (:229-232) */
};
typedef struct {
  int32_t status;
  int32_t n_prism;            /* points inside the prism (cloudObjWithPlane) */
  int32_t n_plane, n_not_plane;
  float coeff_first[4];       /* the first fit */
  float coeff_second[4];      /* the fit on the prism's points */
  float corners[12];          /* the four hull corners, x y z each (:174-188) */
  int64_t iterations_first, iterations_second;
  int64_t launches, host_syncs;
} ope_tabletop_result;
/* getSegmentedObjectsOnPlane up to getClusters (objectsegmentationplane.cpp:124-235): plane fit, the inliers projected
 * into it and their extreme x and y (what getMinMax3D of their convex hull returns), the four corners, the prism, the plane fit
 * of the prism's points (re-indexed in ascending order, the same seed), plane and non-plane cloud.
 * plane / not_plane (required): new device clouds (NULL unless the status is OK);  prism_idx (optional, room for every point):
 * the prism's points as indices into `cloud`;  plane_idx / not_plane_idx (optional, room for every point): both clouds' points
 * as indices into `cloud`.  Launches and synchronisations do not depend on the number of points or of iterations. */
int ope_tabletop_segment(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *params, ope_tabletop_result *out,
                         ope_cloud **plane, ope_cloud **not_plane, int32_t *prism_idx, int32_t *plane_idx, int32_t *not_plane_idx);

/* ObjectSegmentationPlane::getSegmentedObjectsExceptPlane between its crop and getClusters (objectsegmentationplane.cpp:296-319):
 * the dominant plane is fitted and its inliers removed, over and over, until at most keep_fraction of the input's points are left.
 *     m = n0 = the cloud's points (non-finite ones included)
 *     while ((double)m > keep_fraction * (double)n0) {      the test is made BEFORE each fit
 *       [max_planes > 0 and that many planes peeled: stop OPE_PEEL_MAX_PLANES]
 *       a fresh ope_plane_segment fit of the remainder, re-indexed 0..m-1 in ascending original order, the same parameters and seed
 *       no model, or a model without inliers: stop OPE_PEEL_NO_INLIERS
 *       the remainder loses the inliers (ExtractIndices negative, order kept) }
 * The rounds run on one packed point array that shrinks in place of a cloud per plane; one cloud is built, at the end. */
typedef struct {
  double keep_fraction;   /* 0.3 (objectsegmentationplane.cpp:300) */
  int32_t max_planes;     /* 0: no cap, as the reference; > 0: stop after that many planes */
} ope_peel_params;
void ope_peel_default_params(ope_peel_params *p);
enum { OPE_PEEL_FRACTION = 0, OPE_PEEL_NO_INLIERS = 1, OPE_PEEL_MAX_PLANES = 2 };
typedef struct {
  int32_t n_planes;       /* planes peeled (all of them, also beyond cap_planes) */
  int32_t n_rest;         /* points of the remainder */
  int32_t stop;           /* OPE_PEEL_*: why the loop ended (the fraction test comes first: it wins over the cap) */
  int64_t launches, host_syncs;
} ope_peel_result;
/*   plane / peel: NULL takes the defaults;
 *   coeffs (4 floats per plane), counts (inliers per plane), iterations (RANSAC iterations per plane): each optional, written
 *   for the first min(n_planes, cap_planes) planes;
 *   label (optional, one entry per point, ORIGINAL order): the round that took the point, -1 for the remainder;
 *   rest_idx (optional, room for every point): the remainder as ORIGINAL indices of `cloud`, ascending; entries past n_rest are
 *   unspecified;  rest (optional): a new device cloud, exactly ope_cloud_select(cloud, rest_idx[0 .. n_rest)), colours and normals
 *   carried, built once from the input cloud and booked as every selection of this section.
 * OPE_EINVAL, nothing launched: what ope_plane_segment refuses of `plane`, keep_fraction negative or not finite, max_planes < 0,
 * more than 2^31 - 1 points.  An empty cloud: 0 planes, OPE_PEEL_FRACTION, an empty remainder.
 * Per peeled plane the call enqueues a fixed number of launches and synchronises twice; neither depends on the points or on the
 * iterations.  ope_plane_last_stats / ope_plane_last_hypotheses describe the LAST fit of the call (indices of its remainder). */
int ope_plane_peel(ope_ctx *ctx, const ope_cloud *cloud, const ope_plane_params *plane, const ope_peel_params *peel, size_t cap_planes,
                   float *coeffs, int32_t *counts, int64_t *iterations, int32_t *label, int32_t *rest_idx, ope_cloud **rest,
                   ope_peel_result *out);

/* ---------------- ingest: the sensor's depth image -> the frame's cloud ---------------- */
/* DataGrabber::rgbd2Pcl (DetectAndLocalize/src/datagrabber.cpp:65-118, called once per frame at rosinterface.cpp:422) with
 * depthToMeter (:121-174), optionally followed by getPassThrough (rosinterface.cpp:212), on the device: the caller hands over
 * the 16-bit depth image and receives the cloud the later stages consume; no host cloud of the frame is built or uploaded.
 *
 * Arithmetic (all float, each operation rounded once, no contraction; division correctly rounded), datagrabber.cpp:169-171:
 *     Z = (float)depth / scale
 *     y = ((row - c_row) * Z) / f_row
 *     x = ((col - c_col) * Z) / f_col
 * A pixel is dropped iff depth == 0 (:127,142,155 with :90) or (double)Z > z_max (:90, "Z > 2.0": float against double).
 *
 * THE REFERENCE'S QUIRK.  rgbd2Pcl passes the ROW as p_FeatX and the COLUMN as p_FeatY (:86), depthToMeter applies cx / fx to
 * p_FeatX and cy / fy to p_FeatY (:170-171), and rgbd2Pcl stores X into .y and Y into .x (:98-99).  So the reference's cx / fx
 * act on the row and its cy / fy on the column: for the Kinect preset c_row = 319.5, f_row = 525, c_col = 239.5, f_col = 525 —
 * the principal point is swapped against the image's axes.  ope_depth_sensor_params reproduces this, because the rest of the
 * reference (the workspace limits, the model) was tuned on clouds made this way.  A caller with a correctly calibrated sensor
 * fills the struct itself: the names below say what each value multiplies. */
typedef struct {
  float f_row, c_row;   /* y = (row - c_row) * Z / f_row */
  float f_col, c_col;   /* x = (col - c_col) * Z / f_col */
  float scale;          /* Z = (float)depth / scale; 1000 (:137,150,163) */
  double z_max;         /* a pixel is dropped iff depth == 0 or (double)Z > z_max; 2.0 (:90) */
} ope_depth_params;
enum { OPE_SENSOR_KINECT = 0, OPE_SENSOR_ASTRA = 1, OPE_SENSOR_EUCLID = 2 };
/* The reference's three intrinsics sets (fx fy cx cy as float, scale 1000, z_max 2.0):
 *   Euclid 306.178 306.929 158.523 122.747 (:133-137), Kinect 525 525 319.5 239.5 (:146-150), Astra 570.342 570.342 314.5 235.5
 *   (:159-163), with f_row = fx, c_row = cx, f_col = fy, c_col = cy (the quirk above).  OPE_EINVAL for another sensor. */
int ope_depth_sensor_params(int sensor, ope_depth_params *p);
/* depth: rows x cols samples, row r at (const char *)depth + r * row_stride_bytes (cv::Mat::step).
 * lo / hi: both NULL for no crop; otherwise a point also has to satisfy lo[d] <= p[d] <= hi[d] for d = x, y, z
 * (ope_pass_through's rule), and *out is exactly the cloud ope_pass_through_cloud(uncropped cloud, lo, hi) builds.
 * *out (free it with ope_cloud_free): the surviving pixels in the reference's loop order, COLUMNS OUTER, ROWS INNER (:77-79) — the
 * ORIGINAL order of the cloud — and otherwise what ope_cloud_upload of the reference's host cloud would build: same points,
 * same bounding box, same Morton order.  out_pixel (optional, room for rows * cols): out_pixel[k] = row * cols + col of
 * point k, for a caller that gathers colours (the overload of :9-62); *n_out (optional) the number of points.  An image with
 * no surviving pixel gives an empty cloud and OPE_OK.
 * Synchronous on the context's stream.  The image travels as 2 bytes per pixel; a workgroup transposes a 64 x 64 tile
 * through LDS, a count pass and one scan place every (column, 64-row) segment, a second pass writes the points, their pixel
 * indices and the bounding box.  The sequence of launches and host synchronisations is fixed for an image of up to 32 MB (the
 * pinned staging block): it depends on neither the content nor the size.  A larger image travels in blocks, one more copy and
 * one more synchronisation per block.
 * OPE_EINVAL, nothing launched: a NULL ctx, depth, params or out; rows * cols == 0 or > 2^31 - 1; row_stride_bytes < 2 * cols
 * or odd; scale, f_row or f_col not positive and finite; c_row or c_col not finite (no point would be finite, where the
 * cloud of an upload has n_valid == n); one image row, padded to a multiple of 64 samples, above 32 MB; exactly one of lo / hi. */
int ope_depth_to_cloud(ope_ctx *ctx, const uint16_t *depth, size_t rows, size_t cols, size_t row_stride_bytes,
                       const ope_depth_params *params, const float lo[3], const float hi[3], ope_cloud **out, int32_t *out_pixel,
                       size_t *n_out);
/* rgbd2Pcl(p_imageRgb, p_imageDepth), the two-image overload (BuildModel/src/datagrabber.cpp:9-64): ope_depth_to_cloud of `depth`
 * — geometry, drop rule, order, crop, bounding box and Morton order bit for bit — whose point k also carries
 * r << 16 | g << 8 | b of its pixel as the cloud's colour payload (ope_cloud_download_rgb), where b, g, r are bytes 0, 1, 2 of
 * pixel (row, col) of a CV_8UC3 image (:48-51): pixel (r, c) at bgr + r * bgr_stride_bytes + 3 * c.  The top byte is 0.  The
 * cloud has colours also when it is empty.
 * The colour image travels as 3 bytes per pixel in the same pinned block and the same copy as the depth image (a staged row is
 * the depth row followed by its colour row, 5 bytes per padded pixel); the second pass reads a tile's 64 x 64 pixels as 16-byte
 * loads, transposes them through LDS beside the depth tile (12 KB) and writes the colour word with the point; the Morton
 * ordering's gather moves it with the point.  Launches and synchronisations are those of ope_depth_to_cloud, one for one,
 * whatever the images hold and, up to 32 MB of staged rows (6.7 M pixels), whatever their size; above, depth and colour travel
 * together in blocks of whole rows, one more copy and one more synchronisation per block.  ope_depth_last_stats reports the call.
 * OPE_EINVAL, nothing launched: the cases of ope_depth_to_cloud (one padded row here at 5 bytes per pixel); bgr NULL;
 * bgr_stride_bytes < 3 * cols. */
int ope_depth_to_cloud_rgb(ope_ctx *ctx, const uint16_t *depth, size_t rows, size_t cols, size_t depth_stride_bytes,
                           const unsigned char *bgr, size_t bgr_stride_bytes, const ope_depth_params *params, const float lo[3],
                           const float hi[3], ope_cloud **out, int32_t *out_pixel, size_t *n_out);
/* What the last ope_depth_to_cloud or ope_depth_to_cloud_rgb of this context did.  launches and host_syncs are BOOKED along the call's fixed path, not
 * observed from the runtime: one per kernel, copy or rocPRIM call this function enqueues (a rocPRIM call counts as one, however
 * many kernels it issues inside) and one per stream synchronisation.  The Morton ordering of the new cloud is booked as 3
 * launches and 1 synchronisation, for an empty cloud too, which orders nothing; the copy of out_pixel as 1 when asked for.
 * They say that the call has no loop over the content; for what really ran, take a kernel trace. */
typedef struct {
  int64_t launches;
  int64_t host_syncs;
  int64_t pixels;   /* rows * cols */
  int64_t valid;    /* pixels with depth != 0 and Z <= z_max */
  int64_t kept;     /* points of the cloud (valid and inside the crop) */
} ope_depth_stats;
int ope_depth_last_stats(const ope_ctx *ctx, ope_depth_stats *out);

/* ---------------- moving least squares (ProcessingPcd::getSmooth) ---------------- */
/* pcl::MovingLeastSquares::process with upsampling NONE (BuildModel/src/processingpcd.cpp:80-108: polynomial fit, radius search,
 * normals off; regmeshpcd.cpp:264-266 with radius 0.02), DESIGN.md 4.14.  For every finite input point q, in ascending ORIGINAL
 * index: its neighbours are the finite points p of the same cloud with fp32 ((dx*dx + dy*dy) + dz*dz) <= (float)radius *
 * (float)radius, q included, however many.  Fewer than 3: q is DROPPED.  Otherwise, in fp64: centroid, unnormalised covariance,
 * pcl::eigen33's smallest eigenpair (n, lambda), the plane through the centroid, q projected on it, curvature
 * |lambda / trace| (0 for a zero trace).  With polynomial_fit and at least (order + 1)(order + 2) / 2 neighbours: the weighted
 * least-squares polynomial of that order over the neighbours' plane coordinates about the projected point, weights
 * exp(-d^2 / sqr_gauss_param), solved by Cholesky; if c[0] is finite the point moves by c[0] n and, with compute_normals, the normal
 * becomes n - c[order + 1] u - c[1] v (neither normalised nor oriented); otherwise the projection and n stand.
 * Two deviations from PCL: non-finite input points are dropped and are nobody's neighbour (PCL's behaviour on them is undefined);
 * a Cholesky pivot that is <= 0 or not finite makes the fit fail like a non-finite c[0] (Eigen goes on with garbage).
 * radius > 0; order 0, 1 or 2 (3 and 4 belong to MLS upsampling: ope_mls_upsample below): anything else OPE_EINVAL, nothing launched.
 * sqr_gauss_param 0 means radius * radius, as setSearchRadius sets it. */
typedef struct {
  double radius;
  int polynomial_fit;       /* 1 */
  int order;                /* 2 */
  double sqr_gauss_param;   /* 0 */
  int compute_normals;      /* 0 */
} ope_mls_params;
void ope_mls_default_params(ope_mls_params *p);
/* Host outputs, each with room for ope_cloud_size(cloud) points; any may be NULL except n_out.  out_xyz: the smoothed points
 * (x y z); out_normals (x y z) and out_curvature: as above (the plane's normal when compute_normals is 0); out_idx: the ORIGINAL
 * index of each output point (getCorrespondingIndices), ascending.  An empty cloud gives OPE_OK and *n_out = 0. */
int ope_mls_smooth(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params *params, float *out_xyz, float *out_normals,
                   float *out_curvature, int32_t *out_idx, size_t *n_out);
/* The same with the result left on the device: *out is a new cloud of the smoothed points (free it with ope_cloud_free), the
 * input's colours carried (copyMissingFields) and, when compute_normals is set, the normals attached (w = curvature).  An empty
 * result is an empty cloud, coloured if the input was.  out_idx is optional. */
int ope_mls_smooth_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_params *params, ope_cloud **out, int32_t *out_idx,
                         size_t *n_out);
/* What the last ope_mls_smooth / ope_mls_smooth_cloud of this context did.  n_plane_only: output points that stand at their plane
 * projection (no fit asked for, too few neighbours for the order, or a failed fit); n_dropped = n_in - n_out; neighbours_total:
 * neighbourhood sizes summed over the finite input points, the dropped ones included. */
typedef struct {
  int64_t n_in, n_out, n_plane_only, n_dropped, neighbours_total;
} ope_mls_stats;
int ope_mls_last_stats(const ope_ctx *ctx, ope_mls_stats *out);

/* ---------------- moving least squares, upsampled (RegMeshPcd::generateMesh) ---------------- */
/* pcl::MovingLeastSquares::process with upsampling VOXEL_GRID_DILATION (BuildModel/src/regmeshpcd.cpp:275-292: order 4, radius 0.03,
 * voxel 0.002; PCL 1.7.x surface/impl/mls.hpp), DESIGN.md 4.15.  Nothing is produced per input point in this mode; instead:
 *  a. every finite input point with 3 or more neighbours (as for ope_mls_smooth) keeps its MLSResult: the query projected on its
 *     plane (mean), the plane's normal n, the axes v = unitOrthogonal(n) and u = n x v when polynomial_fit is set and it has at least
 *     nr_coeff = (order + 1)(order + 2) / 2 neighbours (both zero otherwise, as 1.7 leaves them), the Cholesky solution c, the
 *     neighbour count m and the curvature.  Points with fewer than 3 neighbours are invalid.
 *  b. MLSVoxelGrid: bmin / bmax the float box of the finite points; data_size = uint64(1.5 * max extent / voxel_size); per finite point
 *     cell = int((p - bmin) / voxel_size) in float; key = (cell0 * data_size + cell1) * data_size + cell2; the grid is the set of distinct
 *     keys in ascending order.  Each of dilation_iterations rounds replaces the set by the union of the 27 neighbours (itself
 *     included) of every voxel.  data_size 0 (all points within 2/3 of a voxel) decodes every key to cell (0, 0, 0).
 *  c. per voxel in key order: position = float(cell) * voxel_size + bmin (multiply, then add, in float); j = the nearest finite input
 *     point in fp32 ((dx*dx + dy*dy) + dz*dz); the voxel is skipped when j is invalid; u_disp, v_disp = the float dot products of
 *     (position - q_j) with j's axes cast to float; projectPointToMLSSurface: result = mean + u u_disp + v v_disp + n n_disp in
 *     double, cast to float, where n_disp is the polynomial of order `order` in (u_disp, v_disp) when polynomial_fit is set, j has at
 *     least 5 nr_coeff neighbours, the fit did not fail and c[0] is finite, and 0 otherwise; with compute_normals the normal is
 *     n - d_u u - d_v v normalised (d_u, d_v the polynomial's partial derivatives there), otherwise j's plane normal; the curvature
 *     is j's.  The voxel is skipped when the result lies farther from q_j than the voxel's position did (both distances in float).
 *     Survivors come out in key order; out_idx is j (getCorrespondingIndices), and the colour word is that of point j.
 * Three deviations from PCL: non-finite input points are dropped, are nobody's neighbour and nobody's nearest point; a Cholesky
 * pivot that is <= 0 or not finite makes the fit count as failed (Eigen goes on with garbage); a dilation neighbour with a cell
 * component outside [0, data_size) is dropped (PCL lets the unsigned key wrap).  Equal fp32 distances of the nearest search go to the
 * lowest original index (FLANN's choice there is implementation-defined).
 * radius > 0; order 0..4; voxel_size > 0 and finite; dilation_iterations 0..8; data_size <= 2^21: anything else OPE_EINVAL, nothing
 * launched.  sqr_gauss_param 0 means radius * radius.  The sequence of launches and host waits depends on the parameters only. */
typedef struct {
  double radius;
  int polynomial_fit;        /* 1 */
  int order;                 /* 2 (generateMesh: 4) */
  double sqr_gauss_param;    /* 0 */
  int compute_normals;       /* 0 */
  float voxel_size;          /* 1.0 (generateMesh: 0.002) */
  int dilation_iterations;   /* 0 */
} ope_mls_upsample_params;
void ope_mls_upsample_default_params(ope_mls_upsample_params *p);
/* Host outputs, each with room for `capacity` points; any may be NULL except n_out.  out_normals (x y z) and out_curvature as above.
 * The size of the result is not known beforehand: when it exceeds `capacity` (and an output array was given) nothing is copied,
 * the call returns OPE_EINVAL and *n_out is set to the size the arrays need, so that a second call with that capacity succeeds
 * (all arrays NULL and capacity 0 only count: OPE_OK).  An empty cloud gives OPE_OK and *n_out = 0. */
int ope_mls_upsample(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params *params, float *out_xyz, float *out_normals,
                     float *out_curvature, int32_t *out_idx, size_t capacity, size_t *n_out);
/* The same with the result left on the device: *out is a new cloud of the upsampled points, Morton-ordered like an upload (its
 * ORIGINAL order is the key order), with the colour word of point j for every output and, when compute_normals is set, the normals
 * attached (w = curvature).  out_idx (optional, room for `capacity`) is in key order; too small a capacity: as above. */
int ope_mls_upsample_cloud(ope_ctx *ctx, const ope_cloud *cloud, const ope_mls_upsample_params *params, ope_cloud **out, int32_t *out_idx,
                           size_t capacity, size_t *n_out);
/* What the last ope_mls_upsample / ope_mls_upsample_cloud of this context did.  n_valid: input points with an MLSResult; n_voxels:
 * the grid after the dilation; n_invalid_nearest: voxels skipped because their nearest point is invalid; n_polynomial: voxels (with
 * a valid nearest point) whose projection applied the polynomial; n_rejected_farther: voxels dropped by the keep rule; n_out =
 * n_voxels - n_invalid_nearest - n_rejected_farther.  launches and host_syncs are BOOKED along the call's fixed path, as for
 * ope_depth_last_stats (the temporary index build counts as one launch, a rocPRIM call as one). */
typedef struct {
  int64_t n_in, n_valid, n_voxels, n_invalid_nearest, n_polynomial, n_rejected_farther, n_out, data_size, launches, host_syncs;
} ope_mls_upsample_stats;
int ope_mls_upsample_last_stats(const ope_ctx *ctx, ope_mls_upsample_stats *out);

/* ---------------- recognition: Viewpoint Feature Histograms and chi-square matching ---------------- */
/* ObjectDetection (BuildModel/src/objectdetection.cpp): getVfhFeature computes k = 30 normals and one pcl::VFHEstimation signature
 * of 308 bins per cloud; getObjectName takes the 15 nearest rows of a table of trained signatures by chi-square distance.
 * The signature restates pcl::VFHEstimation::computeFeature of PCL 1.7.x with its defaults (normalize_bins_ on,
 * normalize_distances_ off, size_component_ off): bins [0, 45) f1, [45, 90) f2, [90, 135) f3, [135, 180) f4 (zero under the
 * defaults), [180, 308) the viewpoint component.  use_given_centroid / use_given_normal are setUseGivenCentroid /
 * setUseGivenNormal with setCentroidToUse / setNormalToUse; they apply to every cluster of the call. */
typedef struct {
  int32_t normals_k;           /* 30 (objectdetection.cpp:17): NormalEstimation of a cloud that carries no normals */
  float viewpoint[3];          /* 0 0 0 (setViewPoint) */
  int32_t use_given_centroid;  /* 0 */
  float centroid[3];
  int32_t use_given_normal;    /* 0 */
  float normal[3];
} ope_vfh_params;
void ope_vfh_default_params(ope_vfh_params *p);
/* One signature per cluster, all clusters in the same launches: out308 has n x 308 floats.  counts_opt (n x 308 int32): the hits of
 * every bin, whose replayed additions of hist_incr are the signature.  bins_opt (4 bytes per point, the clusters' points packed in
 * call order, each cluster in its ORIGINAL order): the f1, f2, f3 bins of the point's pair with the centroid (0xFF each when
 * computePairFeatures rejects the pair) and its viewpoint bin.
 * A cluster that carries normals is taken with them; one that does not gets ope_normals(normals_k, viewpoint 0 0 0), left attached.
 * An empty cluster gives a zero row (stats.empty_clouds).  OPE_EINVAL, nothing launched: n == 0, a NULL cluster, a cluster with a
 * non-finite point, normals attached with ope_cloud_set_normals that are not finite, normals_k outside 3..32, non-finite
 * parameters.  Normals written on the device (ope_normals, MLS) are checked in the first launch: OPE_EINVAL after the call's
 * synchronisation if one is not finite, the outputs then undefined.
 * Launches and host synchronisations do not depend on the number of clusters or their sizes (one synchronisation, at the end),
 * except: one ope_normals per cluster without normals, and one more wait when the cluster table exceeds 4 KiB (~100 clusters). */
int ope_vfh_batch(ope_ctx *ctx, size_t n, ope_cloud *const *clusters, const ope_vfh_params *params, float *out308, int32_t *counts_opt,
                  unsigned char *bins_opt);
/* What the last ope_vfh_batch / ope_vfh_match / ope_vfh_recognise of this context did. */
typedef struct {
  int64_t points;             /* of all clusters */
  int64_t rejected_pairs;     /* points whose pair with the centroid computePairFeatures rejected */
  int64_t normals_estimated;  /* clusters whose normals the call estimated */
  int64_t empty_clouds;
  int64_t launches;           /* kernels and memsets, booked along the call's path (ope_normals not included) */
  int64_t host_syncs;
} ope_vfh_stats;
int ope_vfh_last_stats(const ope_ctx *ctx, ope_vfh_stats *out);
/* A table of m trained signatures (rows: m x 308 finite floats), kept on the device.  OPE_EINVAL for m == 0. */
typedef struct ope_vfh_db ope_vfh_db;
int ope_vfh_db_create(ope_ctx *ctx, const float *rows, size_t m, ope_vfh_db **db);
void ope_vfh_db_free(ope_vfh_db *db);
size_t ope_vfh_db_size(const ope_vfh_db *db);
/* The k nearest rows of every query (q x 308 finite floats) by flann::ChiSquareDistance, fp32 in dimension order: out_idx /
 * out_dist are q x k, nearest first, equal distances by ascending row; past m: -1 / +inf.  1 <= k <= 16.  This is EXACT search:
 * the reference's KDTreeIndexParams(1) with 512 checks is FLANN's approximate search over a randomised tree. */
int ope_vfh_match(ope_ctx *ctx, const ope_vfh_db *db, const float *queries308, size_t q, int k, int32_t *out_idx, float *out_dist);
/* ope_vfh_batch followed by ope_vfh_match with the signatures never leaving the device; out308_opt: the signatures as well. */
int ope_vfh_recognise(ope_ctx *ctx, const ope_vfh_db *db, size_t n, ope_cloud *const *clusters, const ope_vfh_params *params, int k,
                      float *out308_opt, int32_t *out_idx, float *out_dist);

/* The batched entry points that take a list of global rejectors as an argument. */
#include "ope_batch_rejectors.h"
/* The draws of the batched prerejective aligner made on the device. */
#include "ope_device_draws.h"

#ifdef __cplusplus
}
#endif
#endif /* OPE_H */
