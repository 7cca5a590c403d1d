/*
 * apdgicp_hip.h -- C ABI of libapdgicp_hip.so: RIV-SLAM's APD-GICP scan matcher on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE hot path of Wayne-DWA/RIV-SLAM: fast_gicp::FastAPDGICP
 * behind pcl::Registration, as selected by select_registration_method()
 * (radar_graph_slam/src/radar_graph_slam/registrations.cpp:38-50).  Each entry point names the
 * reference member it replaces; "A:" = fast_apdgicp/include/fast_gicp/gicp/impl/fast_apdgicp_impl.hpp,
 * "L:" = .../gicp/impl/lsq_registration_impl.hpp, "H:" = .../gicp/fast_apdgicp.hpp.
 *
 * Conventions
 *   - Plain C: pointers, sizes, PODs.  No C++/torch types.  All functions return 0 on success and a
 *     negative apdgicp_status on failure; apdgicp_last_error() gives the message (thread-local).
 *     Nothing aborts or throws.  Registration failure is DATA (result.converged == 0), like
 *     hasConverged() in the reference (L:71-75), not an error code.
 *   - 4x4 matrices are COLUMN-MAJOR (Eigen::Matrix4f / Matrix4d memory layout): m[row + 4*col].
 *     6x6 H is column-major too (symmetric anyway); b is [rot(3), trans(3)] as in A:248-250.
 *   - Points: `xyz` is the address of the first x; consecutive points are `stride_bytes` apart
 *     (12 for packed xyz, 16 for float4, 32 for pcl::PointXYZI).  Only x,y,z are read
 *     (intensity is never touched on this path).  Points must be finite.
 *   - `on_device` != 0 means `xyz` is a device (HIP) pointer on the handle's device; the data is
 *     copied into the handle's own buffers either way, so the caller may free/reuse its buffer when
 *     the call returns (host) / when the handle's stream has passed the call (device).
 *   - A handle is single-caller (one thread at a time), owns one HIP stream and no global state;
 *     any number of handles may live in one process and be used from different threads.
 */
#ifndef APDGICP_HIP_H
#define APDGICP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APDGICP_ABI_VERSION 6   /* 2: + inlier_fraction, wait_producer, get_stream; 3: pooled LM batches (enqueue never blocks), + batch_pump, sparse cloud slots;
                                   4: T*p is summed pairwise by default (Eigen >= 3.3), APDGICP_FLAG_XF_LINEAR_CHAIN selects the former order;
                                   5: the three fp32 angles of the sensor model (A:168,172-173) through glibc's atan2f algorithm (apd_atan2f.h) instead of the
                                      device library's; + source_stamp, set_trace / get_trace, debug_atan2f;
                                   6: + APDGICP_FLAG_ALGEBRAIC_APD, build_flags, nearest_neighbours_of, get_trace_step_norms;
                                      still 6 (additive, nothing existing changed): + the apdgicp_scan_filter_* object (range gate, voxel grid, outlier removal);
                                      still 6 (additive): + the apdgicp_ego_velocity_* object (Doppler ego velocity, moving-point removal);
                                      still 6 (additive): + the apdgicp_floor_* object (floor plane detection, under-floor removal);
                                      still 6 (additive): + the apdgicp_map_cloud_* object (map cloud generation: pose transform, gate, octree voxel centres);
                                      still 6 (additive): + the apdgicp_scan_context_* object (Scan Context place recognition: descriptors, ring-key ranking, shift search, top-K);
                                      still 6 (additive): + apdgicp_set_vgicp and the apdgicp_vgicp_* calls (voxelized GICP as a mode of the registration handle);
                                      still 6 (additive): + apdgicp_batch_set_vgicp / _get_vgicp and the apdgicp_batch_vgicp_* calls (voxelized GICP as a mode of the batch handle);
                                      still 6 (additive): + apdgicp_set_ndt / _get_ndt and the apdgicp_ndt_* calls (NDT, P2D and D2D, as a mode of the registration handle);
                                      still 6 (additive): + apdgicp_batch_set_ndt / _get_ndt and the apdgicp_batch_ndt_* calls (NDT as a mode of the batch handle);
                                      still 6 (additive): + apdgicp_debug_live_buffers;
                                      still 6 (additive): + the apdgicp_scan_ingest_* object (power gate and packing of a radar message, IMU deskew, frame transform);
                                      still 6 (additive): + apdgicp_set_icp / _get_icp and the apdgicp_icp_* calls (point-to-point ICP as a mode of the registration handle);
                                      still 6 (additive): + apdgicp_batch_set_icp / _get_icp and the apdgicp_batch_icp_* calls (point-to-point ICP as a mode of the batch handle);
                                      still 6 (additive): + apdgicp_set_vgicp_cuda / _get_vgicp_cuda and the apdgicp_vgicp_cuda_* calls (FAST_VGICP_CUDA as a mode of the registration handle);
                                      still 6 (additive): + apdgicp_batch_set_vgicp_cuda / _get_vgicp_cuda and the apdgicp_batch_vgicp_cuda_* calls (FAST_VGICP_CUDA as a mode of the batch handle);
                                      still 6 (additive): + apdgicp_knn_of, apdgicp_radius_search_of / _rows, apdgicp_search_group_stats (exact k-nearest and radius queries of the target);
                                      still 6 (additive): + apdgicp_scan_ingest_run_polar and apdgicp_scan_ingest_histogram_* (the polar message of cloud_callback_scan, the distance histogram) */

typedef enum {
  APDGICP_OK = 0,
  APDGICP_ERR_INVALID_ARG = -1,   /* null pointer, bad size, k out of range ... */
  APDGICP_ERR_HIP = -2,           /* a HIP runtime call failed (no device, OOM, launch failure) */
  APDGICP_ERR_NO_INPUT = -3,      /* source/target (or correspondences) not set yet */
  APDGICP_ERR_TOO_FEW_POINTS = -4,/* cloud has fewer than k_correspondences points (reference: UB, A:318-321) */
  APDGICP_ERR_UNSUPPORTED = -5,   /* e.g. unknown regularization (reference aborts, A:341-343) */
  APDGICP_ERR_INTERNAL = -6
} apdgicp_status;

/* fast_gicp::RegularizationMethod, gicp/gicp_settings.hpp:6 (same numeric values) */
typedef enum {
  APDGICP_REG_NONE = 0,
  APDGICP_REG_MIN_EIG = 1,
  APDGICP_REG_NORMALIZED_MIN_EIG = 2,
  APDGICP_REG_PLANE = 3,
  APDGICP_REG_FROBENIUS = 4
} apdgicp_regularization;

/* apdgicp_params.flags.  PLAIN_GICP: drop the range-dependent polar noise covariance (cov_dist, A:167-184), which turns the
 * cost into upstream fast_gicp::FastGICP (gicp/impl/fast_gicp_impl.hpp: RCR = cov_B + T cov_A T^T) -- the FAST_GICP branch of
 * select_registration_method() (registrations.cpp:28-37). */
/* XF_LINEAR_CHAIN: the fp32 summation order of `pt = trans_f * p.getVector4fMap()` (A:137,149), the one fp32 operation of the path
 * whose order belongs to Eigen, not to the reference.  Default (flag clear): (r0 x + r1 y) + (r2 z + t) -- Eigen >= 3.3, whose
 * coefficient-based product sums the four terms of a row with redux_novec_unroller (halving), i.e. the Eigen 3.3.4 / 3.3.7 of the
 * platforms the reference names (README.md:5-7).  Flag set: ((r0 x + r1 y) + r2 z) + t -- Eigen 3.2's product_coeff_impl, and
 * what ABI versions <= 3 evaluated.  The two differ in the last ulp of a transformed coordinate: enough to resolve a
 * nearest-neighbour near-tie the other way (poses move by <= 1e-5 m, an LM run may stop one iteration earlier or later).
 * INTEGRATION.md section 7 holds a 30-line probe that tells which order an installed Eigen produces. */
/* FP32_POINT_MATH (opt-in, not the reference's arithmetic): the per-point algebra behind the nearest-neighbour search -- sin / cos of
 * elevation and azimuth, the APD covariance A A^T, RCR = (C_B + cov_d) + R (C_A + cov_d) R^T, its inverse, the residual, M e and
 * every J^T M J term (A:174-192, A:229-258) -- in fp32 instead of fp64.  Stays fp64: cos(AoA) and its reciprocal (it cancels near
 * the +-x axis, A:170-171), the sums over the points, the 6x6 solve and the pose update; the search, the gate and the three fp32
 * angles are unchanged, so correspondences are identical at a given pose.  Measured: final poses move by
 * ~1e-6 m / 1e-7 rad against the default, a Levenberg-Marquardt run may stop an iteration earlier or later.  The default (flag
 * clear) is the reference's precision; bench.py's headline runs with the flag clear. */
/* ALGEBRAIC_APD (opt-in, not the reference's arithmetic; ABI 6): the sensor model of A:167-184 without its three fp32 atan2 calls and
 * three fp64 sin / cos pairs.  The reference rounds the angle of arrival, the elevation (polar from +z) and the azimuth of the
 * transformed point to fp32 and takes fp64 sines and cosines of those; everything the model USES of them are ratios of the point's own
 * coordinates, which this mode forms directly in fp64 from the fp32 transformed point (x, y, z):
 *     cos(az) = x / rho, sin(az) = y / rho (rho = sqrt(x^2 + y^2)),   sin(el) = rho / r, cos(el) = z / r (r = sqrt(x^2 + y^2 + z^2)),
 *     1 / cos(AoA) = r / sqrt(y^2 + z^2), clamped to 1 / |cos(float(pi/2))| = 2.2877e7 -- the largest value the reference's fp32 angle can give,
 * three reciprocal square roots instead of ~255 fp32 and ~120 fp64 instructions per matched point.  Conventions of atan2(0, 0) = 0 on the
 * axes are kept (rho = 0: cos(az) = 1, sin(az) = 0).  The search, the gate and hence the correspondences at a given pose are unchanged;
 * the APD covariance differs from the reference's by the fp32 rounding of its angles (~6e-8 relative in the rotation), final poses by
 * ~1e-7 m (measured: DESIGN.md section 6; tests/test_hip_parity.py::test_algebraic_apd_*), a Levenberg-Marquardt run may stop an
 * iteration earlier or later.  Exclusive with FP32_POINT_MATH.  The default (flag clear) is the reference's arithmetic and bench.py's
 * headline runs with the flag clear. */
enum { APDGICP_FLAG_PLAIN_GICP = 1, APDGICP_FLAG_XF_LINEAR_CHAIN = 2, APDGICP_FLAG_FP32_POINT_MATH = 4, APDGICP_FLAG_ALGEBRAIC_APD = 8 };

/* fast_gicp::LSQ_OPTIMIZER_TYPE, gicp/lsq_registration.hpp:13 (reference default: LM, L:17) */
typedef enum { APDGICP_OPT_LM = 0, APDGICP_OPT_GN = 1 } apdgicp_optimizer;

/* Every tunable the reference object has.  Defaults (apdgicp_default_params) are the class
 * defaults: A:14-28, H:107-109, L:11-24.  The ROS factory overrides some of them
 * (registrations.cpp:41-48). */
typedef struct {
  int32_t k_correspondences;            /* setCorrespondenceRandomness, A:45 ; default 20 ; any k >= 1, exact: 1..32 the pruned kernel, 33..64 the brute-force one, above a selection kernel (~35 sweeps of the cloud per query block: experiments) */
  int32_t max_iterations;               /* pcl setMaximumIterations ; default 64, L:13 */
  int32_t lm_max_iterations;            /* L:19 ; default 10 */
  int32_t optimizer;                    /* apdgicp_optimizer ; default LM */
  int32_t regularization;               /* apdgicp_regularization ; default PLANE, A:25 */
  int32_t flags;                        /* APDGICP_FLAG_*; default 0 */
  double max_correspondence_distance;   /* pcl setMaxCorrespondenceDistance ; default FLT_MAX, A:23 */
  double transformation_epsilon;        /* pcl setTransformationEpsilon ; default 5e-4, L:15 */
  double rotation_epsilon;              /* setRotationEpsilon, L:30 ; default 2e-3 */
  double lm_init_lambda_factor;         /* setInitialLambdaFactor, L:35 ; default 1e-9 */
  double distance_variance;             /* setDistVar, A:63 ; default 0.86 */
  double azimuth_variance_deg;          /* setAzimuthVar, A:55 ; default 0.5 */
  double elevation_variance_deg;        /* setElevationVar, A:59 ; default 1.0 */
} apdgicp_params;

/* What align() reports.  converged/iterations mirror pcl::Registration::converged_ /
 * nr_iterations_ as written by L:59,68,75 ; T is final_transformation_ (L:78). */
typedef struct {
  float T[16];                 /* column-major source->target */
  double final_cost;           /* last linearize() cost y0 (sum of e^T M e), for logging */
  int32_t converged;
  int32_t iterations;          /* nr_iterations_: zero-based index of the last outer iteration */
  int32_t n_linearize;         /* number of linearize() evaluations (A:198) */
  int32_t n_compute_error;     /* number of compute_error() evaluations (A:275) */
  int32_t lm_failed;           /* 1 when step_lm exhausted lm_max_iterations ("lm not converged!!", L:71-74) */
  int32_t n_matched;           /* correspondences inside the gate at the last linearize (A:156) */
} apdgicp_result;

typedef struct apdgicp_handle apdgicp_handle;   /* one registration object == one FastAPDGICP */
typedef struct apdgicp_batch apdgicp_batch;     /* many independent registrations on one GPU */

enum { APDGICP_SOURCE = 0, APDGICP_TARGET = 1 };

/* ------------------------------------------------------------------ library */
int apdgicp_abi_version(void);
/* Fingerprint of the kernel sources this library was compiled from (riv-slam_amd/build.py:source_stamp(), the first 16 hex digits
 * of a SHA-256 over csrc/ and include/, passed in at compile time): what bench.py and the test suite compare with the sources on
 * disk before they trust a prebuilt library, and what a committed counter profile names.  "unstamped" for a build that did not
 * go through build.py. */
const char* apdgicp_source_stamp(void);
/* The compiler flags this library was built with (as build.py passed them; "unknown" for a hand build), then " | variant:" followed by every
 * experiment define compiled in that changes kernels or results (APD_ABL_*: ablations, wrong by design; APD_OCML_ATAN2F, APD_SINCOS_NO_TABLE:
 * A/B builds) -- detected by the preprocessor inside the library.  Empty after "variant:" = the product.  The Python loader refuses a variant
 * library unless APDGICP_ALLOW_VARIANT_LIB=1; bench.py prints the string in its line. */
const char* apdgicp_build_flags(void);
const char* apdgicp_last_error(void);
int apdgicp_device_count(int* count);
void apdgicp_default_params(apdgicp_params* p);                                  /* A:14-28, L:11-24 */

/* ------------------------------------------------------------------ single registration object */
/* FastAPDGICP::FastAPDGICP() (A:14).  `stream` may be NULL (the handle creates its own) or a
 * hipStream_t the caller owns. */
int apdgicp_create(const apdgicp_params* p, int device, void* stream, apdgicp_handle** out);
int apdgicp_destroy(apdgicp_handle* h);                                           /* ~FastAPDGICP */
int apdgicp_set_params(apdgicp_handle* h, const apdgicp_params* p);               /* the setters A:34-65, L:30-37 */
int apdgicp_get_params(const apdgicp_handle* h, apdgicp_params* p);

/* setInputSource / setInputTarget (A:90-108).  `token` is the caller's identity of the cloud
 * (the adapter passes the shared_ptr's raw address): a call with the token already held is the
 * reference's pointer-equality early return and keeps the cached covariances; token 0 never matches. */
int apdgicp_set_source(apdgicp_handle* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device, uint64_t token);
int apdgicp_set_target(apdgicp_handle* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device, uint64_t token);
int apdgicp_clear_source(apdgicp_handle* h);                                      /* A:78-81 */
int apdgicp_clear_target(apdgicp_handle* h);                                      /* A:84-87 */
int apdgicp_swap_source_and_target(apdgicp_handle* h);                            /* A:68-75 */

/* calculate_covariances (A:303-363), normally run lazily by align (A:122-127).  which = APDGICP_SOURCE/TARGET */
int apdgicp_compute_covariances(apdgicp_handle* h, int which);
/* getSourceCovariances / getTargetCovariances (H:67-73): n x 16 doubles, each a column-major 4x4
 * with zero 4th row/column, exactly the reference's std::vector<Matrix4d> memory. */
int apdgicp_get_covariances(apdgicp_handle* h, int which, double* out_n16, int64_t n);
/* setSourceCovariances / setTargetCovariances (A:111-118) */
int apdgicp_set_covariances(apdgicp_handle* h, int which, const double* in_n16, int64_t n);

/* linearize (A:198-272) at pose T (the public probe is LsqRegistration::evaluateCost, L:50-52).
 * H and b may both be NULL (cost only, A:242-244).  Updates the correspondences and Mahalanobis
 * matrices held by the handle (update_correspondences, A:133-194). */
int apdgicp_linearize(apdgicp_handle* h, const double T[16], double H[36], double b[6], double* cost);
/* compute_error (A:275-298): frozen correspondences / Mahalanobis of the last linearize */
int apdgicp_compute_error(apdgicp_handle* h, const double T[16], double* cost);
/* correspondences_ / sq_distances_ (H:104-105) and mahalanobis_ (H:102; n x 16 doubles, zeros for
 * unmatched points) after the last linearize; any pointer may be NULL.  After apdgicp_linearize every sq_dist is the
 * exact nearest-neighbour distance.  Inside apdgicp_align the search stops at the correspondence gate: a point with
 * corr == -1 then reports the smallest float >= max_correspondence_distance^2 (or the distance to its previous
 * neighbour) instead of the distance to a neighbour the reference would reject anyway (A:156); correspondences are exact. */
int apdgicp_get_correspondences(apdgicp_handle* h, int32_t* corr, float* sq_dist, int64_t n);
int apdgicp_get_mahalanobis(apdgicp_handle* h, double* out_n16, int64_t n);

/* pcl::Registration::align(output, guess) -> FastAPDGICP::computeTransformation (A:121-130) ->
 * LsqRegistration::computeTransformation (L:55-80): the whole GN/LM loop runs on the device.
 * guess may be NULL (identity, as align(output)). */
int apdgicp_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out);
/* same loop, but driven from the host through apdgicp_linearize / apdgicp_compute_error exactly
 * like the reference's virtual calls (L:127-173): the bit-faithful debug path */
int apdgicp_align_host_loop(apdgicp_handle* h, const float guess[16], apdgicp_result* out);
int apdgicp_get_final_hessian(apdgicp_handle* h, double H[36]);                   /* getFinalHessian, L:45 */
/* Debug: the optimiser's per-iteration trace, as a debugger stepping through L:64-76 / L:127-173 would write it down.  With
 * tracing enabled every apdgicp_align (the device state machine writes the trace itself) and apdgicp_align_host_loop of this
 * handle records, per Levenberg-Marquardt trial, the lambda the step was solved with, its gain ratio rho and the two costs rho
 * compares (L:137-146: y0 of linearize, yi of compute_error at the trial pose; y0s / yis may be NULL) and, per completed outer
 * iteration, the pose x0 behind it (L:119 / L:166; column-major 4x4 doubles).  get_trace returns the counts of the last align
 * (they may exceed the capacities given: only what fits is copied).  Gauss-Newton runs record poses only. */
int apdgicp_set_trace(apdgicp_handle* h, int enable);
int apdgicp_get_trace(apdgicp_handle* h, int64_t trial_capacity, double* lambdas, double* rhos, double* y0s, double* yis, int64_t* n_trials,
                      int64_t pose_capacity, double* poses16, int64_t* n_poses);
/* ... and, per trial, the norm of the step d it solved for: the "|delta|" column of the table the reference prints under setDebugPrint
 * (L:148-154).  Same counts and order as the trials of apdgicp_get_trace. */
int apdgicp_get_trace_step_norms(apdgicp_handle* h, int64_t capacity, double* norms, int64_t* n_trials);
/* Debug: out[i] = atan2f(y[i], x[i]) as the kernels evaluate it on `device` (include/apd_atan2f.h: glibc's generic atan2f restated;
 * A:168,172-173 call the C library's float overload); host arrays.  For the bit-for-bit comparison with the host's evaluation. */
int apdgicp_debug_atan2f(int device, const float* y, const float* x, float* out, int64_t n);
/* Debug: how many device allocations (hipMalloc) and pinned host allocations (hipHostMalloc) the library's objects hold in this process right now,
 * over all handles of every kind.  Every object frees what it holds when it is destroyed, so the counts after create ... destroy equal those
 * before.  The two poll-record blocks of an engine (one per registration or batch handle, two once apdgicp_batch_align_enqueue has been used)
 * are kept outside the counted owners and are not in pinned_buffers.  Either pointer may be NULL. */
int apdgicp_debug_live_buffers(int64_t* device_buffers, int64_t* pinned_buffers);
/* pcl::transformPointCloud(*input_, output, final_transformation_) (L:79): writes n xyz triples
 * `out_stride_bytes` apart into host memory */
int apdgicp_transform_source(apdgicp_handle* h, const float T[16], float* out_xyz, int64_t n, int64_t out_stride_bytes);
/* pcl::Registration::getFitnessScore(max_range): mean squared 1-NN distance of the T-transformed
 * source to the target over the points whose SQUARED distance is <= max_range (PCL compares the
 * squared distance with max_range as is); DBL_MAX when no point qualifies.  Callers:
 * loop_detector.cpp:229, scan_matching_odometry_nodelet.cpp:698.  n_inliers may be NULL */
int apdgicp_fitness_score(apdgicp_handle* h, const float T[16], double max_range, double* score, int64_t* n_inliers);
/* ScanMatchingStatus::inlier_fraction (scan_matching_odometry_nodelet.cpp:701-712): the number of T-transformed source
 * points whose nearest target point is STRICTLY closer than max_correspondence_dist (squared float distance < dist*dist
 * in double, as there), divided by the source size in float.  n_inliers may be NULL */
int apdgicp_inlier_fraction(apdgicp_handle* h, const float T[16], double max_correspondence_dist, double* fraction, int64_t* n_inliers);
/* The nearest target point of every T-transformed source point: what pcl::search::KdTree::nearestKSearch(T * source[i], 1, ...)
 * returns, for all i in ONE batched search on the device -- index into the target cloud as set (a tie: the lowest index) and the
 * fp32 squared distance (FLANN L2_Simple order on the fp32-transformed point, like A:149-153); no correspondence gate.  This is
 * what serves the base-class calls of the nodelets -- getFitnessScore() (loop_detector.cpp:229) and
 * getSearchMethodTarget()->nearestKSearch(aligned[i], 1, ...) (scan_matching_odometry_nodelet.cpp:697-707) -- through the search
 * object FastAPDGICPHip installs, so that PCL never builds its CPU kd-tree.  Leaves the handle as apdgicp_linearize at T would. */
int apdgicp_nearest_neighbours(apdgicp_handle* h, const float T[16], int32_t* index, float* sq_dist, int64_t n);
/* The nearest target point of ARBITRARY query points (host memory, n x {x, y, z, ...} floats, stride_bytes >= 12) in one batched device
 * pass: what pcl::search::Search::nearestKSearch(cloud, indices, 1, ...) returns (search.h: the batch form of the call above) --
 * index into the target as set (a tie: the lowest index) and the fp32 squared distance (FLANN L2_Simple order), no gate.  The queries
 * are sorted along the curve like a source cloud and searched with the same exact pruned kernel; no covariances are computed for them.
 * This serves the search object's queries that are NOT the transformed source points (the per-query host scan of round 5 cost 500 k
 * distance evaluations per query on a submap).  The next align / linearize of the handle sets its own pair up again. */
int apdgicp_nearest_neighbours_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, int32_t* index, float* sq_dist);
/* the points of the source / target cloud as set, n x {x, y, z} floats in the caller's order, into host memory (the fall-back of
 * that search object for a query that is not one of the transformed source points needs the target of a device-resident submap) */
int apdgicp_get_points(apdgicp_handle* h, int which, float* out_xyz, int64_t n);

/* ------------------------------------------------------------------ exact k-nearest and radius queries of the target
 * What else a pcl::search::KdTree over the target is asked for (nearestKSearch with k > 1, radiusSearch: DBSCAN_kdtree.h, the non-dense
 * branch of RadiusOutlierRemoval, FastGICPMultiPoints::update_correspondences), for ARBITRARY query points, in one device pass per call.
 * The kernels (riv-slam_amd/csrc/apd_search.hpp) and the restatement the tests compare with (tests/search_np.py) follow this list:
 *   Q1. Order.  The distance is d2 = sqdist1(t, q): fp32 differences, dx*dx, + dy*dy, + dz*dz, each operation rounded, no contraction.
 *       The key of a target point is (bits of d2) << 32 | its index in the target as set; keys are unique, and ascending key is FLANN's
 *       L2_Simple order with ties by ascending index, the order of every other search here.  The target is the whole target cloud as
 *       set (host or device-resident), in every mode of the handle; mode kernels, maps and prepared clouds are neither read nor written.
 *   Q2. apdgicp_knn_of: for every query the n_found = min(k, M) smallest keys, ascending (M: the target's size).  Output is row-major
 *       n x k: int32 index into the target as set and float distance; the unused tail of a row is -1 / +Inf.  1 <= k <= 64; k < 1 is
 *       APDGICP_ERR_INVALID_ARG, k > 64 is APDGICP_ERR_UNSUPPORTED.
 *   Q3. Queries.  Host memory, n x {x, y, z, ...} floats, stride_bytes >= 12 and a multiple of 4, as in apdgicp_nearest_neighbours_of.
 *       A non-finite coordinate refuses the call with APDGICP_ERR_INVALID_ARG, the message naming the first such query; this is checked
 *       on the host before anything is enqueued.  n <= 0 or a null pointer: APDGICP_ERR_INVALID_ARG; no target: APDGICP_ERR_NO_INPUT.
 *   Q4. Radius.  r2 = (float)((double)radius * (double)radius).  A target point is a hit iff d2 < r2, strictly (FLANN's
 *       RadiusResultSet::addPoint behind pcl::KdTreeFLANN::radiusSearch, which passes that float).  radius is finite and >= 0 (otherwise
 *       APDGICP_ERR_INVALID_ARG); radius = 0 yields no hit, not even a coincident point.
 *   Q5. Rows.  A row holds its hits in ascending key.  With max_nn = 0 or max_nn >= M it holds all of them, otherwise the max_nn
 *       smallest (PCL's max_nn).  max_nn < 0: APDGICP_ERR_INVALID_ARG.
 *   Q6. Rows come back in two calls.  apdgicp_radius_search_of searches, writes row_start[0 .. n] (row i is [row_start[i],
 *       row_start[i + 1])) and *total = row_start[n], and leaves the rows in buffers of the handle; apdgicp_radius_search_rows copies
 *       `total` entries.  The second call without a first is APDGICP_ERR_NO_INPUT, and so is one after the target was set, cleared or
 *       swapped since, or after a search that failed.  More than 2^31 - 1 hits in all: APDGICP_ERR_UNSUPPORTED.  An allocation that
 *       fails is APDGICP_ERR_HIP, and the handle stays usable.
 *   Q7. Handle state is as after apdgicp_nearest_neighbours_of: the handle's own pair is set up again by whoever needs it next, and
 *       the next align returns the bytes it returned before.  Source, target, covariances and cached maps are untouched.
 *   Q8. A row is a pure function of (target, query, k or radius, max_nn): it does not depend on the other queries of the call, on
 *       their order or on their number.
 *   Q9. k = 1 returns the bytes of apdgicp_nearest_neighbours_of.  A radius search with 0 < max_nn <= 64 returns the first max_nn
 *       entries of apdgicp_knn_of(k = max_nn) that pass Q4. */
int apdgicp_knn_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, int32_t k, int32_t* index, float* sq_dist, int32_t* n_found);
int apdgicp_radius_search_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, double radius, int32_t max_nn, int64_t* row_start /* n + 1 */,
                             int64_t* total);
int apdgicp_radius_search_rows(apdgicp_handle* h, int32_t* index, float* sq_dist);
/* of the last apdgicp_knn_of / apdgicp_radius_search_of: target groups (128 points) whose points a wave of the searching launch
 * (the counting one, where a second fills the rows) looked at, summed over its waves, and waves x groups, the same sum with no
 * pruning (the measurement of tests/measure/bench_search_queries.py) */
int apdgicp_search_group_stats(apdgicp_handle* h, int64_t* groups_visited, int64_t* groups_total);

int apdgicp_synchronize(apdgicp_handle* h);
/* Ordering against the stream that PRODUCED device-resident inputs.  The handle's streams are non-blocking: without this
 * call nothing orders a kernel that still writes the cloud (on the caller's stream) against the handle's pack kernel.
 * Everything queued on `producer_stream` (a hipStream_t; NULL = the legacy default stream) before this call completes
 * before anything the handle enqueues afterwards starts; the host does not wait.  The other direction is the caller's:
 * a device buffer handed to set_source/set_target/batch_set_cloud(s) may be freed or overwritten only after the handle
 * has passed the call (apdgicp_synchronize / the align that follows / batch_align_collect of the batch that used it). */
int apdgicp_wait_producer(apdgicp_handle* h, void* producer_stream);
/* the hipStream_t the handle enqueues on (its own, or the one given to apdgicp_create): for callers that order their own
 * work -- or their timing events -- against the handle without a host-side wait.  Every call of a handle ends with all
 * of its work joined back onto this stream. */
int apdgicp_get_stream(apdgicp_handle* h, void** stream);

/* ------------------------------------------------------------------ voxelized GICP as a mode of the handle
 * fast_gicp::FastVGICP, the FAST_VGICP branch of select_registration_method() (registrations.cpp:62-70; it sets reg_resolution and
 * leaves DIRECT1 / ADDITIVE).  "V:" = fast_apdgicp/include/fast_gicp/gicp/impl/fast_vgicp_impl.hpp, "VX:" = .../gicp/fast_vgicp_voxel.hpp.
 * Covariances of both clouds are FastGICP::calculate_covariances (gicp/impl/fast_gicp_impl.hpp:255-312), line for line the computation
 * of A:303-363 -- what apdgicp_compute_covariances does.  The kernels (riv-slam_amd/csrc/apd_vgicp.hpp) and the restatement the tests
 * compare with (tests/vgicp_np.py) follow this list:
 *   V1. Voxel coordinate (VX:158-160): c = (int32) floor(x / res - 0.5) per axis, x the fp64 value of the fp32 coordinate, a true fp64
 *       division (not a multiplication by 1 / res).
 *   V2. Validity and key range.  Target points must be finite with |c| < 2^20 per axis; otherwise apdgicp_linearize / apdgicp_align
 *       (and apdgicp_vgicp_voxel_count) return APDGICP_ERR_INVALID_ARG and name the first offending point.  The key of a voxel is its
 *       three coordinates, each biased by 2^20 into 21 bits, x highest, in a uint64.  A SOURCE point whose coordinate, after an offset
 *       has been added, leaves that range, or whose transformed position is not finite, is a miss; the range is tested BEFORE the key
 *       is packed, so an out-of-range coordinate never aliases a valid key.  The edges, exactly: a coordinate x = 2^20 res has
 *       c = 2^20 - 1 and is still VALID; the first refused positions are x = (2^20 + 0.5) res (c = 2^20) and x = -(2^20 - 0.5) res
 *       (c = -2^20); the last valid ones just inside them.
 *   V3. Voxel order and sums (VX:129-156).  Voxels are numbered in ascending key order (= lexicographic (cx, cy, cz); the reference's
 *       std::unordered_map has no defined order).  Within a voxel the mean and the six unique covariance entries are fp64 sums, started
 *       at 0, over its points IN THE CALLER'S ORDER, then each divided by the count (ADDITIVE; ADDITIVE_WEIGHTED takes the same branch,
 *       VX:138-141): counts, means and covariances are bit-equal to the reference's sequential loop.  A voxel that holds every point
 *       is legal and is summed by one lane.  The map is a pure function of target, covariances, resolution and mode (the reference
 *       rebuilds it in every computeTransformation, V:67); the handle caches it.
 *   V4. Transform (V:84-85): q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in fp64 -- unlike APD-GICP, whose search transforms in fp32.
 *       Eigen's own summation order for Isometry3d * Vector4d is not pinned by the reference tree.
 *   V5. Correspondences (V:86-94).  c(q) + each offset of DIRECT1 / DIRECT7 / DIRECT27 in the order of VX:17-43 ({0}; {0, +x, -x, +y,
 *       -y, +z, -z}; (i - 1, j - 1, k - 1) with k fastest) is looked up; every hit is a correspondence (point, voxel) with
 *       M = (C_voxel + R C_A R^T)^-1 (3x3 block, by cofactors); no distance gate.  linearize (V:119-180): e = mean_voxel - q,
 *       w = sqrt(count), cost += w (e . (M e)), H += w J^T M J, b += w J^T (M e), J = [skew(q) | -I].  A point's correspondences are
 *       added in offset order, points in the caller's order one per lane; lanes, waves and blocks are added in a fixed tree / block
 *       order in fp64 (the reference's own order depends on the OpenMP schedule): the same bits on every run.
 *   V6. Frozen state (V:183-204).  compute_error evaluates the same cost at the trial pose over the voxel indices of the last linearize
 *       and the M of the last linearize POSE.  The handle stores the index per (point, offset) (4 bytes) and that pose and recomputes M
 *       with the same device function -- the same bits as a stored M (6 doubles per correspondence: 1.3 kB per point for DIRECT27).
 *       Which of the two is faster has not been measured.
 *   V7. Degenerate cases.  No correspondence at a linearize inside align: the loop stops there with converged = 0, lm_failed = 0,
 *       T = the pose so far, n_matched = 0 (the reference would solve a singular system).  max_correspondence_distance is ignored, as in
 *       the reference.  MULTIPLICATIVE: APDGICP_ERR_UNSUPPORTED (the ROS factory never selects it).
 * With the mode on, apdgicp_linearize / apdgicp_compute_error run these kernels; apdgicp_align and apdgicp_align_host_loop both run the
 * host-driven loop of apdgicp_align_host_loop over them (trace, final Hessian and apdgicp_result as there; n_matched = the number of
 * correspondences, up to 27 per source point: the int32 field saturates at 2^31 - 1, i.e. beyond 79 million source points with DIRECT27); apdgicp_get_correspondences / apdgicp_get_mahalanobis return APDGICP_ERR_UNSUPPORTED; fitness_score,
 * nearest_neighbours*, transform_source and get_points are unchanged.  The APD flags of apdgicp_params have no meaning for this cost.
 * The map is kept until the target changes (set_target with another token, set_covariances(TARGET), swap_source_and_target,
 * clear_target, a parameter change that invalidates the covariances) or the resolution / mode does.  The handle tracks this by identity, not
 * by call: the map remembers which setting of the target's points and which writing of its covariances it was built from and is rebuilt
 * whenever either is another one -- whichever entry point (with the mode on or off) replaced the cloud or recomputed the covariances in
 * between; the frozen state behind apdgicp_compute_error is tied to the source's points and covariances and to the map in the same way
 * (otherwise APDGICP_ERR_NO_INPUT).  With the mode off nothing differs
 * from a handle that never had it on.
 *
 * Batch handles have the same mode (apdgicp_batch_set_vgicp, declared with the batch calls below; kernels: riv-slam_amd/csrc/apd_vgicp_batch.hpp),
 * with the optimiser loop on the device:
 *   V8. Maps per cloud slot.  Every slot named as target_cloud by a pair of the batch gets the voxel map of V1 .. V3; counts, means and
 *       covariances are bit-equal to those the single handle builds from the same points and covariances.  The map is cached per slot, by
 *       identity: it is rebuilt when the slot's points were set again, its covariances were rewritten, the resolution or the accumulation
 *       mode changed, or apdgicp_batch_clear ran.  A slot used only as a source gets no map.  Building the maps of a batch costs at most
 *       ONE host wait for the whole batch: a slot's voxel buffers are sized for as many voxels as it has points, the voxel count stays on
 *       the device, and the "first offending point" words and voxel counts of all slots come back in one copy.  A target with a point that
 *       V2 refuses fails the align with APDGICP_ERR_INVALID_ARG, the message naming the slot and the point; no pair has run, and the
 *       handle stays usable.
 *   V9. The per-point arithmetic is that of V4 .. V6, bit for bit: the same device functions, the 29 sums in the same written order, one
 *       source point per lane in the caller's order in blocks of 256, the block rows added in block order starting from 0.0.  Hence H, b,
 *       cost and correspondence count of a pair's FIRST linearize equal apdgicp_linearize of a single handle at the same guess, bit for bit.
 *   V10. Optimiser.  The control flow of apdgicp_align_host_loop (L:55-173), run per pair by the device state machine of the APD batch
 *       path, plus V7: a linearize without any correspondence ends that pair there with converged = 0, lm_failed = 0, n_linearize counted,
 *       iterations = the current iteration, T = the pose so far, final_cost = that linearize's cost, n_matched = 0.  The frozen state of
 *       V6 is per pair: the voxel indices per (point, offset) and the pose of the pair's last linearize.  sin / cos of the step's rotation
 *       come from the device library instead of the host's, so iterates agree with the single handle's to rounding, not bit for bit.
 *   V11. A pair's record is a pure function of the pair: the same (source, target, guess, parameters) gives byte-identical records whether
 *       the pair runs alone or among any others, at any position of the list, on a first align and on a reused handle.
 *   V12. No host round trip per iteration.  One tick is two launches (per-point pass, per-pair step); the host enqueues ticks in chunks and
 *       looks at one word in pinned memory, the number of finished pairs, between chunks, with at least one chunk enqueued ahead while it
 *       waits.  A finished pair's blocks exit on reading its status.  The loop ends when every pair is done, or after
 *       max_iterations * (1 + lm_max_iterations) ticks (max_iterations with Gauss-Newton).
 * With the mode on, apdgicp_batch_align / _align_async / _copy_results / _synchronize run this path and fill the same apdgicp_result records
 * (n_matched = the number of correspondences, saturating as above; align_async may wait internally -- the run length is data dependent --
 * and returns with the device records complete); apdgicp_batch_fitness and the cloud calls are unchanged; apdgicp_batch_set_pair_groups is
 * accepted and has no effect; apdgicp_batch_align_enqueue / _collect / _pump return APDGICP_ERR_UNSUPPORTED (one batch at a time) and
 * apdgicp_batch_is_pooled returns 0.  With the mode off a batch handle does exactly what one that never had it on does. */
typedef enum { APDGICP_VGICP_DIRECT1 = 0, APDGICP_VGICP_DIRECT7 = 1, APDGICP_VGICP_DIRECT27 = 2 } apdgicp_vgicp_search;   /* NeighborSearchMethod, gicp_settings.hpp */
typedef enum { APDGICP_VGICP_ADDITIVE = 0, APDGICP_VGICP_ADDITIVE_WEIGHTED = 1, APDGICP_VGICP_MULTIPLICATIVE = 2 } apdgicp_vgicp_mode;   /* VoxelAccumulationMode */
typedef struct {
  double resolution;         /* setResolution, V:31 ; default 1.0, V:22 ; finite and > 0 */
  int32_t neighbor_search;   /* apdgicp_vgicp_search ; default DIRECT1, V:23 */
  int32_t voxel_mode;        /* apdgicp_vgicp_mode ; default ADDITIVE, V:24 */
} apdgicp_vgicp_params;
void apdgicp_vgicp_default_params(apdgicp_vgicp_params* p);                      /* 1.0, DIRECT1, ADDITIVE: V:19-25 */
/* p != NULL: the mode on with these parameters; NULL: back to APD-GICP / plain GICP as apdgicp_params says */
int apdgicp_set_vgicp(apdgicp_handle* h, const apdgicp_vgicp_params* p);
int apdgicp_get_vgicp(const apdgicp_handle* h, apdgicp_vgicp_params* p, int* enabled);   /* either output may be NULL */
/* number of voxels of the target's map (built if it is not there; needs the target only) */
int apdgicp_vgicp_voxel_count(apdgicp_handle* h, int64_t* n_voxels);
/* the map in voxel order (V3), host memory, any pointer may be NULL: coordinates (n x 3), counts, means (n x 3), covariances (n x 9,
 * the 3x3 block); capacity >= the voxel count */
int apdgicp_vgicp_get_voxels(apdgicp_handle* h, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9);
/* voxel_correspondences_ of the last linearize: n_source x n_offsets voxel indices in offset order, -1 = miss */
int apdgicp_vgicp_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_source);
/* Debug: how many times this handle has built a voxel map (the tests of the cache rules read it) */
int apdgicp_vgicp_build_count(apdgicp_handle* h, int64_t* n_builds);

/* ------------------------------------------------------------------ FAST_VGICP_CUDA as a mode of the handle
 * fast_gicp::FastVGICPCuda, the FAST_VGICP_CUDA branch of select_registration_method() (registrations.cpp:51-61).  Not the algorithm of
 * the FAST_VGICP mode above: its PLANE regularisation REMOVES every point whose neighbourhood is line-like from both clouds, k is fixed at
 * 20, and it owns the DIRECT_RADIUS neighbour search.  Citation keys, paths under fast_apdgicp/:
 *   VCI: include/fast_gicp/gicp/impl/fast_vgicp_cuda_impl.hpp      VC: src/fast_gicp/cuda/fast_vgicp_cuda.cu
 *   CE:  src/fast_gicp/cuda/covariance_estimation.cu               CR: src/fast_gicp/cuda/covariance_regularization.cu
 *   GV:  src/fast_gicp/cuda/gaussian_voxelmap.cu                   FC: src/fast_gicp/cuda/find_voxel_correspondences.cu
 *   CD:  src/fast_gicp/cuda/compute_derivatives.cu
 * The kernels (riv-slam_amd/csrc/apd_vgicp_cuda.hpp) and the restatement the tests compare with (tests/vgicp_cuda_np.py) follow this list:
 *   VC1. Neighbours.  k = 20 always (VCI:38: setCorrespondenceRandomness is a no-op); apdgicp_params::k_correspondences is not read.
 *        CPU_PARALLEL_KDTREE (the default, VCI:27) and GPU_BRUTEFORCE both mean the engine's exact k-NN, the point itself included, the
 *        neighbours in rank order: ascending fp32 squared distance, ties by ascending original index (the engine's key order).
 *        GPU_RBF_KERNEL: APDGICP_ERR_UNSUPPORTED.  A cloud of fewer than 20 points: APDGICP_ERR_TOO_FEW_POINTS.
 *   VC2. Raw covariance (CE:26-34).  S1 = sum p, S2 = sum p p^T (six unique entries) over the 20 neighbours in rank order: fp64 sums started
 *        at 0, p the fp64 value of the fp32 point, every product rounded before it is added.  mean = S1 / 20, C_rc = S2_rc / 20 - mean_r mean_c.
 *        This is the reference's expression in absolute coordinates, not the query-relative form of apdgicp_compute_covariances.
 *   VC3. Regularisation (CR:91-117), from the eigen-decomposition the rest of the library uses (cyclic Jacobi), eigenvalues
 *        lambda0 <= lambda1 <= lambda2.
 *        PLANE (the default, VCI:26): the point is KEPT iff lambda1 > 0.1 lambda2 in fp64 (CR:26-31; false for a NaN, which drops the point);
 *        a kept point's covariance is V diag(1e-3, 1, 1) V^T, the 1e-3 on lambda0's vector, each entry the sum of its three products in
 *        the order lambda2's, lambda1's, lambda0's vector (with orthonormal V the reference's V D V^-1).
 *        MIN_EIG (CR:73-87): V diag(max(lambda, 1e-3)) V^T as N3.  No filter.
 *        FROBENIUS (CR:63-71): C' = C + 1e-3 I, the result (C'^-1 / ||C'^-1||_F)^-1.  No filter.
 *        NONE and NORMALIZED_MIN_EIG (the reference prints "unimplemented" and goes on with raw covariances): APDGICP_ERR_UNSUPPORTED.
 *   VC4. The filter compacts.  With PLANE the kept points, in the caller's order, ARE the cloud of this mode, for source and target alike
 *        (CR:104-109 replaces the points): correspondences, rows, the voxel map and n_matched see kept points only.  kept_index[j] = the
 *        original index of kept point j; n_kept and kept_index are readable (apdgicp_vgicp_cuda_kept).  Flags, a block scan, a scatter; no
 *        atomics.  Preparing a cloud (k-NN, VC2, VC3, compaction) costs one host wait.  Zero kept points on either side is legal: VC9.
 *   VC5. Voxel map (GV:229-252, :154-167): V1 .. V3 above, ADDITIVE, over the kept target points and their VC3 covariances -- bit-equal to
 *        what the FAST_VGICP mode builds from those points and covariances.
 *   VC6. Offsets (VC:42-95).  DIRECT1 / DIRECT7 / DIRECT27 in V5's order.  DIRECT_RADIUS(r): for i, j, k from -ceil(r) to ceil(r), k
 *        fastest, the offset (i, j, k) is kept iff sqrt(i^2 + j^2 + k^2) <= r + 1e-3 in fp64 (so r = 1.0 holds DIRECT7's offsets in
 *        another order).  r must be finite with 0 <= r <= 4: 1 offset at r = 0 and 0.5, 7 at 1.0, 19 at 1.5, 33 at 2.0, 81 at 2.5, 123 at
 *        3.0, 257 at 4.0; anything else is APDGICP_ERR_INVALID_ARG.  search_radius is read only with DIRECT_RADIUS.  V2's rule holds for
 *        offsets of this size: a source coordinate up to 2^20 + 3 is still offered to the per-offset range test |c + o| < 2^20, made on
 *        exact integers before the key is packed.
 *   VC7. Correspondences and cost (FC:55-60, CD:50-92): V4 / V5 over the kept source, every hit of an offset a term, M = (C_voxel + R C_A
 *        R^T)^-1, w = sqrt(count), e = mean - q, J = [skew(q) | -I]; terms in offset order, lanes, waves and blocks in V5's fixed order.
 *   VC8. Frozen state (VC:276-284): V6 over the stored indices, n_kept x n_offsets int32, point-major, -1 = miss.
 *   VC9. Degenerate cases: V7.  No correspondence at a linearize inside align (also: no kept point on either side) ends the loop with
 *        converged = 0, lm_failed = 0, n_matched = 0, T = the pose so far.  max_correspondence_distance and the APD flags are not read.
 *   VC10. Mode rules.  apdgicp_set_vgicp_cuda is exclusive with apdgicp_set_vgicp, _set_ndt and _set_icp: switching one on switches the others
 *        off; NULL returns to what apdgicp_params says.  The prepared cloud (kept list + covariances) is cached by the identity of the
 *        cloud's points and the regularisation, the map by that plus the resolution; apdgicp_swap_source_and_target swaps the prepared
 *        clouds and the map is rebuilt (VC:97-107).  The mode's covariances live in buffers of their own: the covariances of
 *        apdgicp_compute_covariances / _set_covariances are neither read nor written.  With the mode off a handle does exactly what one that
 *        never had it on does.  apdgicp_linearize / _compute_error run these kernels; apdgicp_align and apdgicp_align_host_loop run the
 *        host-driven loop over them as in the FAST_VGICP mode (trace, final Hessian, apdgicp_result).  fitness_score, nearest_neighbours*,
 *        transform_source and get_points are unchanged, over the whole cloud; apdgicp_get_correspondences / _get_mahalanobis return
 *        APDGICP_ERR_UNSUPPORTED.
 *
 * Batch handles have the same mode (apdgicp_batch_set_vgicp_cuda, declared with the batch calls below; kernels:
 * riv-slam_amd/csrc/apd_vgicp_cuda_batch.hpp), with the optimiser loop on the device:
 *   VC11. Prepared clouds per slot.  Every slot named by a pair of the batch, as source or as target, gets the prepared cloud of VC1 .. VC4:
 *        kept list, raw and regularised covariances and kept points are bit-equal to what the single handle prepares from the same points
 *        (the same device functions under kernels that carry the slot in the grid).  It is cached per slot by the identity of the slot's
 *        points and the regularisation: rebuilt when the slot is set again, the regularisation changes, or apdgicp_batch_clear ran.  The
 *        covariances of apdgicp_batch_compute_covariances / _set_covariances are neither read nor written and an align does not ask for
 *        them, so a cloud of 20 .. k_correspondences - 1 points aligns.  Preparing all uncached slots of a batch costs ONE host wait: the
 *        launches of all slots are enqueued with no wait in between, every slot's kept count comes back in one copy and the k-NN error
 *        flag in another, and the buffers behind the compaction are sized for n kept points.  (A slot whose buffers exist and are too
 *        small for its new cloud costs one more wait, before they are replaced.)  A slot of fewer than 20 points named by a pair fails the
 *        align with APDGICP_ERR_TOO_FEW_POINTS, the message naming the slot; no pair has run and the handle stays usable.
 *   VC12. Maps per target slot.  VC5 over the kept points of every slot named as target_cloud, by the builder of V8: at most one more wait
 *        per batch, none when every map is current.  A map is cached by its preparation's identity and the resolution and is bit-equal to
 *        the single handle's.  A target slot without a kept point gets an empty map without a sort.  A kept target point that V2 refuses
 *        fails the align with APDGICP_ERR_INVALID_ARG, the message naming the slot and the point by its index in the caller's cloud; no
 *        pair has run and the handle stays usable.
 *   VC13. The per-point arithmetic is that of VC6 .. VC8 through the same device functions: one kept source point per lane in the caller's
 *        order in blocks of 256, every search (DIRECT1 / 7 / 27 too) through the offset table, the block rows added in block order starting
 *        from 0.0.  Hence H, b, cost and n_matched of a pair's FIRST linearize equal apdgicp_linearize of a single handle in this mode at the
 *        same guess, bit for bit.
 *   VC14. Optimiser: V10 as it stands, the frozen indices n_kept x n_offsets per pair (pairs x max n_kept x n_offsets int32 in one buffer,
 *        its size computed in size_t; an allocation that fails comes back as APDGICP_ERR_HIP), and V7 / VC9: a pair with no kept point on
 *        either side ends at its first linearize with n_matched = 0, n_linearize = 1, T = the guess.
 *   VC15. A pair's record is a pure function of the pair, as V11.
 *   VC16. Ticks and mode rules.  One tick is two launches, ticks go out in chunks of 4, one pinned word is looked at between chunks (V12).
 *        apdgicp_batch_set_vgicp_cuda is exclusive with apdgicp_batch_set_vgicp, _set_ndt and _set_icp in both directions: switching one
 *        on switches the others off.  With the mode on apdgicp_batch_align_enqueue / _collect / _pump return APDGICP_ERR_UNSUPPORTED and
 *        apdgicp_batch_is_pooled returns 0; apdgicp_batch_fitness and the cloud calls are unchanged, over the whole clouds.  With the mode
 *        off a batch handle does exactly what one that never had it on does.  The sharded path and the pair pool do not run this mode.
 * Deviations from the reference, all of them: (a) fp64 in a written order where the reference is fp32 with float atomics (GV:107-113) and
 * thrust::transform_reduce (CD:161-176) in no defined order; (b) q by V4 in fp64 (FC:55-60 casts to fp32); (c) the exact voxel set -- the
 * reference's hash table may drop up to 1 % of the points (GV:276); (d) voxels in key order, indices stored point-major (the reference:
 * offset-major, compacted, undefined order); (e) a Jacobi eigen-decomposition for Eigen's closed form; (f) NONE / NORMALIZED_MIN_EIG refused;
 * (g) the resolution is the one that was set: a GaussianVoxelMap of the reference keeps the resolution it was first built with (VC:257-263),
 * and computeTransformation overwrites the core's resolution with a member that setResolution never writes (VCI:41-43, 145) -- neither quirk
 * is reproduced; (h) GPU_RBF_KERNEL is not offered. */
typedef enum { APDGICP_VGICP_CUDA_DIRECT_RADIUS = 3 } apdgicp_vgicp_cuda_search;   /* beside APDGICP_VGICP_DIRECT1 / 7 / 27 = 0 / 1 / 2 */
typedef enum { APDGICP_NN_CPU_PARALLEL_KDTREE = 0, APDGICP_NN_GPU_BRUTEFORCE = 1, APDGICP_NN_GPU_RBF_KERNEL = 2 } apdgicp_nn_method;   /* NearestNeighborMethod, cuda/fast_vgicp_cuda.cuh */
typedef struct {
  double resolution;         /* setResolution ; default 1.0, VCI:24 ; finite and > 0 */
  int32_t neighbor_search;   /* 0 / 1 / 2 = DIRECT1 / 7 / 27, 3 = DIRECT_RADIUS ; default DIRECT1, VC:28 */
  double search_radius;      /* DIRECT_RADIUS only, in voxels ; default 1.5, VC:29 ; finite, 0 <= r <= 4 */
  int32_t regularization;    /* apdgicp_regularization ; default PLANE, VCI:26 */
  int32_t nn_method;         /* apdgicp_nn_method ; default CPU_PARALLEL_KDTREE, VCI:27 */
} apdgicp_vgicp_cuda_params;
void apdgicp_vgicp_cuda_default_params(apdgicp_vgicp_cuda_params* p);
/* p != NULL: the mode on with these parameters (checked first: a refused setting changes nothing); NULL: mode off */
int apdgicp_set_vgicp_cuda(apdgicp_handle* h, const apdgicp_vgicp_cuda_params* p);
int apdgicp_get_vgicp_cuda(const apdgicp_handle* h, apdgicp_vgicp_cuda_params* p, int* enabled);   /* either output may be NULL */
/* VC6: the offset list of p, n x 3 int32 in offset order.  Needs no handle and no device.  *n = the number of offsets; out_n3 may be NULL
 * (it holds up to 257 x 3 values). */
int apdgicp_vgicp_cuda_offsets(const apdgicp_vgicp_cuda_params* p, int32_t* out_n3, int64_t* n);
/* VC4: the kept list of cloud `which` (prepared if it is not): *n_kept, and kept_index (may be NULL; capacity >= n_kept otherwise) */
int apdgicp_vgicp_cuda_kept(apdgicp_handle* h, int which, int64_t* n_kept, int32_t* kept_index, int64_t capacity);
/* VC2 / VC3 per KEPT point of cloud `which`, host memory, either may be NULL: raw (n_kept x 6: xx, xy, xz, yy, yz, zz) and regularised
 * (n_kept x 9); capacity >= n_kept */
int apdgicp_vgicp_cuda_get_covariances(apdgicp_handle* h, int which, double* raw_n6, double* reg_n9, int64_t capacity);
/* as apdgicp_vgicp_voxel_count / _get_voxels / _get_correspondences / _build_count; correspondences: n_kept(source) x n_offsets */
int apdgicp_vgicp_cuda_voxel_count(apdgicp_handle* h, int64_t* n_voxels);
int apdgicp_vgicp_cuda_get_voxels(apdgicp_handle* h, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9);
int apdgicp_vgicp_cuda_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_kept_source);
int apdgicp_vgicp_cuda_build_count(apdgicp_handle* h, int64_t* n_builds);

/* ------------------------------------------------------------------ NDT (P2D / D2D) as a mode of the handle
 * fast_gicp::NDTCuda, the NDT the reference tree holds (the factory's own NDT_OMP fallback, registrations.cpp:101-134, is pclomp, whose
 * sources are not in the tree).  "NC:" = fast_apdgicp/src/fast_gicp/cuda/ndt_cuda.cu, "ND:" = .../cuda/ndt_compute_derivatives.cu,
 * "GV:" = .../cuda/gaussian_voxelmap.cu, "CR:" = .../cuda/covariance_regularization.cu.  The reference is fp32 throughout and leaves several
 * orders to chance: atomic float adds in accumulate_points_kernel, thrust::transform_reduce, and a hash table that may drop up to 1 % of the
 * points (GV:276).  None of that can be pinned, so -- as for voxelized GICP -- the reference's FORMULAS are evaluated in fp64, in a written
 * order, over the exact voxel set.  The deviations from the reference, all in one place:
 *     - fp64 instead of fp32 everywhere: the voxel coordinate (vector3_hash.cuh:35-38 takes it in fp32), the sums, the pose (the reference
 *       casts it to fp32), the cost;
 *     - voxels are numbered in ascending key order (the reference: atomic arrival order), sums run in the caller's order, reductions in a
 *       fixed tree / block order;
 *     - every point reaches its voxel (no hash table, no dropped points);
 *     - the symmetric eigen-decomposition of N3 is the handle's Jacobi routine, not Eigen's SelfAdjointEigenSolver;
 *     - N8 (the reference would solve a singular system).
 * The kernels (riv-slam_amd/csrc/apd_ndt.hpp) and the restatement the tests compare with (tests/ndt_np.py) follow this list:
 *   N1. Keys, range and voxel order are V1 .. V3's: c = floor(x / res - 0.5) per axis in fp64, a true division; points of a cloud that gets
 *       a map must be finite with |c| < 2^20; voxels are numbered in ascending key order.
 *   N2. Voxel statistic (GV:118-143, 174-194).  For each voxel, over its points in the caller's order, fp64 sums started at 0:
 *       S1 = sum x and S2 = sum x x^T (six unique entries); mean = S1 / n; the raw covariance is the LOWER triangle of the reference's
 *       expression, which SelfAdjointEigenSolver reads: c_rc = (S2_rc - mean_r S1_c) / n for r >= c.  Counts, means and raw covariance
 *       entries are bit-equal to a sequential loop written this way.
 *   N3. Regularisation (CR:73-87, always MIN_EIG, NC:128,139): C = V diag(max(lambda_i, 1e-3)) V^T.  The floor is absolute, not relative.
 *       A voxel with one point has raw covariance 0 and becomes 1e-3 I.
 *   N4. Two maps.  The target always gets a map, the source only in D2D (NC:120-129).  Both are pure functions of (points, resolution),
 *       separate from the voxelized-GICP map (another statistic); no k-NN covariance is involved: with the mode on apdgicp_align /
 *       apdgicp_linearize do not compute them and accept clouds smaller than k_correspondences.  Caching is by identity, as for the
 *       voxelized-GICP map: the setting of the cloud's points, the resolution.  apdgicp_swap_source_and_target swaps the maps with the
 *       clouds: in D2D with both maps built it rebuilds nothing (NC:90-93); in P2D the new target's map is built on demand.  A target
 *       point refused by V2 gives APDGICP_ERR_INVALID_ARG naming the cloud and the point, and so does a source point in D2D; in P2D a
 *       refused source point is a miss.  The handle stays usable.
 *   N5. Rows.  A row is a source voxel in voxel order (D2D: its mean is the position, its regularised covariance C_A) or a source point in
 *       the caller's order (P2D).  q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in fp64 (V4).  c(q) + each offset of DIRECT1 / DIRECT7 /
 *       DIRECT27 in the order of NC:43-68 (identical to V5's) is looked up; every hit is stored as a voxel index per (row, offset), -1 for
 *       a miss.  DIRECT_RADIUS: APDGICP_ERR_UNSUPPORTED.
 *   N6. Cost (ND:50-91, 120-163).  A hit whose target voxel has count <= 6 contributes nothing.  Otherwise M = (C_B + R_lin C_A R_lin^T)^-1
 *       (D2D; R_lin the rotation of the last linearize pose) or M = C_B^-1 (P2D), by cofactors; e = mean_B - q; w = res^2 / (res^2 + e.e),
 *       the Cauchy weight with k = resolution; cost += w e.(M e), H += w J^T M J, b += w J^T (M e), J = [skew(q) | -I].  Terms of a row are
 *       added in offset order, one row per lane in blocks of 256; lanes, waves and blocks are added in the fixed tree / block order of V5.
 *       No floating-point atomics.  n_matched is the number of contributing terms.
 *   N7. Frozen state (NC:162-177).  compute_error evaluates the same cost at the trial pose over the stored indices with R_lin of the last
 *       linearize; q, e and w come from the trial pose; M is recomputed by the same device function, as in V6.  The frozen state is tied by
 *       identity to the source's points and to the maps it was made against (otherwise APDGICP_ERR_NO_INPUT).
 *   N8. No contributing term at a linearize inside align: the loop stops there with converged = 0, lm_failed = 0, n_matched = 0 and T = the
 *       pose so far (V7's rule).  max_correspondence_distance and the APD flags have no meaning for this cost.
 *   N9. Mode rules.  Defaults: resolution 1.0, D2D, DIRECT7 (NC:15-22).  apdgicp_set_ndt and apdgicp_set_vgicp are exclusive: switching one
 *       on switches the other off; NULL returns to what apdgicp_params says.  With NDT on, apdgicp_align and apdgicp_align_host_loop both
 *       run the host-driven loop of apdgicp_align_host_loop over the two kernels (trace, final Hessian and apdgicp_result as there);
 *       apdgicp_get_correspondences / apdgicp_get_mahalanobis return APDGICP_ERR_UNSUPPORTED; the covariance calls are untouched (they
 *       compute, return or set the k-NN covariances, which this cost does not read); fitness_score, nearest_neighbours*, transform_source
 *       and get_points are unchanged.  Batch handles: N10 .. N15.  With the mode off nothing differs from a handle that never had it on.
 *
 * Batch handles have the same mode (apdgicp_batch_set_ndt, declared with the batch calls below; kernels: riv-slam_amd/csrc/apd_ndt_batch.hpp),
 * exclusive with their voxelized-GICP mode, with the optimiser loop on the device:
 *   N10. One map per cloud slot.  The map is N1 .. N3's, a pure function of the slot's points and the resolution; the same map serves the
 *       slot as a target and, in D2D, as a source.  A slot named as target_cloud by a pair of the batch gets one, in D2D a slot named as
 *       source_cloud too; in P2D a source-only slot gets none.  Coordinates, counts, means, raw and regularised covariances are bit-equal to
 *       what the single handle builds from the same points.  The map is cached by identity -- the setting of the slot's points, the
 *       resolution -- and rebuilt when either is another one, or after apdgicp_batch_clear; maps are kept across mode off / on.  Building
 *       all maps of a batch costs at most ONE host wait: buffers are sized for as many voxels as the slot has points, the voxel count stays
 *       on the device, and the words of all slots come back in one copy (V8).  A target point refused by V2 fails the align with
 *       APDGICP_ERR_INVALID_ARG, and so does a source point in D2D: the message names slot and point, no pair has run, the handle stays
 *       usable.  In P2D a refused source point is a miss.
 *   N11. No k-NN covariances.  With the mode on align does not compute them, and clouds smaller than k_correspondences align.  The
 *       clouds' curve sort still runs where the engine needs it (a staged host cloud's points are written to the device by its sort).
 *   N12. The per-row arithmetic is N5 .. N7's, bit for bit, through the same device functions the single handle's kernels call: one row per
 *       lane in blocks of 256, the 29 sums added in the written order, the block rows added in block order from 0.0.  In D2D a pair's row
 *       count is its source slot's voxel count, read on the device, never by the host.  Hence H, b, cost and n_matched of a pair's FIRST
 *       linearize equal apdgicp_linearize of a single handle at the same guess, bit for bit.
 *   N13. Optimiser.  V10's state machine with N8 in place of V7: a linearize without a contributing term ends that pair there with
 *       converged = 0, lm_failed = 0, n_linearize counted, iterations = the current iteration, T = the pose so far, final_cost = that
 *       linearize's cost, n_matched = 0.  The frozen state of N7 is per pair: the indices per (row, offset) and the pose of the pair's last
 *       linearize, whose rotation is R_lin.  sin / cos of the step's rotation come from the device library instead of the host's, so
 *       iterates agree with the single handle's to rounding, not bit for bit.
 *   N14. A pair's record is a pure function of the pair: the same (source, target, guess, parameters) gives byte-identical records whether
 *       the pair runs alone or among any others, at any position of the list, on a first align and on a reused handle.
 *   N15. No host round trip per iteration: V12 -- two launches per tick, ticks enqueued in chunks, one pinned word looked at between chunks,
 *       one chunk ahead, the same tick bound.  apdgicp_batch_align / _align_async / _copy_results / _synchronize run this path;
 *       apdgicp_batch_align_enqueue / _collect / _pump return APDGICP_ERR_UNSUPPORTED and apdgicp_batch_is_pooled returns 0;
 *       apdgicp_batch_set_pair_groups is accepted and has no effect; apdgicp_batch_fitness and the cloud calls are unchanged.
 *       apdgicp_batch_set_ndt and apdgicp_batch_set_vgicp are exclusive, as on the single handle: switching one on switches the other
 *       off.  With the mode off a batch handle does exactly what one that never had it on does. */
typedef enum { APDGICP_NDT_P2D = 0, APDGICP_NDT_D2D = 1 } apdgicp_ndt_distance;   /* NDTDistanceMode, ndt_settings.hpp */
#define APDGICP_NDT_DIRECT_RADIUS 3   /* NeighborSearchMethod::DIRECT_RADIUS as a value of neighbor_search: refused (N5) */
typedef struct {
  double resolution;         /* setResolution ; default 1.0 ; finite and > 0 */
  int32_t distance_mode;     /* apdgicp_ndt_distance ; default D2D */
  int32_t neighbor_search;   /* apdgicp_vgicp_search ; default DIRECT7 */
} apdgicp_ndt_params;
void apdgicp_ndt_default_params(apdgicp_ndt_params* p);                          /* 1.0, D2D, DIRECT7: NC:15-22 */
/* p != NULL: the mode on with these parameters (and voxelized GICP off); NULL: back to what apdgicp_params says */
int apdgicp_set_ndt(apdgicp_handle* h, const apdgicp_ndt_params* p);
int apdgicp_get_ndt(const apdgicp_handle* h, apdgicp_ndt_params* p, int* enabled);   /* either output may be NULL */
/* number of voxels of the map of `which` (APDGICP_SOURCE / APDGICP_TARGET; built if it is not there; needs that cloud only) */
int apdgicp_ndt_voxel_count(apdgicp_handle* h, int which, int64_t* n_voxels);
/* that map in voxel order (N1), host memory, any pointer may be NULL: coordinates (n x 3), counts, means (n x 3), raw covariances of N2
 * (n x 6: xx, yx, zx, yy, zy, zz), regularised covariances of N3 (n x 9, the 3x3 block); capacity >= the voxel count */
int apdgicp_ndt_get_voxels(apdgicp_handle* h, int which, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* raw_covs_n6, double* covs_n9);
/* the stored indices of the last linearize: n_rows x n_offsets target voxel indices in offset order, -1 = miss; n_rows = the source's
 * voxel count (D2D) or point count (P2D) */
int apdgicp_ndt_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_rows);
/* Debug: how many voxel maps (of either cloud) this handle has built in this mode (the tests of the cache rules read it) */
int apdgicp_ndt_build_count(apdgicp_handle* h, int64_t* n_builds);

/* ------------------------------------------------------------------ point-to-point ICP as a mode of the handle
 * pcl::IterativeClosestPoint, the ICP branch of select_registration_method() (registrations.cpp:71-78).  PCL is not under the reference tree, so
 * nothing below can be cited by line: the source is PCL 1.10 "as published", unpinned like the filters (DESIGN.md sections 4 and 5) --
 * registration/impl/icp.hpp, correspondence_estimation.hpp, default_convergence_criteria.hpp and transformation_estimation_svd.hpp with
 * Eigen >= 3.3's umeyama.  The kernels (riv-slam_amd/csrc/apd_icp.hpp) and the restatement the tests compare with (tests/icp_np.py) follow
 * this list:
 *   IC1. Working cloud.  W0 = guess * source, or the source itself when the guess is the identity.  Each iteration replaces W by T_k * W in
 *        fp32, in place; the order of T * p is the handle's: pairwise by default, APDGICP_FLAG_XF_LINEAR_CHAIN otherwise.  W is never
 *        recomputed from the source.  Non-finite source points take no part: they have no match, are nobody's reciprocal neighbour, and
 *        come back as NaN from apdgicp_icp_get_working_cloud.
 *   IC2. Forward correspondences.  For every point of W its nearest target point with the fp32 squared distance in the engine's L2_Simple
 *        order ((dx dx + dy dy) + dz dz over d = target - W); a tie resolves to the lowest target index.  A point is rejected iff
 *        (double)d2 > max_correspondence_distance^2, the product taken in fp64; equality is kept.
 *   IC3. Reciprocal correspondences (use_reciprocal_correspondences).  A forward match (i, j) is kept iff the nearest point of W to target[j]
 *        is i, and that distance also passes the gate of IC2.  Same fp32 arithmetic (the same expression, so the reciprocal distance of a
 *        kept pair is the forward one); a tie resolves to the lowest index of W in the caller's order.  The stored distance is the forward one.
 *   IC4. Minimum.  Fewer than min_correspondences (default 3) matches give state NO_CORRESPONDENCES; the loop stops with converged = 0 and
 *        T = the product so far, which is the guess if this happens at the first iteration.
 *   IC5. Estimation (Umeyama without scaling).  pm, qm = the means of the matched W points and target points; Sigma = (1/n) sum (q - qm)(p - pm)^T,
 *        Sigma = U D V^T, S = diag(1, 1, sign(det U det V)), R = U S V^T, t = qm - R pm.  Everything in fp64 from the fp32 coordinates, two
 *        passes, sums in a fixed order (lanes by a fixed tree, waves and blocks in index order).  T_k is the fp32 rounding of the result; a
 *        non-finite T_k stops the loop with converged = 0.  STATED DEVIATION: PCL sums in fp32 in Eigen's vectorised order, which cannot be
 *        pinned.  The SVD is a one-sided Jacobi iteration, not Eigen's JacobiSVD; with fewer than two non-zero singular values R is not
 *        unique (Sigma = 0 gives R = I).
 *   IC6. Accumulation.  final = T_k * final as an fp32 4x4 product, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3 without contraction
 *        (STATED DEVIATION: Eigen's order for this product is its own).  nr_iterations is then incremented, so in this mode
 *        apdgicp_result.iterations is a COUNT, not a zero-based index.
 *   IC7. Convergence (DefaultConvergenceCriteria), in this order: iterations >= max_iterations -> ITERATIONS, converged = 1.  With
 *        cos = 0.5 (T00 + T11 + T22 - 1) and t2 = T03^2 + T13^2 + T23^2 of T_k in fp64 the step is similar if cos >= rot_thr and
 *        t2 <= transformation_epsilon (NOT squared, as there); rot_thr = rotation_epsilon if rotation_epsilon > 0, else
 *        1 - transformation_epsilon -> TRANSFORM.  mse = the fp64 mean of the kept fp32 d2; |mse - prev| < mse_threshold_absolute (default
 *        1e-12) -> ABS_MSE; |mse - prev| / prev < euclidean_fitness_epsilon (default -DBL_MAX: never) -> REL_MSE.  Each of the three tests
 *        fires only once iterations_similar_transforms >= max_similar_transforms (default 0), otherwise it counts the iteration as similar;
 *        the counter is incremented when the iteration was similar and reset otherwise.  prev starts at DBL_MAX.
 *   IC8. Result.  T = final; final_cost = the mse of the last iteration's matches (0 without a match); n_matched = the last count (saturating);
 *        iterations = n_linearize = the iteration count; n_compute_error = 0, lm_failed = 0.  apdgicp_icp_convergence_state reads the state.
 *        After an align W has had every T_k of the trace applied.
 *   IC9. Mode rules.  apdgicp_set_icp, apdgicp_set_vgicp and apdgicp_set_ndt are exclusive: switching one on switches the others off, as in
 *        N9.  No covariances are computed, clouds of any size >= 1 are accepted.  apdgicp_linearize, apdgicp_compute_error,
 *        apdgicp_get_final_hessian (and apdgicp_get_correspondences / apdgicp_get_mahalanobis) answer APDGICP_ERR_UNSUPPORTED;
 *        apdgicp_align_host_loop runs the same loop as apdgicp_align.  apdgicp_fitness_score, apdgicp_inlier_fraction,
 *        apdgicp_nearest_neighbours*, apdgicp_transform_source, swap and clear keep working.  With the mode off the handle's APD / GICP
 *        results are bit for bit what they were.
 *   IC10. Determinism.  The same inputs give the same bytes on every run; no floating-point atomics.
 *
 * Batch handles have the same mode (apdgicp_batch_set_icp, declared with the batch calls below; kernels: riv-slam_amd/csrc/apd_icp_batch.hpp),
 * exclusive with their voxelized-GICP and NDT modes, with the loop on the device:
 *   IC11. Working cloud per pair.  Every pair owns a working cloud W, a slice of one buffer of sum(n_source) x 16 bytes, initialised by IC1
 *        from the pair's source slot and the pair's guess.  Two pairs may share a source slot and a target slot, and a pair may name the same
 *        slot as source and target.  Nothing of a slot is written.
 *   IC12. Arithmetic.  The per-iteration arithmetic is IC2 .. IC7, bit for bit, through the same device functions the single handle's kernels
 *        call: the engine's exact search with W in place of the sorted source at the identity pose, cold every iteration (W moves while the
 *        pose stays the identity, so a kept neighbour would be unproven); the same gate; the same reciprocal test, pruned or
 *        APDGICP_ICP_RECIP_MODE=brute; one point per lane in blocks of 256; lane, wave and block sums in the written order; the block rows
 *        added in block order from 0.0 over the pair's own ceil(n / 256) rows only; the one-lane step.
 *   IC13. Records.  A pair's apdgicp_result, its convergence state, trace, last correspondences and final W are byte-identical to what
 *        apdgicp_align of a single handle returns for the same (source, target, guess, parameters, flags).  No host arithmetic is left that
 *        could differ.  The trace keeps a pair's first 1024 iterations; the count goes on.
 *   IC14. Purity.  The same pair gives the same bytes alone or among others, at any position of the list, on a first align and on a reused
 *        handle.
 *   IC15. Device loop.  No host round trip per iteration.  One tick of the whole batch is a fixed number of launches (7 forward, 10
 *        reciprocal, 8 with the brute reciprocal search) that depends neither on n_pairs nor on n: the pair is a grid dimension of every
 *        kernel, the two box passes and the reciprocal search included.  Ticks are enqueued in chunks as in V12, one pinned word looked at
 *        between chunks, one chunk ahead.  T_k is applied to W exactly once per iteration, the last included; a finished pair's blocks exit
 *        on reading its status and the engine's search skips it.  The tick bound is max(1, max_iterations), the iterations the single handle
 *        runs at most.  optimizer, the LM fields and k_correspondences have no meaning in this mode; no covariances are computed, and clouds
 *        of any size >= 1 align.  A pair stopped by IC4 at its first iteration returns T = guess and iterations = 0 while the others go on.
 *   IC16. Mode rules.  apdgicp_batch_set_icp, apdgicp_batch_set_vgicp and apdgicp_batch_set_ndt are exclusive: switching one on switches the
 *        others off.  apdgicp_batch_align / _align_async / _copy_results / _synchronize run this path; apdgicp_batch_align_enqueue /
 *        _collect / _pump return APDGICP_ERR_UNSUPPORTED and apdgicp_batch_is_pooled returns 0; apdgicp_batch_set_pair_groups is accepted
 *        and has no effect; apdgicp_batch_last_ticks reports the ticks.  apdgicp_batch_fitness with T == NULL scores the poses of the ICP
 *        align, i.e. the records' T; with explicit T it is unchanged.  With the mode off a batch handle does exactly what one that never had
 *        it on does.
 * Not built: the pair pool and the sharded path in this mode; correspondence rejectors; point-to-plane; PCL's own GICP / NDT. */
typedef enum {
  APDGICP_ICP_NOT_CONVERGED = 0,
  APDGICP_ICP_ITERATIONS = 1,
  APDGICP_ICP_TRANSFORM = 2,
  APDGICP_ICP_ABS_MSE = 3,
  APDGICP_ICP_REL_MSE = 4,
  APDGICP_ICP_NO_CORRESPONDENCES = 5
} apdgicp_icp_state;   /* DefaultConvergenceCriteria::ConvergenceState, same numeric values */
typedef struct {
  int32_t enable;                          /* apdgicp_set_icp: non-zero switches the mode on, 0 stores the parameters and switches it off */
  int32_t use_reciprocal_correspondences;  /* setUseReciprocalCorrespondences ; default 0 */
  int32_t min_correspondences;             /* min_number_correspondences_ ; default 3 ; >= 1 */
  int32_t max_similar_transforms;          /* setMaximumIterationsSimilarTransforms ; default 0 ; >= 0 */
  double euclidean_fitness_epsilon;        /* setEuclideanFitnessEpsilon ; default -DBL_MAX (never) */
  double rotation_epsilon;                 /* setTransformationRotationEpsilon ; default 0: 1 - transformation_epsilon is used */
  double mse_threshold_absolute;           /* DefaultConvergenceCriteria::setAbsoluteMSE ; default 1e-12 */
} apdgicp_icp_params;
/* max_iterations, transformation_epsilon, max_correspondence_distance and flags stay in apdgicp_params, where pcl::Registration keeps them */
void apdgicp_icp_default_params(apdgicp_icp_params* p);   /* enable = 1 and the defaults above */
/* p != NULL with p->enable: the mode on with these parameters (voxelized GICP and NDT off); NULL or enable = 0: back to what apdgicp_params says */
int apdgicp_set_icp(apdgicp_handle* h, const apdgicp_icp_params* p);
int apdgicp_get_icp(const apdgicp_handle* h, apdgicp_icp_params* p, int* enabled);   /* either output may be NULL */
/* The per-iteration probe, this mode's linearize: W = T * source (the source itself when T is the identity), then IC2 .. IC5.  T_out = T_k
 * (column-major; the identity when IC4 or a non-finite result refused the estimate), *n_corr the matches, *mse their fp64 mean d2, and
 * sums[16] the reduction: [0] sum d2; [1..3] sum p; [4..6] sum q; [7..15] sum (q - qm)(p - pm)^T row-major (row: q, column: p) -- NOT
 * divided by n; p runs over the matched points of W, q over their target points.  Any output may be NULL.  Nothing is accumulated (no IC6 / IC7). */
int apdgicp_icp_estimate(apdgicp_handle* h, const float T[16], float T_out[16], int64_t* n_corr, double* mse, double sums[16]);
/* the matches of the last estimate or of the last iteration of the last align, in the caller's source order: target index or -1 for a
 * rejected point; sq_dist the forward fp32 d2 of every finite point whether kept or not (NaN for a non-finite one).  n = the source size. */
int apdgicp_icp_get_correspondences(apdgicp_handle* h, int32_t* match, float* sq_dist, int64_t n);
/* W in the caller's order, n x 3 floats */
int apdgicp_icp_get_working_cloud(apdgicp_handle* h, float* xyz, int64_t n);
/* the iterations of the last align, one entry each (the first min(capacity, *n_iterations) are written; any array may be NULL): T_k,
 * the matches, their mse, iterations_similar_transforms after the iteration.  An iteration stopped by IC4 has T_k = identity. */
int apdgicp_icp_get_trace(apdgicp_handle* h, int64_t capacity, float* T_k16, int64_t* n_corr, double* mse, int32_t* similar, int64_t* n_iterations);
int apdgicp_icp_convergence_state(apdgicp_handle* h, int32_t* state);   /* apdgicp_icp_state of the last align (NOT_CONVERGED before any) */
/* Debug: launches and host waits of the last align in this mode (tests/measure/bench_icp.py) */
int apdgicp_icp_debug_counts(apdgicp_handle* h, int64_t* launches, int64_t* waits);

/* ------------------------------------------------------------------ FastGICPMultiPoints as a mode of the handle
 * fast_gicp::FastGICPMultiPoints (fast_gicp/gicp/experimental/fast_gicp_mp.hpp and fast_gicp_mp_impl.hpp, "MPI:n" below): GICP with many
 * correspondences per point -- every source point takes ALL target points inside neighbor_search_radius, fuses their means and covariances
 * with distance weights into one distribution, and a plain Gauss-Newton loop minimises the whitened residuals.  The consumer of the radius
 * queries of section Q.  The reference marks the class experimental and keeps it out of its library target; on sparse scenes it may run to
 * max_iterations and end decimetres from the truth.  The bar here is parity with a literal restatement (tests/gicp_mp_np.py), not accuracy,
 * and nothing of the algorithm is "fixed": not its cost |M d|^2, not its translation update.  The kernels (riv-slam_amd/csrc/apd_gicp_mp.hpp
 * over apd_search.hpp) and the restatement follow this list:
 *   MP1. Clouds and covariances.  Both clouds need n >= k_correspondences points (MPI:233-239 reads uninitialised columns otherwise);
 *        a smaller cloud is APDGICP_ERR_TOO_FEW_POINTS.  The covariances are the handle's own: those of apdgicp_compute_covariances /
 *        apdgicp_get_covariances, or what apdgicp_set_covariances stored.  MPI:242 forms the scatter matrix without dividing by k; PLANE
 *        (MPI:258-260, the constructor's default) and NORMALIZED_MIN_EIG (MPI:264-267) do not depend on that scale, so the engine's bytes are
 *        the mode's covariances.  MIN_EIG and FROBENIUS act on the undivided scatter and would differ, NONE reaches abort (MPI:255-257): all
 *        three are APDGICP_ERR_UNSUPPORTED, checked when the mode is switched on and at every linearize / align; nothing changes on a
 *        refusal.  STATED DEVIATION: the reference uses an fp32 JacobiSVD<Matrix3f>, the engine its fp64 symmetric eigen-decomposition.
 *   MP2. Queries.  q_i = T_f * p_i in fp32, T_f the fp32 rounding of the fp64 pose (MPI:131-141), in the handle's transform order
 *        (pairwise, or APDGICP_FLAG_XF_LINEAR_CHAIN): the point the APD path searches with.
 *   MP3. Rows.  The row of source point i is exactly the row that apdgicp_radius_search_of defines for q_i, neighbor_search_radius and
 *        max_nn = 0: Q1's distance and key, Q4's r2 = (float)(r * r) and d2 < r2 strictly, Q5's ascending key.  A non-finite source point
 *        (or one whose q is not finite) has an empty row.  STATED DEVIATION: PCL's tie order is unspecified.
 *   MP4. Fusion (MPI:180-195).  Per non-empty row, in fp64, in row order, sums started at 0.0: w_j = max(1e-3, min(1.0, 1.0 -
 *        (double)sqrtf(d2_j) / r)) -- the square root in fp32, the division in fp64, as written; sw += w; sm += w * (double)t_j;
 *        sc += w * C_B[j] over the six unique entries, every product rounded before it is added (no contraction).  mean_B = sm / sw and
 *        cov_B = sc / sw as true divisions.  STATED DEVIATION: the reference rounds both to fp32 and continues in fp32 (MPI:194-209); from
 *        here on everything is fp64.
 *   MP5. Terms (MPI:197-213).  Ta = R a + t from (double)p_i with the fp64 pose, each row ((r0 x + r1 y) + r2 z) + t; d = mean_B - Ta;
 *        RCR = cov_B + R C_A R^T; M = RCR^-1, the 3x3 inverse that the 4x4 inverse of MPI:199-202 contains; l = M d; J = M [skew(Ta) | -I],
 *        3x6 with the rotation block first (so3.hpp:9-19).  H += J^T J, g += J^T l, cost += l^T l, n_matched += 1.  The cost is |M d|^2, not
 *        d^T M d: as the reference writes it.  Sums in the handle's written order: lanes by a fixed tree, waves and blocks in index order.
 *   MP6. Step.  delta solves H delta = g with the 6x6 LDL^T of the host loop, no damping (the normal equations GaussNewton::delta names;
 *        fast_gicp/opt/gauss_newton.hpp is not under the reference tree, so the solver is unpinned).  R <- so3_exp(-delta_r) R and
 *        t <- t - delta_t (MPI:101-102): the translation is not rotated, this is not an SE(3) product.  STATED DEVIATION: the reference
 *        keeps the pose as an fp32 rotation vector and goes through Sophus log / exp every iteration; here R and t are fp64 and start as
 *        the guess's blocks, widened, without re-orthonormalisation.
 *   MP7. Loop (MPI:92-108).  For i = 0 .. max_iterations - 1: iterations = i; linearize at the pose; n_matched < 2 stops with converged =
 *        0, the pose unchanged, state TOO_FEW_ROWS (H has rank <= 3 per row, a solve decides nothing; STATED DEVIATION: the reference solves
 *        anyway and draws a random step); a non-finite entry of delta stops the same way with state SINGULAR; else delta is applied and
 *        converged = is_converged over so3_exp(delta_r) - I and delta_t with rotation_epsilon and transformation_epsilon (L:83-92's
 *        expression).  Result: T the fp32 pose, iterations the zero-based index of the last iteration, n_linearize = iterations + 1,
 *        n_compute_error = 0, final_cost and n_matched those of the last linearize, lm_failed = 0.  optimizer, the LM fields and
 *        max_correspondence_distance (MPI:34, never read) have no meaning in this mode.
 *   MP8. Defaults of the class (MPI:27-35): k 20, max_iterations 64, rotation_epsilon 1e-5, transformation_epsilon 1e-5, PLANE, radius 0.5.
 *        The ABI reads apdgicp_params as set; the Python class and the C++ class set these defaults.
 *   MP9. Mode rules.  Exclusive with the four other modes as in IC9 / N9.  apdgicp_linearize returns H, b = g and the cost of MP5;
 *        apdgicp_get_final_hessian the last H (identity before any).  apdgicp_compute_error, apdgicp_get_correspondences and
 *        apdgicp_get_mahalanobis are APDGICP_ERR_UNSUPPORTED; apdgicp_align_host_loop runs the same loop as apdgicp_align.  Fitness, inlier
 *        fraction, the nearest-neighbour and Q calls, apdgicp_transform_source, swap and clear keep working; the rows live in buffers of the
 *        mode's own, so a Q call between two linearizes changes nothing of its results (Q7).  With the mode off the handle returns the
 *        bytes it returned before, and the getters below answer APDGICP_ERR_NO_INPUT.
 *   MP10. Probes.  The rows of the last linearize come back in two calls as in Q6; per source point in the caller's order sum_w, mean_B[3]
 *        and cov_B[6] (xx, xy, xz, yy, yz, zz; zeros for an empty row); the trace of the last align, per iteration the pose before the step
 *        (4x4 fp64, column-major), the cost, n_matched and delta[6] (zeros where TOO_FEW_ROWS stopped it); the end state; launches and host
 *        waits since the start of the last align.  A linearize waits twice: behind the total that sizes the rows, and behind the sums.
 *   MP11. Determinism.  The same bytes on every run; no floating-point atomics; a point's fused terms are a pure function of (target, its
 *        covariances, q_i, r).
 * Not built in this mode: batch handles, the loop verifier, the sharded path and the pair pool; MIN_EIG / FROBENIUS on the undivided scatter;
 * a device-side loop; a cooperative (wave per row) form of the fusion. */
typedef enum {
  APDGICP_GICP_MP_NOT_CONVERGED = 0,   /* ran to max_iterations (or no align yet) */
  APDGICP_GICP_MP_CONVERGED = 1,
  APDGICP_GICP_MP_TOO_FEW_ROWS = 2,
  APDGICP_GICP_MP_SINGULAR = 3
} apdgicp_gicp_mp_state_t;
typedef struct {
  int32_t enable;                  /* apdgicp_set_gicp_mp: non-zero switches the mode on, 0 stores the parameters and switches it off */
  int32_t reserved;                /* 0 */
  double neighbor_search_radius;   /* MPI:35 ; default 0.5 ; finite and > 0.  The reference has no setter for it: the one extension */
} apdgicp_gicp_mp_params;
void apdgicp_gicp_mp_default_params(apdgicp_gicp_mp_params* p);   /* enable = 1, radius 0.5 */
/* p != NULL with p->enable: the mode on with these parameters (the other modes off); NULL or enable = 0: back to what apdgicp_params says.
 * A radius that is not finite and positive: APDGICP_ERR_INVALID_ARG, checked before the handle. */
int apdgicp_set_gicp_mp(apdgicp_handle* h, const apdgicp_gicp_mp_params* p);
int apdgicp_get_gicp_mp(const apdgicp_handle* h, apdgicp_gicp_mp_params* p, int* enabled);   /* either output may be NULL */
/* MP10: the rows of the last linearize (of apdgicp_linearize or of the last iteration of an align), while source and target are the
 * clouds it ran on.  row_start[0 .. n], n = the source size, *total = row_start[n]; then `total` entries: index into the target as set and
 * the fp32 d2 */
int apdgicp_gicp_mp_get_rows(apdgicp_handle* h, int64_t* row_start /* n + 1 */, int64_t n, int64_t* total);
int apdgicp_gicp_mp_get_row_entries(apdgicp_handle* h, int32_t* index, float* sq_dist);
/* of the same linearize, per source point in the caller's order; any output may be NULL */
int apdgicp_gicp_mp_get_fused(apdgicp_handle* h, double* sum_w /* n */, double* mean_B /* n x 3 */, double* cov_B /* n x 6 */, int64_t n);
/* the iterations of the last align, one entry each (the first min(capacity, *n_iterations) are written; any array may be NULL) */
int apdgicp_gicp_mp_get_trace(apdgicp_handle* h, int64_t capacity, double* pose16, double* cost, int64_t* n_matched, double* delta6, int64_t* n_iterations);
int apdgicp_gicp_mp_state(apdgicp_handle* h, int32_t* state);   /* apdgicp_gicp_mp_state_t of the last align */
int apdgicp_gicp_mp_debug_counts(apdgicp_handle* h, int64_t* launches, int64_t* waits);
/* Measurement (tests/measure/bench_gicp_mp.py): with profiling on, a linearize records events at its phase boundaries, in a series of their
 * own, and the times of the last one come back in ms: transform, count (with the mask and the total), scan, fill, row sort, the per-point
 * kernel (with the block sums).  Off by default; results are the same bytes either way. */
int apdgicp_gicp_mp_set_profiling(apdgicp_handle* h, int enable);
int apdgicp_gicp_mp_last_phases(apdgicp_handle* h, double ms[6]);

/* ------------------------------------------------------------------ batched registrations
 * Independent (source, target) pairs -- loop-closure candidates (loop_detector.cpp:222-236,404-423)
 * or one scan against several keyframes -- solved concurrently on one GPU.  Clouds are registered
 * once and referenced by index, so a cloud shared by many pairs has its covariances computed once. */
typedef struct {
  int32_t source_cloud;
  int32_t target_cloud;
  float guess[16];            /* column-major */
} apdgicp_pair;

int apdgicp_batch_create(const apdgicp_params* p, int device, void* stream, apdgicp_batch** out);
int apdgicp_batch_destroy(apdgicp_batch* b);
int apdgicp_batch_set_params(apdgicp_batch* b, const apdgicp_params* p);
/* drops all clouds (and their covariances) */
int apdgicp_batch_clear(apdgicp_batch* b);
/* returns the cloud's index (>= 0) or a negative status */
int apdgicp_batch_add_cloud(apdgicp_batch* b, const float* xyz, int64_t n, int64_t stride_bytes, int on_device);
/* sets cloud slot `index` (>= 0; slots need not be contiguous: a caller that keeps several batches in flight gives each its own
 * range), reusing the slot's device buffers; its covariances are recomputed by the next align */
int apdgicp_batch_set_cloud(apdgicp_batch* b, int32_t index, const float* xyz, int64_t n, int64_t stride_bytes, int on_device);
/* sets clouds first_index .. first_index+count-1 in one call: xyz[i] / n[i] describe cloud first_index+i, all with the same stride.
 * on_device: one pack launch.  Host clouds (four or more, 32 k points or more in all): packed by a few host threads
 * (APDGICP_HOST_THREADS, default 4, the caller included; ONE pool per process, sized when first used) into one pinned region, ONE asynchronous copy, one pack launch; the
 * caller's buffers are free on return */
int apdgicp_batch_set_clouds(apdgicp_batch* b, int32_t first_index, int32_t count, const float* const* xyz, const int64_t* n,
                             int64_t stride_bytes, int on_device);
/* covariances of every cloud that does not have them yet (align does this lazily as well) */
int apdgicp_batch_compute_covariances(apdgicp_batch* b);
/* aligns all pairs; results[i] belongs to pairs[i].  `results` is host memory. */
int apdgicp_batch_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, apdgicp_result* results);
/* same, but results stay on the device (n_pairs x sizeof(apdgicp_result) bytes at *d_results,
 * owned by the batch, valid until the next align) and the call does not wait: for callers that
 * gather results with RCCL.  apdgicp_batch_synchronize() waits for the stream. */
int apdgicp_batch_align_async(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, void** d_results);
int apdgicp_batch_synchronize(apdgicp_batch* b);
int apdgicp_batch_wait_producer(apdgicp_batch* b, void* producer_stream);   /* see apdgicp_wait_producer */
int apdgicp_batch_get_stream(apdgicp_batch* b, void** stream);              /* see apdgicp_get_stream */
/* A stream of batches (one per keyframe, loop_detector.cpp:222-236) with several of them in flight on ONE handle and ONE host
 * thread: enqueue prepares the clouds set since the last call (packing, sorting, covariances), hands the batch to the device and
 * returns without waiting; collect(ticket) waits for that batch, reports its error if it had one, and hands out its records:
 * *d_results (device, n_pairs x sizeof(apdgicp_result)) and/or host_results (either may be NULL).  Collecting is optional.
 *   Gauss-Newton (the run length is known): every tick and the final poll are enqueued at once; TWO batches may be in flight, the
 *   next batch may reuse the same cloud slots (stream order), and a ticket stays collectable until the SECOND enqueue after its own.
 *   Levenberg-Marquardt (the reference's default, L:17; the run length is data dependent, L:64-76): the pairs of up to TWENTY-FOUR
 *   batches (APDGICP_POOL_LANES, at most 32; apdgicp_batch_is_pooled reports the number) share one pool of pair slots on the device; every optimiser tick is one launch over the pairs of all batches that
 *   still run, pairs leave as they converge and the pairs of the next batch join between two ticks, so a batch is never held
 *   by the slowest pair of another one and the GPU never waits for the host (ticks are enqueued two chunks ahead by whichever
 *   call of the handle is running; collect pumps until its batch is done).  A ticket stays collectable until its lane is
 *   needed again: the twenty-fourth enqueue after its own at the latest (a batch with more pairs or larger clouds than any before makes
 *   the pool lay itself out anew; the device record pointer of an EARLIER ticket collected after that is a copy of its
 *   host records, not a view of the pool).  A cloud slot referenced by a batch in flight must not be
 *   replaced -- set_cloud(s) on such a slot first waits for that batch -- so callers that want overlap give consecutive batches
 *   disjoint slot ranges (keyframe clouds that stay registered are shared freely).  If a covariance launch raises the device
 *   error flag, every batch in flight at that moment fails at its collect; the handle stays usable.
 *   APDGICP_LM_POOL=0 in the environment selects the round-2 host-polled loop instead (the cross-check of tests/test_lm_pool.py). */
int apdgicp_batch_align_enqueue(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, uint64_t* ticket);
/* Serves the Levenberg-Marquardt pair pool without waiting: reads the polls that have arrived and keeps the chunks of ticks
 * enqueued ahead.  Every call of the handle does this anyway; a caller that goes away for more than a few hundred microseconds
 * between calls while batches are in flight (a worker thread waiting for its next job) calls this in between so that the GPU
 * does not run out of enqueued ticks.  No-op for Gauss-Newton handles and when nothing is in flight. */
int apdgicp_batch_pump(apdgicp_batch* b);
/* > 0 when apdgicp_batch_align_enqueue runs batches through the pair pool with the handle's current parameters (Levenberg-Marquardt,
 * pruned search, APDGICP_LM_POOL != 0): the number of batches that may be in flight on this one handle (24 unless
 * APDGICP_POOL_LANES says otherwise); 0: two record buffers, one batch at a time per handle for LM.  For callers that choose their
 * pipelining accordingly (ShardedBatchAlignerHip). */
int apdgicp_batch_is_pooled(apdgicp_batch* b);
/* A batch runs as up to three pair groups on three HIP streams (about 8 pairs per group), which is the best a single handle
 * can do.  A caller that keeps several HANDLES busy at once -- batch s on handle s % 3, each enqueued before the previous
 * ones are collected -- does better with one group (= one stream, larger launches) per handle: one handle's covariance
 * phase then fills the latency gaps of the others' optimiser ticks (bench.py: 1.70 -> 1.30 ms per batch of 32). */
int apdgicp_batch_set_pair_groups(apdgicp_batch* b, int max_groups);
int apdgicp_batch_align_collect(apdgicp_batch* b, uint64_t ticket, void** d_results, apdgicp_result* host_results);
/* pcl getFitnessScore(max_range) of every pair at the given poses (T: n_pairs x 16 floats, column-major;
 * NULL = the poses found by the last align of the same pair list -- APDGICP_ERR_NO_INPUT when there is none, when a cloud of the
 * list was set again since, or when a call with explicit poses has come between): mean squared nearest-neighbour distance of the
 * transformed source over the points with squared distance <= max_range, DBL_MAX when none qualifies.  One NN launch
 * for the whole batch -- the per-candidate getFitnessScore of LoopDetector::matching (loop_detector.cpp:415).
 * inliers may be NULL. */
int apdgicp_batch_fitness(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, const float* T, double max_range,
                          double* scores, int64_t* inliers);
/* copies the n_pairs result records of the last align into caller memory (device pointer when
 * dst_on_device != 0, e.g. a tensor that RCCL will all-gather) and waits for the copy */
int apdgicp_batch_copy_results(apdgicp_batch* b, void* dst, int64_t n_pairs, int dst_on_device);
/* Measurement hooks (bench.py's roofline leg).  With profiling enabled, launches of the dominant kernel (the
 * nearest-neighbour search) carry their own start/stop events (hipExtLaunchKernelGGL: the kernel's begin and end
 * timestamps on the stream it runs on); last_nn_time returns their summed milliseconds and the launch count for
 * the last align; last_ticks returns the number of state-machine ticks and the launch shape that was used. */
int apdgicp_batch_set_profiling(apdgicp_batch* b, int enable);
int apdgicp_batch_last_nn_time(apdgicp_batch* b, double* total_ms, int64_t* launches);
/* same, plus the number of pairs the timed launches covered (a launch covers one pair group; only every 10th tick is
 * timed, with a phase rotating from align to align, because timing every launch costs ~5 % of a step).  Pooled LM batches:
 * the timed launches (the first tick of every 10th chunk, per list slice) belong to no single batch -- the call returns what
 * has been harvested since the previous call and resets it; pairs_covered counts the pairs really on the list, not the slots */
int apdgicp_batch_last_nn_profile(apdgicp_batch* b, double* total_ms, int64_t* launches, int64_t* pairs_covered);
int apdgicp_batch_last_ticks(apdgicp_batch* b, int* ticks, int* nn_sources_per_lane, int* nn_target_splits);
/* name of the nearest-neighbour kernel the last launch used (e.g. "k_nn_compact<4>", "(k_nn_pruned<1, 8>)", "k_nn_partial<4>") */
int apdgicp_batch_last_nn_kernel(apdgicp_batch* b, char* name, int capacity);
/* pruning diagnostics, collected only when the environment has APDGICP_STATS=1 (else zeros); reading
 * resets them.  [0..3] nearest neighbour: groups scanned, chunks tested, chunks scanned, waves;
 * [4..9] covariance k-NN: groups loaded, (NN: batches of 64 group boxes visited), (NN: points that kept their neighbour without a search), waves sampled, list tightenings, (query, group) steps;
 * [10..15] sampled phase timers (s_memtime ticks) of whichever of the two kernels ran last (tools/prune_stats.py, tools/knn_time.py) */
/* Measurement: what the pair pool of a Levenberg-Marquardt batch handle has enqueued since it was created -- chunks (polls), ticks, and
 * slot-ticks = the sum over the tick launches of the pair slots they covered (grid y; slots behind the end of a list execute nothing).
 * bench.py turns per-slot counter profiles into a per-batch figure with it (the LM line's valu_busy).  Zeros for a handle without a pool. */
int apdgicp_batch_pool_counters(apdgicp_batch* b, int64_t* chunks, int64_t* ticks, int64_t* slot_ticks);

/* Voxelized GICP as a mode of the batch handle: V8 .. V12 above.  p != NULL: the mode on with these parameters (MULTIPLICATIVE:
 * APDGICP_ERR_UNSUPPORTED, V7); NULL: mode off.  The maps built so far are kept across off / on. */
int apdgicp_batch_set_vgicp(apdgicp_batch* b, const apdgicp_vgicp_params* p);
int apdgicp_batch_get_vgicp(const apdgicp_batch* b, apdgicp_vgicp_params* p, int* enabled);   /* either output may be NULL */
/* number of voxels of the map of cloud slot `cloud` (built if it is not current; needs the mode on and that slot only) */
int apdgicp_batch_vgicp_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels);
/* that map in voxel order, as apdgicp_vgicp_get_voxels */
int apdgicp_batch_vgicp_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9);
/* Debug: how many voxel maps this handle has built, all slots together (the tests of the cache rules read it) */
int apdgicp_batch_vgicp_build_count(apdgicp_batch* b, int64_t* n_builds);
/* NDT as a mode of the batch handle: N10 .. N15 above.  p != NULL: the mode on with these parameters (and voxelized GICP off; DIRECT_RADIUS:
 * APDGICP_ERR_UNSUPPORTED); NULL: mode off.  The parameters are checked before the handle.  The maps built so far are kept across off / on. */
int apdgicp_batch_set_ndt(apdgicp_batch* b, const apdgicp_ndt_params* p);
int apdgicp_batch_get_ndt(const apdgicp_batch* b, apdgicp_ndt_params* p, int* enabled);   /* either output may be NULL */
/* number of voxels of the map of cloud slot `cloud` (built if it is not current; needs the mode on and that slot only) */
int apdgicp_batch_ndt_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels);
/* that map in voxel order, as apdgicp_ndt_get_voxels */
int apdgicp_batch_ndt_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* raw_covs_n6,
                                 double* covs_n9);
/* Debug: how many NDT voxel maps this handle has built, all slots together (the tests of the cache rules read it) */
int apdgicp_batch_ndt_build_count(apdgicp_batch* b, int64_t* n_builds);
/* Point-to-point ICP as a mode of the batch handle: IC11 .. IC16 above.  p != NULL with p->enable: the mode on with these parameters (batch
 * voxelized GICP and NDT off); NULL or enable = 0: mode off (a non-NULL p is stored).  The parameters are checked before the handle. */
int apdgicp_batch_set_icp(apdgicp_batch* b, const apdgicp_icp_params* p);
int apdgicp_batch_get_icp(const apdgicp_batch* b, apdgicp_icp_params* p, int* enabled);   /* either output may be NULL */
/* The getters below read the last align in this mode; they answer APDGICP_ERR_NO_INPUT once a cloud slot has been set since, or before any.
 * apdgicp_icp_state of every pair of that align; n_pairs = its number of pairs */
int apdgicp_batch_icp_states(apdgicp_batch* b, int32_t* states, int64_t n_pairs);
/* pair `pair` of that align, each as the single handle's call of the same name: the matches of its last iteration in the caller's source
 * order (n = the pair's source size), its W, its trace */
int apdgicp_batch_icp_get_correspondences(apdgicp_batch* b, int64_t pair, int32_t* match, float* sq_dist, int64_t n);
int apdgicp_batch_icp_get_working_cloud(apdgicp_batch* b, int64_t pair, float* xyz, int64_t n);
int apdgicp_batch_icp_get_trace(apdgicp_batch* b, int64_t pair, int64_t capacity, float* T_k16, int64_t* n_corr, double* mse, int32_t* similar, int64_t* n_iterations);
/* Debug: launches, host waits and ticks of the last align in this mode (tests/measure/bench_icp_batch.py); any output may be NULL */
int apdgicp_batch_icp_debug_counts(apdgicp_batch* b, int64_t* launches, int64_t* waits, int64_t* ticks);
/* FAST_VGICP_CUDA as a mode of the batch handle: VC11 .. VC16 above.  p != NULL: the mode on with these parameters (batch voxelized GICP, NDT
 * and ICP off); NULL: mode off.  The parameters are checked before the handle, with the single handle's error codes.  Prepared clouds and maps
 * built so far are kept across off / on. */
int apdgicp_batch_set_vgicp_cuda(apdgicp_batch* b, const apdgicp_vgicp_cuda_params* p);
int apdgicp_batch_get_vgicp_cuda(const apdgicp_batch* b, apdgicp_vgicp_cuda_params* p, int* enabled);   /* either output may be NULL */
/* The four getters below need the mode on and slot `cloud` only; they prepare the slot (and build its map) when it is not current.
 * VC4: the kept list of the slot, as apdgicp_vgicp_cuda_kept */
int apdgicp_batch_vgicp_cuda_kept(apdgicp_batch* b, int32_t cloud, int64_t* n_kept, int32_t* kept_index, int64_t capacity);
/* VC2 / VC3 per kept point of the slot, as apdgicp_vgicp_cuda_get_covariances */
int apdgicp_batch_vgicp_cuda_get_covariances(apdgicp_batch* b, int32_t cloud, double* raw_n6, double* reg_n9, int64_t capacity);
/* the map over the slot's kept points, as apdgicp_vgicp_cuda_voxel_count / _get_voxels */
int apdgicp_batch_vgicp_cuda_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels);
int apdgicp_batch_vgicp_cuda_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9);
/* the frozen indices of pair `pair`'s last linearize in the last align in this mode: n_kept(source) x n_offsets, point-major, -1 = miss.
 * APDGICP_ERR_NO_INPUT before any such align, or once a cloud slot or the mode has been set since.  voxel_index = NULL: nothing is copied and
 * the return value is the pair's n_kept(source). */
int apdgicp_batch_vgicp_cuda_get_correspondences(apdgicp_batch* b, int64_t pair, int32_t* voxel_index, int64_t n_kept_source);
/* Debug: how many clouds this handle has prepared and how many maps it has built in this mode, all slots together; either may be NULL */
int apdgicp_batch_vgicp_cuda_build_count(apdgicp_batch* b, int64_t* n_prepared, int64_t* n_maps);
/* Debug: host waits this handle has spent preparing clouds and building maps since it was created, and the ticks of the last align; any
 * output may be NULL (the tests of VC11 / VC12 and tests/measure/bench_vgicp_cuda_batch.py read them) */
int apdgicp_batch_vgicp_cuda_debug_counts(apdgicp_batch* b, int64_t* prepare_waits, int64_t* map_waits, int64_t* ticks);
/* Measurement: preparation, map builds and ticks of the last align in this mode, in ms by the host clock.  Meaningful with
 * apdgicp_batch_set_profiling on, which puts one more wait in front of the preparation (the cloud sorts end there); the other boundaries are
 * behind waits the align makes anyway. */
int apdgicp_batch_vgicp_cuda_last_phases(apdgicp_batch* b, double ms[3]);
int apdgicp_batch_debug_stats(apdgicp_batch* b, unsigned long long out[16]);
/* APDGICP_STATS=2 and a library built with -DAPD_BLOCK_TIMELINE (a diagnostics variant: tools/build_variant.py) only: {start, end} (100 MHz wall-clock ticks) and the index of every block of the LAST one-pair dense search launch
 * (k_nn_pruned), three words per block, up to 8192 blocks; reading resets.  For tools/c5_blocks.py: where the time of a 100k x 500k
 * iteration goes -- the blocks' own durations or the order they are dealt in. */
int apdgicp_batch_debug_block_timeline(apdgicp_batch* b, unsigned long long* out, int64_t capacity_blocks, int64_t* n_blocks);

/* ------------------------------------------------------------------ scan-to-submap target assembly
 * The step in front of registration_s2m->setInputTarget in scan-to-map mode
 * (scan_matching_odometry_nodelet.cpp:606-618): the clouds of the last <= max_submap_frames keyframes are
 * transformed by their poses relative to the newest keyframe (pcl::transformPointCloud with a Matrix4d),
 * concatenated, and downsampled by downsample() (:412-422) -- pcl::VoxelGrid with the configured leaf
 * (preprocessing_nodelet.cpp:137-144, "VOXELGRID") or, after apdgicp_submap_set_downsample_method, pcl::ApproximateVoxelGrid
 * ("APPROX_VOXELGRID", :145-149; scan_matching_odometry_nodelet.cpp:156-160).  Everything stays on the device; the result can be
 * handed to apdgicp_set_target / apdgicp_batch_set_cloud as a device pointer (16-byte stride).
 *
 * APPROX_VOXELGRID: pcl::ApproximateVoxelGrid<PointXYZI>::applyFilter, PCL 1.10, filters/impl/approximate_voxel_grid.hpp, "as
 * published" like the exact grid.  A table of histsize_ = 512 entries {ix, iy, iz, count, centroid}, all reset at the start of every
 * call; downsample_all_data_ = true (the default, which the reference never changes): the centroid is {x, y, z, intensity}.
 *   AV1. inv[a] = 1.0f / leaf[a] in fp32 (Array3f::Ones() / leaf_size_).
 *   AV2. Voxel index, for point cp in input order: ix = (int)floorf(x * inv[0]), iy, iz likewise; the product is one fp32 multiply
 *        rounded on its own.  A value that an int cannot hold (beyond +-2^31, an infinite product of finite factors, NaN) becomes
 *        INT_MIN, as the reference's x86-64 build converts it -- on the positive side too.
 *   AV3. hash = (ix * 7171 + iy * 3079 + iz * 4231) & 511, in unsigned arithmetic (two's complement: ix = -1, iy = iz = 0 gives 509).
 *   AV4. Eviction.  If entry `hash` has count > 0 and another (ix, iy, iz), it is flushed: centroid / (float)count -- a true fp32
 *        division per component, Eigen >= 3.3 -- becomes the next output point, count and centroid are zeroed.  Then, in every case,
 *        the entry takes (ix, iy, iz), count++ and centroid += {x, y, z, intensity}: fp32 additions in input order.
 *   AV5. Final flush.  After the last point the entries with count > 0 are flushed in ascending entry index.
 *   AV6. Consequences: a voxel can be emitted more than once (evicted, then revisited); the output is not sorted by voxel; n_out lies
 *        between the number of occupied voxels and n; there is no bounding box and no leaf that is "too small".
 *   AV7. Deviations.  A point with a non-finite x, y or z takes no part (PCL's class has undefined behaviour there; in the reference
 *        the range gate has removed such points before the grid, here the gate leaves them as NaN holes: skipping them is the same
 *        thing).  Eigen 3.2's `v /= s`, which multiplies by the reciprocal, is not built.
 * The device does not run the loop: it sorts the points by hash (stable, so input order survives inside an entry), takes every maximal
 * stretch of one voxel inside a hash as one stay in the entry, places the evicted stays by a scan over the points that evicted them
 * and the remaining ones behind them in entry order, and adds every stay's points in input order (apd_approx_voxel.hpp).  The bytes
 * are the loop's (tests/approx_voxel_np.py restates it literally).  At most 2^27 points, like the exact grid.  15 kernel launches and one
 * wait (for n_out) per call, whatever n.  Measured on an MI355X (profiles/approx_voxel.json, tests/measure/bench_approx_voxel.py; device
 * input, leaf 0.1, median ms per assemble; the ranges are those of several sessions, which differ by about 10 %): 0.08 - 0.09 at 512
 * points, 0.09 - 0.10 at 8 192, 0.11 - 0.13 at 100 000, against 0.08 / 0.09 - 0.10 / 0.19 - 0.21 for VOXELGRID on the same clouds in the
 * same process; the whole scan filter at 8 192 points is 0.20 - 0.22 with either.  Both are launch and wait latency up to a scan's size.
 * No bar was set. */
typedef enum { APDGICP_DOWNSAMPLE_VOXELGRID = 0, APDGICP_DOWNSAMPLE_APPROX_VOXELGRID = 1 } apdgicp_downsample_method;
typedef struct apdgicp_submap apdgicp_submap;
int apdgicp_submap_create(int device, void* stream, apdgicp_submap** out);
int apdgicp_submap_destroy(apdgicp_submap* s);
/* Which filter downsample() is (an apdgicp_downsample_method): stays on the object until set again, VOXELGRID after create.  A NULL
 * object or an unknown method: APDGICP_ERR_INVALID_ARG.  A NULL leaf or leaf[0] <= 0 still means NONE, whatever the method. */
int apdgicp_submap_set_downsample_method(apdgicp_submap* s, int method);
/* xyz[c]: first coordinate of cloud c (n_points[c] points, stride_bytes apart, host or device memory as on_device says);
 * intensity_offset_bytes: distance from a point's x to its intensity field (16 for pcl::PointXYZI), < 0: none (0 is kept);
 * rel_poses: n_clouds x 16 doubles, column-major 4x4 (keyframes[i].odom^-1 * keyframes.back().odom, :609), NULL = identity;
 * leaf: voxel size per axis (downsample_resolution), NULL or leaf[0] <= 0: no downsampling (downsample_method NONE);
 * n_out: number of points of the assembled cloud.  Non-finite points are skipped by the voxel filter, as PCL does for
 * non-dense clouds.  A leaf too small for the extent (the voxel index would overflow int32): pcl::VoxelGrid warns ("Leaf size is
 * too small for the input dataset") and returns its input unfiltered -- so does this call: the transformed, concatenated cloud,
 * the warning on stderr and in apdgicp_last_error(), status 0. */
int apdgicp_submap_assemble(apdgicp_submap* s, int n_clouds, const void* const* xyz, const int64_t* n_points, int64_t stride_bytes,
                            int64_t intensity_offset_bytes, int on_device, const double* rel_poses, const float* leaf, int64_t* n_out);
/* device pointer to the last assembled cloud: n points of {x, y, z, intensity} floats, valid until the next assemble */
int apdgicp_submap_points(apdgicp_submap* s, const float** device_xyzi, int64_t* n);
/* copies the last assembled cloud ({x, y, z, intensity} per point) into caller memory */
int apdgicp_submap_copy(apdgicp_submap* s, float* dst_xyzi, int64_t capacity_points, int dst_on_device);

/* ------------------------------------------------------------------ scan preprocessing
 * What PreprocessingNodelet::cloud_callback does to every scan before it is published and becomes a registration source
 * (radar_graph_slam/apps/preprocessing_nodelet.cpp:812-815), in the reference's order, on the device:
 *   1. distance_filter (:881-889), when use_distance_filter: a point stays iff  d > near && d < far && z < z_high && z > z_low  with
 *      d = the fp32 norm sqrtf((x*x + y*y) + z*z) and z, both widened to double; a non-finite point fails; input order is kept.
 *      (Eigen's own summation order for a 3-vector norm is not pinned here; it can matter only within 1 ulp of a threshold.)
 *   2. downsample (:850-866): leaf[0] > 0: pcl::VoxelGrid ("VOXELGRID", :137-144) through the kernels of apdgicp_submap_assemble --
 *      one point per occupied voxel in ascending voxel index, a leaf too small for the extent returns the cloud unfiltered with the
 *      same warning (non-finite points are dropped from it here, in input order); leaf[0] <= 0: pcl::removeNaNFromPointCloud (:852-857),
 *      order kept.  downsample_method APPROX_VOXELGRID (:145-149) with leaf[0] > 0: pcl::ApproximateVoxelGrid instead, AV1 .. AV7 above
 *      (one point per stay of a voxel in its table entry, in eviction order and then entry order; never "too small").
 *   3. outlier_removal (:868-879) on the cloud of step 2, whose order the output keeps.  d2 = the fp32 squared distance in FLANN
 *      L2_Simple order, neighbours in rank order, the first one the point itself (or a duplicate) at 0:
 *        STATISTICAL (:167-175, pcl::StatisticalOutlierRemoval): k = mean_k + 1; score = (float)(sum_{r=1..mean_k} (double)sqrtf(d2[r]) / mean_k)
 *          added in rank order; sum = sum of the scores, sq = sum of (double)(score * score) (fp32 product); mean = sum / n,
 *          var = (sq - sum * sum / n) / (n - 1), thr = mean + stddev_mul * sqrt(var); a point stays iff (double)score <= thr.  The device
 *          adds sum / sq in a fixed tree (PCL: point after point): the same bits on every run, mean / thr may differ from PCL's in the last bits.
 *        RADIUS (:176-184, pcl::RadiusOutlierRemoval, dense branch): k = min_neighbors + 1; a point stays iff (double)d2[k - 1] <= radius * radius.
 *        NONE: the cloud of step 2.
 *      mean_k / min_neighbors up to 31 (the exact pruned k-NN of the covariances serves them; APDGICP_KNN_MODE=brute: the brute-force one);
 *      above: APDGICP_ERR_UNSUPPORTED.  A step-2 cloud with fewer than k points: APDGICP_ERR_TOO_FEW_POINTS; an empty one: n_out = 0, status 0.
 * PCL is not part of the reference tree: "as published" (PCL 1.10), like the voxel grid.  The power filter, the ego-velocity RANSAC,
 * underfloor_filter, tf and ROS are not part of this object. */
typedef enum { APDGICP_OUTLIER_NONE = 0, APDGICP_OUTLIER_STATISTICAL = 1, APDGICP_OUTLIER_RADIUS = 2 } apdgicp_outlier_method;
typedef struct {
  int32_t use_distance_filter;   /* "use_distance_filter", :201 ; default 1 */
  int32_t outlier_method;        /* apdgicp_outlier_method, "outlier_removal_method", :166 ; default STATISTICAL */
  int32_t mean_k;                /* "statistical_mean_k", :168 ; default 20 */
  int32_t min_neighbors;         /* "radius_min_neighbors", :178 ; default 2 */
  double near;                   /* "distance_near_thresh", :202 ; default 1.0 */
  double far;                    /* "distance_far_thresh", :203 ; default 100.0 */
  double z_low;                  /* "z_low_thresh", :204 ; default -5.0 */
  double z_high;                 /* "z_high_thresh", :205 ; default 20.0 */
  double stddev_mul;             /* "statistical_stddev", :169 ; default 1.0 */
  double radius;                 /* "radius_radius", :177 ; default 0.8 */
  float leaf[3];                 /* "downsample_resolution", :138 ; default 0.1 each; leaf[0] <= 0: "downsample_method" NONE */
  int32_t downsample_method;     /* apdgicp_downsample_method, "downsample_method", :137-156 ; default VOXELGRID (0); anything else: INVALID_ARG */
} apdgicp_scan_filter_params;
typedef struct apdgicp_scan_filter apdgicp_scan_filter;
void apdgicp_scan_filter_default_params(apdgicp_scan_filter_params* p);                       /* the nodelet's defaults, :137-205 */
/* PreprocessingNodelet::initialize_params (:136-206).  `stream` may be NULL (the object creates its own) or a hipStream_t of the caller */
int apdgicp_scan_filter_create(const apdgicp_scan_filter_params* p, int device, void* stream, apdgicp_scan_filter** out);
int apdgicp_scan_filter_destroy(apdgicp_scan_filter* f);
int apdgicp_scan_filter_set_params(apdgicp_scan_filter* f, const apdgicp_scan_filter_params* p);
/* distance_filter -> downsample -> outlier_removal (:812-815) of one scan: xyz / n / stride_bytes / intensity_offset_bytes / on_device as in
 * apdgicp_submap_assemble (intensity is carried through: the centroid's in a voxel, the point's own otherwise).  The call waits for
 * the size of the cloud of step 2 (the launches of step 3 are sized by it) and for n_out. */
int apdgicp_scan_filter_run(apdgicp_scan_filter* f, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device,
                            int64_t* n_out);
/* device pointer to the filtered scan: n points of {x, y, z, intensity} floats (16-byte stride), valid until the next run; what
 * apdgicp_set_source(..., on_device = 1) and apdgicp_batch_set_cloud accept -- the cloud points_pub publishes (:826) never leaves the device */
int apdgicp_scan_filter_points(apdgicp_scan_filter* f, const float** device_xyzi, int64_t* n);
/* copies the filtered scan ({x, y, z, intensity} per point) into caller memory */
int apdgicp_scan_filter_copy(apdgicp_scan_filter* f, float* dst_xyzi, int64_t capacity_points, int dst_on_device);
/* sizes of the last run: counts[0] the input, [1] behind distance_filter, [2] behind downsample, [3] the output */
int apdgicp_scan_filter_stage_counts(apdgicp_scan_filter* f, int64_t counts[4]);
/* What step 3 of the last run decided on, in the order of the cloud of step 2 (counts[2] entries; 0 entries for NONE): stat = the score
 * (STATISTICAL) or d2[k - 1] (RADIUS), kept = 1 / 0; mean / stddev / thr: STATISTICAL's, RADIUS: 0, 0, radius * radius.  Any pointer may
 * be NULL; host memory.  For tests and for tuning the two thresholds. */
int apdgicp_scan_filter_scores(apdgicp_scan_filter* f, float* stat, uint8_t* kept, int64_t capacity, double* mean, double* stddev, double* thr);

/* ------------------------------------------------------------------ Doppler ego velocity and moving-point removal
 * rio::RadarEgoVelocityEstimator::estimate ("E:" = radar_graph_slam/src/radar_ego_velocity_estimator.cpp, "EH:" =
 * radar_graph_slam/include/radar_ego_velocity_estimator.h), the step PreprocessingNodelet::cloud_callback runs on the raw
 * {x, y, z, intensity, doppler} scan right before the filters above (preprocessing_nodelet.cpp:708-741); its inlier cloud replaces the
 * raw scan as src_cloud when enable_dynamic_object_removal is set (:775-786).  On the device, in the reference's order:
 *   1. E:75-91, per point (input order kept):  xd, yd, zd = the coordinates widened to double;  r = sqrt((xd*xd + yd*yd) + zd*zd)
 *      (Eigen's own order for Vector3d::norm() is not pinned here; it can matter only within 1 ulp of min_dist / max_dist);
 *      az = (double)atan2f(y, x),  el = (double)atan2f(sqrtf(x*x + y*y), z) - M_PI_2  (fp32 products and sum each rounded on their own;
 *      atan2f is glibc's, apd_atan2f.h);  valid = r > min_dist && r < max_dist && intensity > min_db (fp32) && fabs(az) < az_thr &&
 *      fabs(el) < el_thr, *_thr = (double)deg * M_PI / 180.0 (angles::from_degrees), a NaN fails;  v = (-doppler) * factor in fp32;
 *      row = {xd/r, yd/r, zd/r, (double)v}.  m = the number of valid rows; m <= 2: no estimate (success = 0).
 *   2. E:99-118, zero velocity:  n0 = (size_t)((double)m * (1.0 - (double)allowed_outlier_percentage)), clamped to m - 1 (the reference
 *      reads one past the end at 0 %);  the n0-th smallest |v| (exact: a radix selection on the fp32 bits) < thresh_zero_velocity:
 *      v = 0, sigma = sigma_zero_velocity_*, the inliers are the rows with |v| < thresh in order, no outliers.
 *   3. E:190-199, K hypotheses of S = N_ransac_points rows each.  The reference draws from std::random_device (E:187-194), which nobody
 *      can reproduce; the CALLER supplies K * S uint32 words, and sample i of hypothesis k is  c = words[k * S + i] % (m - i)  among the
 *      rows this hypothesis has not picked yet (for every earlier pick t in ascending order: t <= c moves c up by one): the stand-in for
 *      std::shuffle, S distinct rows.  m < S: no hypotheses, success = 0.  The solve (E:257-273): H^T H (6 sums) and H^T y (3 sums)
 *      added row after row in sample order, then an UNPIVOTED 3x3 LDL^T:  d0 = a00, l10 = a01/d0, l20 = a02/d0, d1 = a11 - l10*a01,
 *      t = a12 - l20*a01, l21 = t/d1, d2 = (a22 - l20*a02) - l21*t;  z0 = b0, z1 = b1 - l10*z0, z2 = (b2 - l20*z0) - l21*z1;
 *      w = z / d;  v2 = w2, v1 = w1 - l21*v2, v0 = (w0 - l10*v1) - l20*v2.  (Eigen's ldlt() pivots: a deviation, like the 6x6 solve of
 *      the registration.)  use_cholesky_instead_of_bdcsvd = 0 (bdcSvd): APDGICP_ERR_UNSUPPORTED.
 *   4. E:203-214, every hypothesis against every row in one pass:  inlier = fabs(y - ((h0*v0 + h1*v1) + h2*v2)) < (double)inlier_thresh.
 *   5. E:215-233, the reference's bookkeeping, quirks included:  n_out = m - n_in;  (double)((float)n_out / (float)m) > 0.05: the
 *      hypothesis's outliers are appended behind its inliers and it counts as n_in = m, n_out = 0;  best_in = the lowest k with the
 *      largest such n_in, best_out = the lowest k with the largest such n_out if any is above 0 (it may be ANOTHER hypothesis).
 *   6. E:239-247, 257-293, the fit on best_in's list in list order:  H^T H, H^T y, then e^T e (e = H v - y) as fixed-tree fp64 sums
 *      (Eigen: its own order; the same bits on every run, the last bits may differ from Eigen's), the LDL^T of 3,
 *      C = e^T e * inv(H^T H) / (rows - 3) with the inverse by cofactors, sigma = sqrt(diag C) + sigma_offset_radar_*.  The reference
 *      returns true on every path (E:302): success = 1 whenever the inlier list is not empty; sigma_in_bounds says whether
 *      diag C >= 0 and sigma < max_sigma_* held (if diag C < 0, sigma holds diag C as in the reference).
 *   use_ransac = 0 (E:138-142): every valid row is an inlier, step 6 alone.
 * Not part of this object: bdcSvd; deskewing (:792) is apdgicp_scan_ingest_deskew below, which takes _inliers' device pointer.  The radius filter on the outlier cloud (:766-774) is the scan filter with
 * APDGICP_OUTLIER_RADIUS, its clustering into moving objects apdgicp_dbscan_* below; both take the device pointers of _outliers. */
typedef struct {
  float min_dist;                             /* EH:32 ; default 0.1 */
  float max_dist;                             /* EH:33 ; default 400 */
  float min_db;                               /* EH:34 ; default 5 */
  float elevation_thresh_deg;                 /* EH:35 ; default 60 */
  float azimuth_thresh_deg;                   /* EH:36 ; default 120 */
  float doppler_velocity_correction_factor;   /* EH:37 ; default 1 */
  float thresh_zero_velocity;                 /* EH:39 ; default 0.05 */
  float allowed_outlier_percentage;           /* EH:40 ; default 0.30 */
  float sigma_zero_velocity_x;                /* EH:41 ; default 1.0e-3 */
  float sigma_zero_velocity_y;                /* EH:42 ; default 3.2e-3 */
  float sigma_zero_velocity_z;                /* EH:43 ; default 1.0e-2 */
  float sigma_offset_radar_x;                 /* EH:45 ; default 0 */
  float sigma_offset_radar_y;                 /* EH:46 ; default 0 */
  float sigma_offset_radar_z;                 /* EH:47 ; default 0 */
  float max_sigma_x;                          /* EH:49 ; default 0.2 */
  float max_sigma_y;                          /* EH:50 ; default 0.2 */
  float max_sigma_z;                          /* EH:51 ; default 0.2 */
  float max_r_cond;                           /* EH:52 ; never read by the reference (E:269) nor here; default 1000 */
  float outlier_prob;                         /* EH:56 ; default 0.05 */
  float success_prob;                         /* EH:57 ; default 0.995 */
  float inlier_thresh;                        /* EH:59 ; default 0.5 */
  int32_t use_cholesky_instead_of_bdcsvd;     /* EH:53 ; default 1 ; 0: APDGICP_ERR_UNSUPPORTED */
  int32_t use_ransac;                         /* EH:55 ; default 1 */
  int32_t N_ransac_points;                    /* EH:58 (a float there) ; default 5 ; 3 .. 8 */
  int32_t n_hypotheses;                       /* 0 (default): setRansacIter's formula, EH:138-143 (3 at the defaults); else 1 .. 1024 */
  int32_t reserved;                           /* 0 */
} apdgicp_ego_velocity_params;
/* What estimate() reports (E:52-170) and how it got there.  best_in / best_out: -1 when there is none. */
typedef struct {
  double v[3];                /* v_r */
  double sigma[3];            /* sigma_v_r */
  int32_t success;            /* estimate()'s return value */
  int32_t zero_velocity;      /* the branch of E:108 was taken */
  int32_t sigma_in_bounds;    /* E:284-292 */
  int32_t m;                  /* valid rows (E:74-91) */
  int32_t n_inlier;           /* points of the inlier cloud */
  int32_t n_outlier;          /* points of the outlier cloud */
  int32_t best_in;
  int32_t best_out;
  int32_t K;                  /* hypotheses of this run (ransac_iter_) */
  int32_t reserved;
} apdgicp_ego_velocity_result;
typedef struct apdgicp_ego_velocity apdgicp_ego_velocity;
void apdgicp_ego_velocity_default_params(apdgicp_ego_velocity_params* p);                     /* RadarEgoVelocityEstimatorConfig's defaults, EH:30-60 */
/* RadarEgoVelocityEstimator() + configure() (EH:86-88, 152-188).  `stream` may be NULL (the object creates its own) or a hipStream_t of the caller */
int apdgicp_ego_velocity_create(const apdgicp_ego_velocity_params* p, int device, void* stream, apdgicp_ego_velocity** out);
int apdgicp_ego_velocity_destroy(apdgicp_ego_velocity* e);
int apdgicp_ego_velocity_set_params(apdgicp_ego_velocity* e, const apdgicp_ego_velocity_params* p);   /* configure(), EH:152-188 */
/* the number of hypotheses a run with these parameters scores: n_hypotheses, or setRansacIter's (EH:138-143)
 * uint(log(1.0 - success_prob) / log(1.0 - pow(1.0 - outlier_prob, N_ransac_points))) ; needs no device */
int apdgicp_ego_velocity_hypothesis_count(const apdgicp_ego_velocity_params* p, int32_t* K);
/* estimate() (E:60-170) of one scan: `pts` is the address of the first x, points `stride_bytes` apart, intensity (snr_db) and doppler
 * floats at the given byte offsets inside a point; on_device as everywhere.  `words`: HOST memory, n_words >= K * N_ransac_points
 * uint32 (fewer: APDGICP_ERR_INVALID_ARG; unused without RANSAC, may be NULL then).  n = 0: status 0, success = 0.  The call waits once,
 * for the result record (a host scan is staged by a copy on the object's stream, without a wait); the clouds stay on the device. */
int apdgicp_ego_velocity_run(apdgicp_ego_velocity* e, const float* pts, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes,
                             int64_t doppler_offset_bytes, int on_device, const uint32_t* words, int64_t n_words, apdgicp_ego_velocity_result* result);
/* The inlier (static) / outlier (moving) cloud of the last run in device memory, valid until the next run: n points of {x, y, z, intensity}
 * floats, 16 bytes apart -- what apdgicp_scan_filter_run(..., on_device = 1) and apdgicp_set_source accept --, beside it one float doppler
 * per point (toRadarPointCloudType, E:41-50: -v) and the point's index in the input scan.  Any pointer but e may be NULL. */
int apdgicp_ego_velocity_inliers(apdgicp_ego_velocity* e, const float** device_xyzi, const float** device_doppler, const int32_t** device_index, int64_t* n);
int apdgicp_ego_velocity_outliers(apdgicp_ego_velocity* e, const float** device_xyzi, const float** device_doppler, const int32_t** device_index, int64_t* n);
/* copies one of the two clouds to HOST memory: which = 0 inliers, 1 outliers; xyzi [4 * capacity], doppler / index / row [capacity]
 * (row: the point's index among the valid rows, i.e. the reference's inlier_idx_best / outlier_idx_best); any destination may be NULL */
int apdgicp_ego_velocity_copy(apdgicp_ego_velocity* e, int which, float* xyzi, float* doppler, int32_t* index, int32_t* row, int64_t capacity);
/* every hypothesis of the last run: v_k [3 * capacity] doubles and n_in [capacity] (before the 5 % rule); host memory; for tests and tuning */
int apdgicp_ego_velocity_hypotheses(apdgicp_ego_velocity* e, double* v_k, int32_t* n_in, int64_t capacity);
/* The intermediate results of the last run, host memory, any pointer may be NULL (for tests): valid [n] 0 / 1 per input point
 * (valid_capacity >= n entries); rows [4 * m] doubles (rows_capacity >= m rows); samples [K * N_ransac_points] row indices
 * (samples_capacity >= that many entries; RANSAC runs only, else untouched); selected_abs_v: the n0-th smallest |v|.  A destination that
 * is too small: APDGICP_ERR_INVALID_ARG, nothing is written. */
int apdgicp_ego_velocity_debug(apdgicp_ego_velocity* e, uint8_t* valid, int64_t valid_capacity, double* rows, int64_t rows_capacity, int32_t* samples,
                               int64_t samples_capacity, float* selected_abs_v);

/* ------------------------------------------------------------------ floor plane detection and under-floor removal
 * radar_graph_slam::FloorDetectionNodelet ("F:" = radar_graph_slam/apps/floor_detection_nodelet.cpp), which runs on every raw scan
 * (radar_graph_slam.launch:13-14): its coefficients become the ground-plane factor of every keyframe, its under-floor-clipped cloud is
 * published for the rest of the chain.  PCL is not part of the reference tree: the steps below follow its published algorithm, and every
 * operation order that is PCL's or Eigen's (not pinned by the reference, like T*p above) is the one written here.  On the device:
 *   1. F:156-163, per point (input order kept):  t = R p with R = R_y(tilt_deg) in fp32 -- angle = (float)(tilt_deg * M_PI / 180.0),
 *      c / s = its cosine / sine evaluated in double and rounded to fp32, R = {c, 0, s; 0, (1 - c) + c, 0; -s, 0, c}, a coordinate is
 *      (r0 x + r1 y) + r2 z (every fp32 operation rounded on its own; the zero translation is not added).  A plane distance is
 *      ((a x + b y) + c z) + d everywhere (PlaneClipper3D::getDistance).  The point stays iff the distance to (0, 0, 1,
 *      (float)(sensor_height + height_clip_range)) is >= 0 and the distance to (0, 0, 1, (float)(sensor_height - height_clip_range)) is
 *      not.  n_clipped points.
 *   2. F:280-307 (use_normal_filtering): per clipped point the normal_k nearest clipped points, itself included (the exact k-NN of the
 *      registration, keys = fp32 squared distance, then index); their population covariance in fp64 (the sums of
 *      apdgicp_compute_covariances, no regularisation), its eigenvectors by the Jacobi sweeps of the registration; u = the eigenvector of
 *      the smallest eigenvalue; stat = (float)(|u_z| / |u|); the point stays iff (double)stat > cos(normal_filter_thresh * M_PI / 180.0).
 *      Deviations: PCL forms the covariance in fp32 and uses eigen33; the viewpoint flip (F:289) cannot change an absolute value and is
 *      not evaluated.  n_clipped < normal_k: PCL's normals are NaN, nothing stays (no search is launched).
 *      Then the inverse tilt (F:169): the fp32 TRANSPOSE of R (Eigen's 4x4 inverse divides by c c + s s, 1 within an ulp).  n_filtered points.
 *   3. F:177: n_filtered < floor_pts_thresh: no floor.  Else K = n_hypotheses three-point hypotheses.  PCL's sampler cannot be
 *      reproduced: the CALLER supplies K * 3 uint32 words and row i of hypothesis k is drawn as in apdgicp_ego_velocity_run (step 3 there).
 *      SampleConsensusModelPlane::computeModelCoefficients:  a = p1 - p0, b = p2 - p0;  the sample is BAD (collinear) iff
 *      ax/bx == ay/by && az/bz == ay/by;  n = a x b = {ay bz - az by, az bx - ax bz, ax by - ay bx};  n /= sqrtf((nx nx + ny ny) + nz nz);
 *      d = -((nx x0 + ny y0) + nz z0).
 *   4. countWithinDistance, every hypothesis against every filtered point in one pass:
 *      inlier = (double)fabsf(((a x + b y) + c z) + d) < distance_threshold.
 *   5. RandomSampleConsensus::computeModel replayed over hypotheses 0, 1, ...:  while (iterations < k && skipped < 10 * max_iterations):
 *      a bad sample: ++skipped; else: strictly more inliers than the best so far replaces it and k = log(1 - probability) /
 *      log(p), p = 1 - (w w) w clamped to [eps, 1 - eps], w = n_best * (1.0 / n_filtered); ++iterations; stop when iterations >
 *      max_iterations.  table_exhausted = 1 when the K hypotheses ran out before that loop stopped (supply more words).
 *   6. F:192-213: no model or n_inliers < floor_pts_thresh: no floor;  |(a r0 + b r1) + c r2| < cos(floor_normal_thresh * M_PI / 180.0)
 *      with r = tilt^-1 e_z = (-s, 0, c): no floor;  c < 0: the four coefficients times -1.
 *   7. F:100-134, the callback's memory, kept on the device: a detected floor becomes prev_coeffs and is published; without one the
 *      published coefficients are prev_coeffs after a first detection, (0, 0, 1, 0) before.  Under-floor removal keeps an input point iff
 *      ((a x + b y) + c z) + (float)((double)d + floor_tolerance) >= 0 with prev_coeffs, initially (0, 0, 0, (float)(sensor_height -
 *      height_clip_range)).
 * The call waits once for the result record; with use_normal_filtering it waits once more before that, for n_clipped (the search is
 * sized on the host, like apdgicp_scan_filter_run's).  Not part of this object: the ROS plumbing, the marker, optimizeModelCoefficients
 * (the nodelet never calls it). */
typedef struct {
  double tilt_deg;              /* F:63 ; default 0 */
  double sensor_height;         /* F:64 ; default 2 */
  double height_clip_range;     /* F:65 ; default 1 ; > 0 */
  double floor_normal_thresh;   /* F:67 ; default 10 [deg] ; > 0 */
  double normal_filter_thresh;  /* F:69 ; default 20 [deg] ; > 0 */
  double floor_tolerance;       /* F:70 ; default 0.1 */
  double distance_threshold;    /* F:185 ; default 0.06 ; > 0 */
  double probability;           /* pcl::SampleConsensus::probability_ ; default 0.99 ; inside (0, 1) */
  int32_t floor_pts_thresh;     /* F:66 ; default 50 ; >= 0 */
  int32_t use_normal_filtering; /* F:68 ; default 1 */
  int32_t max_iterations;       /* pcl::SampleConsensus::max_iterations_ ; default 1000 ; >= 1 */
  int32_t normal_k;             /* F:288 ; default 10 ; 3 .. 64, above 32: APDGICP_ERR_UNSUPPORTED */
  int32_t n_hypotheses;         /* K ; default 64 ; 1 .. 1024 */
  int32_t reserved[3];          /* 0 */
} apdgicp_floor_params;
typedef enum { APDGICP_FLOOR_OK = 0, APDGICP_FLOOR_FEW_POINTS = 1, APDGICP_FLOOR_NO_MODEL = 2, APDGICP_FLOOR_FEW_INLIERS = 3, APDGICP_FLOOR_NOT_HORIZONTAL = 4 } apdgicp_floor_reject;
typedef struct {
  float coeffs[4];              /* what floor_pub publishes (F:100-130) */
  float raw_coeffs[4];          /* the winning model as RANSAC left it, before the upward flip; zeros without a model */
  int32_t detected;             /* detect() returned coefficients */
  int32_t ground_initialized;   /* F:110, after this scan */
  int32_t reject_reason;        /* apdgicp_floor_reject */
  int32_t n_input;
  int32_t n_clipped;            /* behind the height clip (F:162-163) */
  int32_t n_filtered;           /* behind normal_filtering (F:165-169): RANSAC's cloud */
  int32_t n_inliers;            /* inliers of the winning model (0 without one); the inlier LIST exists for a detected floor only */
  int32_t n_under_floor;        /* points of the under-floor-filtered cloud (F:132-134) */
  int32_t iterations;           /* iterations_ of computeModel */
  int32_t skipped;              /* skipped_count of computeModel */
  int32_t winner;               /* index of the winning hypothesis, -1: none */
  int32_t table_exhausted;      /* the hypotheses ran out before computeModel's loop would have stopped */
  int32_t K;                    /* hypotheses of this run */
  int32_t reserved[3];
} apdgicp_floor_result;
typedef struct apdgicp_floor apdgicp_floor;
void apdgicp_floor_default_params(apdgicp_floor_params* p);   /* initialize_params (F:62-70), F:185, pcl::SampleConsensus's defaults */
/* FloorDetectionNodelet::onInit (F:36-56).  `stream` may be NULL (the object creates its own).  Parameter errors need no device; without a
 * device: APDGICP_ERR_UNSUPPORTED */
int apdgicp_floor_create(const apdgicp_floor_params* p, int device, void* stream, apdgicp_floor** out);
int apdgicp_floor_destroy(apdgicp_floor* f);
/* initialize_params (F:62-70) again; the callback's memory (prev_coeffs, ground_intialized) is kept: apdgicp_floor_reset restores it */
int apdgicp_floor_set_params(apdgicp_floor* f, const apdgicp_floor_params* p);
int apdgicp_floor_reset(apdgicp_floor* f);                    /* F:75-80 */
/* cloud_callback (F:88-137) of one scan: `xyz` is the address of the first x, points `stride_bytes` apart, the intensity float at
 * `intensity_offset_bytes` inside a point (< 0: none, 0 is carried), on_device as everywhere.  `words`: HOST memory, n_words >= 3 * K
 * uint32 (fewer: APDGICP_ERR_INVALID_ARG).  n = 0: the callback returns before anything (F:92-94): status 0, a zero record, no change. */
int apdgicp_floor_run(apdgicp_floor* f, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device,
                      const uint32_t* words, int64_t n_words, apdgicp_floor_result* result);
/* floor_points (F:215-222) of the last run in device memory, valid until the next run: n points of {x, y, z, intensity}, 16 bytes apart,
 * in input order, beside them each point's index in the input scan; n = 0 unless a floor was detected.  Any pointer but f may be NULL. */
int apdgicp_floor_inliers(apdgicp_floor* f, const float** device_xyzi, const int32_t** device_index, int64_t* n);
/* /underfloor_filtered_points (F:132-137) of the last run in device memory, like apdgicp_floor_inliers: what
 * apdgicp_scan_filter_run(..., on_device = 1) and apdgicp_set_source accept, without a host round trip */
int apdgicp_floor_under_floor_filtered(apdgicp_floor* f, const float** device_xyzi, const int32_t** device_index, int64_t* n);
/* copies one cloud of the last run to HOST memory: which = 0 the height-clipped cloud (tilted frame, F:162-163), 1 the filtered cloud
 * RANSAC ran on (F:169, floor_filtered_points), 2 the inliers, 3 the under-floor-filtered cloud; xyzi [4 * capacity], index [capacity]
 * (into the input scan); any destination may be NULL; a capacity below the cloud's size: APDGICP_ERR_INVALID_ARG */
int apdgicp_floor_copy(apdgicp_floor* f, int which, float* xyzi, int32_t* index, int64_t capacity);
/* every hypothesis of the last run (computeModelCoefficients / countWithinDistance): coeffs [4 * capacity] floats, bad [capacity] 0 / 1,
 * n_in [capacity]; host memory, any may be NULL; all zero when RANSAC did not run (F:177) */
int apdgicp_floor_hypotheses(apdgicp_floor* f, float* coeffs, uint8_t* bad, int32_t* n_in, int64_t capacity);
/* intermediate results of the last run, host memory, any pointer may be NULL (for tests): clip_mask [n] 0 / 1 per input point (F:162-163),
 * normal_stat [n_clipped] floats (step 2; untouched unless the search ran), samples [3 * K] row indices of the filtered cloud (untouched
 * when RANSAC did not run).  A destination that is too small: APDGICP_ERR_INVALID_ARG, nothing is written. */
int apdgicp_floor_debug(apdgicp_floor* f, uint8_t* clip_mask, int64_t mask_capacity, float* normal_stat, int64_t stat_capacity, int32_t* samples, int64_t samples_capacity);

/* ------------------------------------------------------------------ map cloud generation
 * radar_graph_slam::MapCloudGenerator::generate (radar_graph_slam/src/radar_graph_slam/map_cloud_generator.cpp:13-53, "M:"), which the
 * back end calls after every graph optimisation (radar_graph_slam_nodelet.cpp:793) and for the save-map service (:1246) with all
 * keyframes and map_cloud_resolution.  The keyframe clouds do not change between two calls, only their poses do: a cloud is uploaded
 * once (add_keyframe) and stays in device memory the object owns; generate uploads poses only.  PCL is not part of the reference tree;
 * the octree follows PCL 1.10 as published (octree/impl/octree_pointcloud.hpp: addPointsFromInputCloud, adoptBoundingBoxToPoint,
 * getKeyBitSize, genOctreeKeyforPoint, genLeafNodeCenterFromOctreeKey; octree_base.hpp / octree_key.h:
 * getOccupiedVoxelCentersRecursive, pushBranch).  eps = FLT_EPSILON widened to double, res = the resolution.
 *   M1 (M:22-31): keyframes in the order given, points in cloud order.  d = (double)sqrtf((x*x + y*y) + z*z), every fp32 operation
 *      rounded on its own; a point is skipped iff d > 50 (a NaN point is kept).  P = the 16 doubles of the pose rounded to fp32;
 *      dst = P * (x, y, z, 1) in fp32, per row (r0*x + r1*y) + (r2*z + t), with APDGICP_FLAG_XF_LINEAR_CHAIN in `flags`
 *      ((r0*x + r1*y) + r2*z) + t -- the two orders of apdgicp_params.flags; the intensity is copied.  The "pushed" cloud, in order.
 *   M2 (M:38-39): res <= 0: the output is the pushed cloud itself, intensities and non-finite points included.
 *   M3: the bounding box, replayed over the finite pushed points in order; comparisons on the fp32 coordinate widened to double.
 *      First point p: min = p - res/2, max = p + res/2; mk = ceil((max - min - eps) / res) per axis; depth = ceil(log2(max(mk, 2)) - eps);
 *      side = 2^depth * res; per axis o = (side - (max - min)) / 2, and if o > eps: min -= o, max += o.  Every later point: while
 *      p[a] < min[a] or p[a] >= max[a] on any axis: side = (double)(1 << depth) * res; min[a] -= side on every axis with !(p[a] >= max[a]);
 *      depth += 1; max[a] = min[a] + ((double)(1 << depth) * res - eps) on all axes.  A depth above 21: APDGICP_ERR_UNSUPPORTED (PCL shifts
 *      an int by the depth; 21 keeps the interleaved key within 63 bits; at 0.05 m depth 21 is 104 km).
 *   M4: key[a] = (unsigned)(((double)p[a] - min[a]) / res) with the final min, an IEEE fp64 division, truncated.
 *   M5: one output point per distinct (kx, ky, kz), ascending in the interleaved key whose bit triple at level L, from the most
 *      significant, is (kx_L << 2) | (ky_L << 1) | kz_L -- the depth-first walk; coordinates (float)(((double)key[a] + 0.5) * res + min[a]);
 *      intensity 0 (the reference pushes a default-constructed point).
 *   M6: no keyframes: APDGICP_ERR_INVALID_ARG (the reference returns nullptr); no finite pushed point: n_out = 0, status 0; more than
 *      2^31 - 1 input points: APDGICP_ERR_UNSUPPORTED; a resolution that is NaN or infinite: APDGICP_ERR_INVALID_ARG.
 * Nothing per point goes to the host.  The distinct keys come from a stable radix sort of the interleaved keys.  The calls wait for
 * their own work. */
typedef struct {
  int64_t n_input, n_pushed, n_finite, n_out;   /* points of the keyframes given, M1's cloud, its finite points, the output */
  double min[3], max[3];                        /* M3's final box (zeros without an octree) */
  int32_t depth, rounds;                        /* octree depth; points after the first that made the box grow */
  int32_t sort_passes, sort_kind;               /* radix passes (8-bit digits over 3 * depth bits); always 0 (the radix sort) */
  float stage_ms[4];                            /* device time of the last generate: M1, M3, keys + sort, heads + centres */
} apdgicp_map_cloud_stats;
typedef struct apdgicp_map_cloud apdgicp_map_cloud;
int apdgicp_map_cloud_create(int device, void* stream, apdgicp_map_cloud** out);
int apdgicp_map_cloud_destroy(apdgicp_map_cloud* m);
/* copies a keyframe's cloud (n >= 0 points, stride_bytes apart, host or device memory; intensity_offset_bytes < 0: intensity 0) into
 * device memory the object owns; *id = 0, 1, 2 ... in the order of the calls */
int apdgicp_map_cloud_add_keyframe(apdgicp_map_cloud* m, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device, int32_t* id);
int apdgicp_map_cloud_clear(apdgicp_map_cloud* m);   /* forgets every keyframe and the last result; ids start at 0 again */
/* ids: n_keyframes ids in visiting order (any subset, repeats allowed; NULL: 0 .. n_keyframes - 1), an unknown id: APDGICP_ERR_INVALID_ARG;
 * poses: n_keyframes x 16 doubles, column-major 4x4; flags: 0 or APDGICP_FLAG_XF_LINEAR_CHAIN */
int apdgicp_map_cloud_generate(apdgicp_map_cloud* m, int32_t n_keyframes, const int32_t* ids, const double* poses, double resolution, int32_t flags, int64_t* n_out);
/* device pointer to the last generated cloud: n points of {x, y, z, intensity} floats, valid until the next generate / clear; what
 * apdgicp_set_target accepts (16-byte stride) */
int apdgicp_map_cloud_points(apdgicp_map_cloud* m, const float** device_xyzi, int64_t* n);
int apdgicp_map_cloud_copy(apdgicp_map_cloud* m, float* dst_xyzi, int64_t capacity_points, int dst_on_device);
int apdgicp_map_cloud_info(apdgicp_map_cloud* m, apdgicp_map_cloud_stats* info);

/* ------------------------------------------------------------------ Scan Context place recognition
 * radar_graph_slam::SCManager (radar_graph_slam/src/radar_graph_slam/Scancontext.cpp, "SC:"), called from
 * LoopDetector::performScanContextLoopClosure (loop_detector.cpp:208) with sc_dist_thresh 0.5 and sc_azimuth_range 56.5.  The database of
 * descriptors lives in device memory.  Two knobs generalise the reference's cost limits: num_candidates (the reference scores the 3 nearest
 * ring keys; 0 or >= n: every candidate) and search_ratio (the reference tries the shifts within 0.1 * S / 2 of the sector-key alignment; 1.0:
 * all).  R = num_ring, S = num_sector, each 1 .. 64.
 *   S1 (SC:162-214) descriptor.  Per point (x, y, intensity), z unused: range = sqrtf(x*x + y*y), fp32, every operation rounded on its own;
 *      angle = (float)(((double)atan2f(x, y) - M_PI_2) * 180.0 / M_PI) with apd_atan2f (note the argument order); the point is skipped if
 *      fabsf(angle) > azimuth_max or (double)range > max_radius; ring = clamp((int)ceil(((double)range / max_radius) * R), 1, R);
 *      sector = clamp((int)ceil((((double)angle - azimuth_min) / (azimuth_max - azimuth_min)) * S), 1, S); bin[ring-1][sector-1] = the maximum
 *      intensity among its points with intensity > -1000, 0 for a bin nobody wrote.  Stored as R x S fp32, ring-major (exact: every entry is
 *      an intensity or 0); every later operation is fp64 on the widened values.
 *   S2 (SC:217-246) ring_key[r] = (float)(sum_c d[r][c] / S); sector_key[c] = sum_r d[r][c] / R; col_norm[c] = sqrt(sum_r d[r][c]^2): fp64,
 *      ascending index, one accumulator, unfused; computed once, when the descriptor is added.
 *   S3 (SC:284-305) query_id < num_exclude_recent: no loop, zero matches.  Otherwise the candidate set is the given ids with
 *      query_id - id >= num_exclude_recent, in the given order; "position" is the position in this filtered list, n its length.
 *   S4 (SC:322-328) d2 = sum_r (q[r] - k[r])^2 in fp32, ascending r, result += diff * diff (nanoflann's L2_Simple_Adaptor).  The
 *      num_candidates smallest by (d2, position) are kept, in this order: their ring-key rank.  num_candidates <= 0 or >= n: all, same order.
 *   S5 (SC:104-124, :42-62) shifted(B, s)[:, j] = B[:, (j - s) mod S].  a = argmin_s sqrt(sum_c (vq[c] - vk[(c - s) mod S])^2), ascending c,
 *      the square roots compared with strict < over s = 0 .. S-1 from 1e7 (the lowest shift wins a tie).
 *   S6 (SC:127-159, :80-101) radius = (int)floor(0.5 * search_ratio * S + 0.5).  Shifts: a and (a +- i) mod S, i = 1 .. radius, visited in
 *      ascending numeric order.  Per shift s, per column c ascending: n1 = col_norm_q[c], n2 = col_norm_k[(c - s) mod S]; the column is skipped
 *      if either is 0; otherwise sum += (sum_r q[r][c] * k[r][(c - s) mod S], ascending r) / (n1 * n2) and eff += 1.  dist(s) = 1.0 - sum /
 *      (double)eff (NaN when eff == 0).  The minimum over the shifts with strict < from 1e7; a NaN never wins; a candidate whose shifts all
 *      give NaN reports distance NaN and shift 0.
 *   S7 matches ranked by (distance, ring-key rank), NaN last; the first top_k are returned.  loop_id = the first match's id if its distance
 *      < dist_thresh, else -1; yaw = (float)((double)(float)(shift * ((azimuth_max - azimuth_min) / S)) * M_PI / 180.0) of the first match
 *      (SC:374), 0 without a match.
 *   S8 deviations: a point with a non-finite x, y or intensity is skipped; a stored -0.0 is written as +0.0; the candidate set is rebuilt at
 *      every call (the reference rebuilds its tree every 10th call and indexes the current list with the stale tree's positions); fewer than
 *      num_candidates candidates are scored once each (the reference re-scores index 0); ring-key ties go to the lower position; the
 *      summation orders of S2, S5, S6 are the ones above (Eigen's depend on its SIMD width).
 * One detect call waits for the device once.  set_params may change S3 .. S7 parameters at any time, S1 parameters only while the database
 * is empty.  The capacity doubles as descriptors arrive, up to 65 536. */
typedef struct {
  int32_t num_ring, num_sector;                /* 40, 20 */
  double max_radius, azimuth_max, azimuth_min; /* 80.0, 56.5, -56.5 (what setAzimuthRange(56.5) leaves, loop_detector.cpp:89) */
  int32_t num_exclude_recent, num_candidates;  /* 10, 3 */
  double search_ratio, dist_thresh;            /* 0.1, 0.5 */
} apdgicp_scan_context_params;
typedef struct {
  int32_t id, shift;  /* keyframe id; the column shift of the minimum distance */
  double distance;    /* S6 */
  float ring_d2;      /* S4 */
  int32_t ring_rank;  /* S4: 0 = nearest ring key */
} apdgicp_scan_context_match;
typedef struct apdgicp_scan_context apdgicp_scan_context;
int apdgicp_scan_context_default_params(apdgicp_scan_context_params* p);  /* Scancontext.h's constants after setAzimuthRange(56.5) */
int apdgicp_scan_context_create(const apdgicp_scan_context_params* params, int device, void* stream, apdgicp_scan_context** out);
int apdgicp_scan_context_destroy(apdgicp_scan_context* h);
int apdgicp_scan_context_set_params(apdgicp_scan_context* h, const apdgicp_scan_context_params* params);  /* SC:64-71 and the two knobs */
/* SC:255-269 makeAndSaveScancontextAndKeys: S1 + S2 of one cloud (n >= 0 points, stride_bytes apart, host or device memory, e.g. the
 * pointer apdgicp_scan_filter_points returns; intensity_offset_bytes < 0: intensity 0); *id = 0, 1, 2 ... in the order of the calls */
int apdgicp_scan_context_add(apdgicp_scan_context* h, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device, int32_t* id);
/* a ready descriptor (R x S floats, ring-major, host memory): S2 only (SC:258-265); for saved maps */
int apdgicp_scan_context_add_descriptor(apdgicp_scan_context* h, const float* ring_major_RxS, int32_t* id);
int apdgicp_scan_context_clear(apdgicp_scan_context* h);  /* forgets every descriptor; ids start at 0 again */
int apdgicp_scan_context_size(apdgicp_scan_context* h, int32_t* n);
/* SC:272-379 detectLoopClosureID: S3 .. S7.  matches: room for top_k records; *n_matches = min(top_k, kept candidates).  A candidate id
 * out of range or given twice: APDGICP_ERR_INVALID_ARG. */
int apdgicp_scan_context_detect(apdgicp_scan_context* h, int32_t query_id, const int32_t* candidate_ids, int32_t n_candidates, int32_t top_k,
                                apdgicp_scan_context_match* matches, int32_t* n_matches, int32_t* loop_id, float* yaw_rad);
/* the new keyframes of one LoopDetector::detect call (loop_detector.cpp:102) in one launch sequence: query q's candidates are
 * cand_ids[cand_offsets[q] .. cand_offsets[q + 1]), its records matches[q * top_k ...]; the records equal those of single calls */
int apdgicp_scan_context_detect_batch(apdgicp_scan_context* h, int32_t n_queries, const int32_t* query_ids, const int32_t* cand_offsets, const int32_t* cand_ids,
                                      int32_t top_k, apdgicp_scan_context_match* matches, int32_t* n_matches, int32_t* loop_ids, float* yaws);
/* reads back descriptors first .. first + count - 1 (SC:249-252 getConstRefRecentSCD and the keys): desc count x R x S floats, ring_keys
 * count x R floats, sector_keys and col_norms count x S doubles; any destination may be NULL */
int apdgicp_scan_context_descriptors(apdgicp_scan_context* h, int32_t first, int32_t count, float* desc, float* ring_keys, double* sector_keys, double* col_norms);

/* ------------------------------------------------------------------ DBSCAN clustering (moving objects from the ego-velocity outliers)
 * DBSCANSimpleCluster<PointT>::extract ("DB:" = radar_graph_slam/include/dbscan/DBSCAN_simple.h): the clustering the
 * reference ships for the points the ego-velocity estimate rejects.  DBSCAN_precomp.h stores the same distances and gives the same
 * clusters; DBSCAN_kdtree.h searches through PCL's kd-tree, whose arithmetic is not in the tree: not offered.  The sequential loop of
 * DB:27-90 is equivalent to the following properties, quirks included (tests/dbscan_np.py is the literal loop and checks exactly that):
 *   D1. DB:118-142, adjacency.  Points i != j are adjacent iff  dx*dx + dy*dy + dz*dz <= eps*eps  with dx = (double)(x_j - x_i) -- an fp32
 *       subtraction, then widened --, products and sum in fp64 left to right, eps*eps in fp64.  The relation is symmetric.  A point with a
 *       non-finite coordinate is adjacent to nothing (every comparison with it is false).  The device prunes with an integer grid of cell
 *       side h = eps * (1 + 2^-20): the fp32 difference is within a factor 1 + 2^-24 of the true one and the fp64 quotient x / h within
 *       2^-32 inside the key range, so an accepted pair's quotients are less than 1 apart and its cells at most 1 apart on every axis; the
 *       27 cells around a point hold every pair D1 accepts, and D1's arithmetic decides.  A finite point more than 2^20 cells from the
 *       origin on an axis fails the run with APDGICP_ERR_UNSUPPORTED and a message naming the first such point; the handle stays usable.
 *   D2. DB:124, 141, core.  cnt_i = 1 + the adjacent points: the point itself counts (whatever the comment at DB:112 says).  Core iff
 *       cnt_i >= min_pts.
 *   D3. DB:32-44, 61-70, clusters.  The outer loop opens a cluster at the first unprocessed core point in index order and the BFS closes
 *       it before the loop goes on: a cluster is a connected component of core points under D1, its SEED is its smallest core index,
 *       clusters are created in ascending seed order.  (Device: lock-free union-find, the larger root hooked under the smaller with
 *       32-bit integer atomics; the root of a component is its seed whatever order the atomics land in.)
 *   D4. DB:61-70, border points.  A non-core point adjacent to at least one core point joins the first-created cluster it touches: the
 *       smallest seed among the components of its adjacent cores.  That is its primary label -- also when D6 discards that cluster.  A core
 *       point's primary label is its own seed.  Every other point is noise (-1).
 *   D5. DB:46-51, the seed quirk.  The seed's own neighbours are pushed without a look at their state: a border point that already belongs
 *       to an earlier cluster and is adjacent to the SEED POINT of a later one is also a member of the later one -- in two member lists,
 *       primary label unchanged.  Borders adjacent only to non-seed cores of the later cluster are not.
 *   D6. DB:75, size filter.  size = members of D3 + D4 + D5 (the queue holds no duplicates: DB:82-83 change nothing).  Kept iff
 *       min_cluster_size <= size <= max_cluster_size; the points of a discarded cluster get final label -1.
 *   D7. DB:82, 89, order.  Member lists in ascending index; clusters by size, largest first.  std::sort leaves equal sizes unspecified:
 *       here equal sizes go by ascending seed (a deviation).
 * The table row of a kept cluster is taken over its member list (D5's guests included): the centroid is an fp64 sum of the widened fp32
 * coordinates in a fixed order (lane t of 256 adds members t, t + 256, ... in list order, then a fixed tree) over the size -- the same bits on
 * every run, the last bits may differ from a sequential sum --, min / max are fp32, the Doppler columns likewise when a Doppler lane is given
 * (else 0).  Integer atomics only; no floating-point atomics.
 * One run is 17 + 4 * (8 + p1 + p2) launches (the three radix sorts: 8 passes over the cell keys, p1 = ceil((2 b + 1) / 8) over the rank keys
 * with n <= 2^b, p2 = ceil(bits of K / 8) over the member pairs; 6 fewer and no p2 when K = 0) and ONE wait, for {first refused point, K, CSR length}; a host cloud is staged by a copy on the object's stream. */
typedef struct {
  double eps;                 /* DB:111 eps_ (setClusterTolerance) ; default 0: a run is refused until it is finite and > 0 */
  int32_t min_pts;            /* DB:112 minPts_ (setCorePointMinPts) ; default 1 ; >= 1 */
  int32_t min_cluster_size;   /* DB:113 ; default 1 ; >= 1 */
  int32_t max_cluster_size;   /* DB:114 ; default INT_MAX */
  int32_t reserved;           /* 0 */
} apdgicp_dbscan_params;
typedef struct {
  double centroid[3];
  double doppler_mean;
  float min[3], max[3];       /* axis-aligned extent */
  float doppler_min, doppler_max;
  int32_t seed;               /* D3 */
  int32_t size;               /* D6 */
  int32_t n_core;             /* core members */
  int32_t reserved;
} apdgicp_dbscan_cluster;
typedef struct apdgicp_dbscan apdgicp_dbscan;
void apdgicp_dbscan_default_params(apdgicp_dbscan_params* p);   /* DB:111-114 */
/* The parameters are checked before the device (eps NaN, infinite or negative, min_pts / min_cluster_size < 1, max_cluster_size < 1:
 * APDGICP_ERR_INVALID_ARG); eps = 0 is accepted here and by _set_params -- the reference's default -- and refused by _run.  NULL: the defaults. */
int apdgicp_dbscan_create(const apdgicp_dbscan_params* p, int device, void* stream, apdgicp_dbscan** out);
int apdgicp_dbscan_destroy(apdgicp_dbscan* h);
int apdgicp_dbscan_set_params(apdgicp_dbscan* h, const apdgicp_dbscan_params* p);
/* extract() of one cloud: xyz is the address of the first x, points stride_bytes apart (>= 12, a multiple of 4); doppler: one float per
 * point doppler_stride_bytes apart, or NULL; both in device memory (on_device = 1) or both on the host.  *n_clusters = kept clusters K.
 * n = 0: K = 0, status 0.  More than 2^24 points: APDGICP_ERR_UNSUPPORTED. */
int apdgicp_dbscan_run(apdgicp_dbscan* h, const float* xyz, int64_t n, int64_t stride_bytes, const float* doppler, int64_t doppler_stride_bytes, int on_device,
                       int32_t* n_clusters);
/* device memory, valid until the next run: one int32 per point, the rank (D7) of its kept primary cluster or -1 */
int apdgicp_dbscan_labels(apdgicp_dbscan* h, const int32_t** device_labels, int64_t* n);
int apdgicp_dbscan_copy_labels(apdgicp_dbscan* h, int32_t* labels, int64_t capacity);                       /* the same, to HOST memory */
int apdgicp_dbscan_clusters(apdgicp_dbscan* h, apdgicp_dbscan_cluster* table, int64_t capacity);            /* K rows in rank order, HOST memory */
/* the member lists as CSR, HOST memory: offsets [K + 1], indices [offsets[K]] (cluster r: indices[offsets[r] .. offsets[r + 1]), ascending;
 * a point of D5 is listed by both clusters); *n_indices = offsets[K].  Any destination may be NULL; too small: APDGICP_ERR_INVALID_ARG. */
int apdgicp_dbscan_members(apdgicp_dbscan* h, int32_t* offsets, int64_t offsets_capacity, int32_t* indices, int64_t indices_capacity, int64_t* n_indices);
/* before the size filter, HOST memory, capacity >= n entries each, any may be NULL (for tests): cnt (D2), core 0 / 1, root (a core point's
 * seed, else -1), primary (D4: the seed of the primary cluster, -1 noise) */
int apdgicp_dbscan_debug(apdgicp_dbscan* h, int32_t* cnt, uint8_t* core, int32_t* root, int32_t* primary, int64_t capacity);
/* For the measurement scripts.  _set_profiling(1): a run records events at its phase boundaries and waits a second time, at its end.
 * _stats: kernel launches and host waits of the last run as counted by the host code that enqueued them, and (profiling on, else zeros) the
 * device time between the boundaries in ms: {cells + sort + sorted copy, count, union + flatten, border, everything behind it -- rank sort,
 * the wait, member lists, labels, table}.  Any destination may be NULL. */
int apdgicp_dbscan_set_profiling(apdgicp_dbscan* h, int enable);
int apdgicp_dbscan_stats(apdgicp_dbscan* h, int64_t* launches, int64_t* waits, double phase_ms[5]);

/* ------------------------------------------------------------------ scan ingest and deskew: the two ends of cloud_callback
 * What PreprocessingNodelet::cloud_callback ("P:" = radar_graph_slam/apps/preprocessing_nodelet.cpp) does to the message before the
 * ego-velocity estimate (P:667-697; the hugin callback P:497-506) and to src_cloud between that estimate and distance_filter
 * (deskewing P:914-975, the base-link transform P:796-810).  With this object every per-point step of the callback is on the device:
 *   _run (or _run_polar) -> apdgicp_ego_velocity_run on the rows -> its inliers (or the rows) -> _deskew -> apdgicp_scan_filter_run -> apdgicp_set_source.
 *   I1. Lanes (P:667-683, P:497-506).  A point's x, y, z are three consecutive floats at xyz + i * xyz_stride_bytes; intensity (the
 *       message's "Power") and doppler are one float each at their own base and stride.  geometry_msgs::Point32[] plus channels[2] /
 *       channels[0]: strides 12 / 4 / 4.  A sensor_msgs::PointCloud2 or any array of structures: all strides = point_step, the bases
 *       offset by the field offsets.  Strides are multiples of 4, >= 12 / 4 / 4.  Input order is kept.  on_device = 0: the lanes are
 *       staged by copies on the object's stream without a wait (one copy when they are fields of one array of structures).
 *   I2. Gate (P:670-673), gate = 1.  A point is kept iff power > power_threshold (fp32; a NaN power fails) and none of x, y, z equals
 *       +infinity.  The reference's `== NAN` tests are never true: a NaN coordinate is kept.  -infinity is kept.  gate = 0 (P:497-506):
 *       every point is kept.
 *   I3. Pre-transform (P:477-480), applied to the kept points.  pre_transform == NULL: none.  Otherwise x, y, z become rows 0..2 of the
 *       column-major 4x4 times (x, y, z, 1) in fp32: (r0 x + r1 y) + (r2 z + t), or ((r0 x + r1 y) + r2 z) + t with
 *       APDGICP_FLAG_XF_LINEAR_CHAIN in params.flags -- the order of apdgicp_params.flags and of M1 of the map cloud.  Eigen's own order
 *       is not pinned by the reference tree.
 *   I4. Output of _run.  n_out rows of 32 bytes {x, y, z, intensity, doppler, 0, 0, 0}: what apdgicp_ego_velocity_run(..., stride 32,
 *       intensity offset 12, doppler offset 16, on_device = 1) accepts, and apdgicp_scan_filter_run, apdgicp_set_source and
 *       apdgicp_dbscan_run likewise.  Beside the rows one int32 per row: the point's index in the message.  One host wait per run, for
 *       n_out.  n = 0: n_out = 0, status 0.  At most 2^24 points (indices are int32, the block counts are scanned by one block);
 *       above: APDGICP_ERR_UNSUPPORTED.
 *   I5. Deskew (P:951-972), per point i of n in the order of the input cloud (the rows of _run, the ego-velocity inlier cloud, any
 *       xyzi cloud), v = its (x, y, z):
 *         a_k = -(float)ang_vel[k];  dt = (scan_period * (double)i) / (double)n;  h = dt / 2.0;
 *         q = ((float)(h * (double)a_x), (float)(h * (double)a_y), (float)(h * (double)a_z)), qw = 1.0f;
 *         Quaternionf::inverse():  n2 = (qx qx + qy qy) + (qz qz + qw qw), each product rounded on its own, no FMA; with
 *           APDGICP_FLAG_XF_LINEAR_CHAIN ((qx qx + qy qy) + qz qz) + qw qw.  n2 > 0: c = (-qx / n2, -qy / n2, -qz / n2), cw = qw / n2
 *           (IEEE divisions); otherwise (a NaN rate) c = 0, cw = 0: Eigen's zero quaternion.
 *         Quaternion::_transformVector, literally (the quaternion is not of unit length):  uv = c x v;  uv = uv + uv;
 *           out = (v + cw * uv) + (c x uv)  with  a x b = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x),
 *           everything fp32 without contraction.
 *       The intensity is copied.  ang_vel == NULL (imu_queue.empty(), P:916): the cloud passes through bit for bit.  Eigen's reduction
 *       order for squaredNorm() is not pinned by the reference tree (the two orders above are those of the two Eigen generations named
 *       at XF_LINEAR_CHAIN).  Which message of the IMU queue supplies ang_vel (P:939-949) is host bookkeeping: select_imu of the
 *       Python package, ScanIngestHip::selectImu.
 *   I6. Frame transform (P:796-810), behind the deskew in the same launch.  T == NULL: none; otherwise as I3.
 *   I7. Output of _deskew.  n rows {x, y, z, intensity} of 16 bytes: what apdgicp_scan_filter_run(on_device = 1) and
 *       apdgicp_set_source accept; valid until the next _deskew.  No host wait: n is the caller's.  A consumer on another stream orders
 *       itself behind the launch with _synchronize (or shares the object's stream).  The call is legal on the rows the same object's
 *       _run produced and on any other device or host cloud.
 * The polar message: _run_polar is the head of cloud_callback_scan (P:324-464), the callback of every dataset that is neither hugin
 * nor eagle -- a msgs_radar/RadarScanExtended with range, azimuth, elevation, velocity and snr per target.  Behind it the chain is the one
 * above, with the ego-velocity inlier cloud always as the source (P:416-420).
 *   PI1. Lanes (P:331-337).  Five byte-strided float lanes as in I1: range, azimuth, elevation, snr, velocity, each one float per target
 *       at its own base and stride; strides are multiples of 4 and >= 4.  A RadarTargetExtended[] is one array of 76-byte structures
 *       (19 floats): all strides 76, the bases at the field offsets 0 / 4 / 8 / 16 / 12.  The lanes are all on the host or all on the
 *       device.  on_device = 0: staged by copies on the object's stream without a wait; one copy when all five lie inside one array of
 *       structures (same stride, bases within one stride of each other), as I1.
 *   PI2. No gate.  P:331-340 pushes every target: n_out = n, power_threshold and gate are not read, non-finite values pass through.  No
 *       count, no scan and NO HOST WAIT: *n_out is written from n.
 *   PI3. Coordinates (P:333-335).  `using namespace std;` (P:47) makes the unqualified cos / sin of a float member the float overloads, so
 *       the reference is x = (range * cosf(el)) * cosf(az), y = (range * cosf(el)) * sinf(az), z = (-range) * sinf(el), all fp32, left to
 *       right, each product rounded on its own, no FMA.  The C library's cosf / sinf are not correctly rounded and their algorithm is not
 *       restated here (apd_atan2f.h covers atan2f only).  The device defines each of the four factors as THE FP64 VALUE ROUNDED ONCE TO
 *       FP32: for |angle| <= pi, (float)cos((double)angle) and (float)sin((double)angle) through sincos_pi (csrc/apd_math.hpp, at most
 *       0.77 ulp in fp64); for any other argument, NaN and +-inf included, through the device library's fp64 sincos.  The three products
 *       follow in fp32 exactly as written above, without contraction.
 *       Deviation from the reference: a factor can differ from the C library's by one fp32 ulp.  Measured against glibc 2.35
 *       (tests/test_polar_ingest_cpu.py): over every 64th float of [2^-20, 1.6] cosf differs from the rounded fp64 value in 0.13 % and
 *       sinf in 0.47 % of the arguments, never by more than one ulp; over 2 000 000 targets (range 2 .. 100 m, azimuth +-0.986 rad,
 *       elevation +-0.262 rad) 0.54 % / 1.85 % / 1.90 % of x / y / z differ at all, by 3 / 2 / 2 ulps at most (the derived bound is 6:
 *       two factors off by one ulp each and two product roundings).
 *   PI4. Output.  n rows of 32 bytes {x, y, z, snr, velocity, 0, 0, 0} and index[i] = i, in input order, from one launch; _points,
 *       _copy and _stats serve them as they serve _run's.  n = 0: status 0, no launch.  n > 2^24: APDGICP_ERR_UNSUPPORTED.  A stride that
 *       is not a multiple of 4 or is below 4, a NULL lane with n > 0, n < 0: APDGICP_ERR_INVALID_ARG.  After an error the object stays
 *       usable and the rows of the last good run stay readable.
 *   PI5. Interplay.  A _run_polar after a _run, or the other way round, replaces the rows; a smaller second run leaves nothing of the
 *       first visible (n of _points is the new one).  _deskew on the object's own polar rows is legal (I7).
 * The distance histogram that ends all three callbacks (P:451-461, P:618-628, P:818-828; num_frame is never incremented, so it runs on
 * every frame) and the point_distribution command that reads it (P:1009-1021):
 *   H1. Per point d = sqrtf((x * x + y * y) + z * z) in fp32, each product rounded on its own, no FMA: the writing of
 *       getVector3fMap().norm() that the scan filter's range gate uses.  b = (int)floorf(d); the point is counted in bin b iff d is finite
 *       and b < 100.  A non-finite d is NOT counted: the reference converts it to int, which is undefined, and on x86 the result
 *       (INT_MIN) passes `dist < 100` and indexes out of bounds.
 *   H2. _histogram_add costs two launches (zero the frame's counts, then count) and NO HOST WAIT.  It leaves the frame's 100 int32 counts
 *       on the device, adds them to a running int64[100] sum on the device and increments a frame counter there.  Per-block LDS
 *       histograms with 32-bit integer atomics, then at most 100 integer atomic adds per block to global memory; integer addition
 *       commutes, so the bytes are the same on every run.  n = 0 is a frame of zeros, as the reference pushes one.
 *   H3. _histogram_last returns the counts of the last _add (zeros before the first), _histogram_read the running sum and the number of
 *       frames; either of its two destinations may be NULL.  The point_distribution command is the sum divided by frames, element-wise, as
 *       integer division.  The reference adds into an Eigen::VectorXi data(100) that was never zeroed; this sum starts from zero.
 *       _histogram_reset zeroes the counts, the sum and the frame counter (no wait).
 *   H4. Errors as PI4.  stride_bytes >= 12 and a multiple of 4.  The input can be the cloud of apdgicp_scan_filter_points (16-byte rows),
 *       the ingest rows (32 bytes) or any host cloud; a producer on another stream is the caller's to order, as for _deskew.
 * Not part of this object: the ranges / predicted_ranges topics (P:660-700), the colour cloud (P:921-937), the Doppler statistics of the
 * outlier cloud (P:395-405: nothing reads them), underfloor_filter (its result is unused, P:449, P:816). */
typedef struct {
  float power_threshold;   /* "power_threshold", P:107 ; default 0 */
  int32_t gate;            /* 1 (default): I2 ; 0: every point is kept (P:497-506) */
  int32_t flags;           /* 0 or APDGICP_FLAG_XF_LINEAR_CHAIN (I3, I5, I6) */
  int32_t reserved;        /* 0 */
} apdgicp_scan_ingest_params;
typedef struct apdgicp_scan_ingest apdgicp_scan_ingest;
void apdgicp_scan_ingest_default_params(apdgicp_scan_ingest_params* p);
/* `stream` may be NULL (the object creates its own) or a hipStream_t of the caller; params NULL: the defaults */
int apdgicp_scan_ingest_create(const apdgicp_scan_ingest_params* p, int device, void* stream, apdgicp_scan_ingest** out);
int apdgicp_scan_ingest_destroy(apdgicp_scan_ingest* h);
int apdgicp_scan_ingest_set_params(apdgicp_scan_ingest* h, const apdgicp_scan_ingest_params* p);
/* I1 .. I4 of one message; the three lanes all in device memory (on_device = 1) or all on the host; pre_transform: float[16] column-major or NULL */
int apdgicp_scan_ingest_run(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t xyz_stride_bytes, const float* intensity, int64_t intensity_stride_bytes,
                            const float* doppler, int64_t doppler_stride_bytes, int on_device, const float* pre_transform, int64_t* n_out);
/* PI1 .. PI5 of one polar message; the five lanes all in device memory (on_device = 1) or all on the host.  Does not wait. */
int apdgicp_scan_ingest_run_polar(apdgicp_scan_ingest* h, const float* range, int64_t range_stride_bytes, const float* azimuth, int64_t azimuth_stride_bytes,
                                  const float* elevation, int64_t elevation_stride_bytes, const float* snr, int64_t snr_stride_bytes, const float* velocity,
                                  int64_t velocity_stride_bytes, int64_t n, int on_device, int64_t* n_out);
/* the rows of the last run and their message indices in device memory, valid until the next run; any pointer but h may be NULL */
int apdgicp_scan_ingest_points(apdgicp_scan_ingest* h, const float** device_rows, const int32_t** device_index, int64_t* n);
/* the same to HOST memory: rows [8 * capacity] floats, index [capacity]; either may be NULL */
int apdgicp_scan_ingest_copy(apdgicp_scan_ingest* h, float* rows, int32_t* index, int64_t capacity);
/* I5 .. I7: xyz / n / stride_bytes / intensity_offset_bytes (< 0: none, 0 is kept) / on_device as in apdgicp_scan_filter_run;
 * ang_vel: double[3] (the IMU message's angular_velocity, HOST memory) or NULL; T: float[16] column-major (HOST memory) or NULL */
int apdgicp_scan_ingest_deskew(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device,
                               const double* ang_vel, double scan_period, const float* T);
/* the cloud of the last deskew in device memory (I7); any pointer but h may be NULL */
int apdgicp_scan_ingest_deskewed(apdgicp_scan_ingest* h, const float** device_xyzi, int64_t* n);
int apdgicp_scan_ingest_deskewed_copy(apdgicp_scan_ingest* h, float* xyzi, int64_t capacity);   /* the same to HOST memory, [4 * capacity] floats; waits */
int apdgicp_scan_ingest_synchronize(apdgicp_scan_ingest* h);                                      /* waits for the object's stream (I7) */
/* H1 .. H4: one frame of the distance histogram from a device or host cloud (xyz first); does not wait */
int apdgicp_scan_ingest_histogram_add(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device);
int apdgicp_scan_ingest_histogram_last(apdgicp_scan_ingest* h, int32_t counts[100]);                 /* waits */
int apdgicp_scan_ingest_histogram_read(apdgicp_scan_ingest* h, int64_t sum[100], int64_t* frames);   /* waits */
int apdgicp_scan_ingest_histogram_reset(apdgicp_scan_ingest* h);
/* kernel launches and host waits of the last _run, _run_polar, _deskew or _histogram_add as counted by the host code that enqueued them (for the measurement scripts) */
int apdgicp_scan_ingest_stats(apdgicp_scan_ingest* h, int64_t* launches, int64_t* waits);

#ifdef __cplusplus
}
#endif
#endif /* APDGICP_HIP_H */
