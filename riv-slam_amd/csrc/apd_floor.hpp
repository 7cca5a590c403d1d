// Floor plane detection and under-floor removal on the device: radar_graph_slam::FloorDetectionNodelet
// (radar_graph_slam/apps/floor_detection_nodelet.cpp), the per-scan consumer of the raw cloud whose coefficients become the ground-plane
// factor of every keyframe and whose clipped cloud is published for the rest of the chain:
//   .cpp:75-80    the callback's memory: prev_coeffs = (0, 0, 0, sensor_height - height_clip_range), ground_intialized = false;
//   .cpp:97-134   cloud_callback: detect(); a detected floor replaces prev_coeffs; without one the previous coefficients (or (0, 0, 1, 0)
//                 before the first detection) are published; the under-floor clip plane_clip(cloud, prev_coeffs + (0, 0, 0, floor_tolerance), false);
//   .cpp:154-249  detect(): the tilt transform, the two height clips (:162-163), normal_filtering, the inverse tilt (:169), the two
//                 "too few" tests (:177, :192), pcl::RandomSampleConsensus on a SampleConsensusModelPlane with threshold 0.06 (:183-186),
//                 the verticality test against tilt^-1 * e_z (:198-208), the upward flip (:211-213), the inlier cloud (:215-222);
//   .cpp:258-273  plane_clip: pcl::PlaneClipper3D::clipPointCloud3D + ExtractIndices (negative or not);
//   .cpp:280-307  normal_filtering: pcl::NormalEstimation with k = 10, |normalized normal . e_z| > cos(normal_filter_thresh).
// PCL is not part of the reference tree; the kernels follow its published algorithm (filters/impl/plane_clipper3D.hpp,
// features/impl/normal_3d.hpp, sample_consensus/impl/sac_model_plane.hpp: computeModelCoefficients / countWithinDistance,
// sample_consensus/impl/ransac.hpp: computeModel).  The reference scores its hypotheses one after another; here all K <= 1024 are scored
// in one pass over the filtered points (k_floor_score) and the sequential loop is replayed over the counts (k_floor_replay): given the
// same samples the result is that of the sequential loop.
//
// Deviations and operation orders that belong to PCL / Eigen and not to the reference, all stated in include/apdgicp_hip.h:
//   - sin / cos of the tilt: in double, rounded to fp32; R_y = {c, 0, s; 0, (1 - c) + c, 0; -s, 0, c}; a transformed coordinate is
//     (r0 x + r1 y) + r2 z (the translation column is zero and is not added); tilt_matrix.inverse() is the fp32 TRANSPOSE;
//   - a plane distance is ((a x + b y) + c z) + d (PlaneClipper3D, countWithinDistance and the model's d = -((nx x0 + ny y0) + nz z0));
//   - the normal statistic comes from the fp64 population covariance of the k nearest points (the KNN_EPI_COV sums) and sym3_eig, not
//     from PCL's fp32 covariance and eigen33; |u_z| / |u|: the viewpoint flip (setViewPoint, :289) cannot change an absolute value, so
//     it is not evaluated;
//   - PCL's sampler (boost::mt19937 + its own shuffling, isSampleGood retries) cannot be reproduced: the caller supplies three words per
//     hypothesis and ego_sample() (apd_ego.hpp) turns them into three distinct rows; a collinear sample is a skipped iteration;
//   - cross product, squared norm ((x x + y y) + z z), division by the norm: each fp32 operation rounded on its own;
//   - pow(w, 3) of the adaptive iteration count is (w w) w.
// No floating-point atomics; integer counts use atomicAdd.  Every pointer of this file is a kernel argument (see apd_ego.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "apd_ego.hpp"
#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int FLOOR_BLK = EGO_BLK;    // compaction kernels: 16 waves, one point per lane (ego_block_counts / ego_block_slot)
constexpr int FLOOR_TILE = 256;       // points of a scoring block, one per lane
constexpr int FLOOR_GROUP = 64;       // hypotheses of a scoring block
constexpr int FLOOR_MAX_K = 1024;
enum { FLOOR_NF_OFF = 0, FLOOR_NF_STAT = 1, FLOOR_NF_NONE = 2 };
enum { FLOOR_OK = 0, FLOOR_FEW_POINTS = 1, FLOOR_NO_MODEL = 2, FLOOR_FEW_INLIERS = 3, FLOOR_NOT_HORIZONTAL = 4 };

struct FloorParams {  // the device's view of apdgicp_floor_params
  float R[9], Ri[9];  // the tilt rotation and its inverse, row-major
  float ref[3];       // tilt^-1 * e_z (:198)
  float d_hi, d_lo;   // (float)(sensor_height + height_clip_range), (float)(sensor_height - height_clip_range) (:162-163)
  float pad_;
  double cos_nf, cos_fn, dist_thr, log_prob, floor_tol;
  int pts_thresh, max_iter, K, nf_mode;
};

struct FloorState {  // what cloud_callback remembers from scan to scan (:75-80)
  float prev[4];
  int initialized;
  int pad_[3];
};

struct FloorRecord {  // head: apdgicp_floor_result, byte for byte
  float coeffs[4], raw[4];
  int detected, ground_initialized, reject_reason, n_input;
  int n_clipped, n_filtered, n_inliers, n_under_floor;
  int iterations, skipped, winner, table_exhausted;
  int K, n_inlier_list, reserved[2];
};

__device__ __forceinline__ float floor_plane_dist(float a, float b, float c, float d, float x, float y, float z) {  // ((a x + b y) + c z) + d
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
}
__device__ __forceinline__ float floor_dot3(float a, float b, float c, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z));
}
__device__ __forceinline__ float4 floor_rotate(const float* M, float4 p) {  // pcl::transformPointCloud with a pure rotation; intensity carried
  return make_float4(floor_dot3(M[0], M[1], M[2], p.x, p.y, p.z), floor_dot3(M[3], M[4], M[5], p.x, p.y, p.z), floor_dot3(M[6], M[7], M[8], p.x, p.y, p.z), p.w);
}
__device__ __forceinline__ bool floor_inlier(float4 c, float4 p, double thr) {  // countWithinDistance / selectWithinDistance; a NaN is an outlier
  return (double)fabsf(floor_plane_dist(c.x, c.y, c.z, c.w, p.x, p.y, p.z)) < thr;
}

__global__ void k_floor_reset(FloorState* st, float d0) {  // initialize_params (:75-80)
  if (threadIdx.x == 0 && blockIdx.x == 0) st->prev[0] = st->prev[1] = st->prev[2] = 0.f, st->prev[3] = d0, st->initialized = 0;
}

// ---- stage 1 (:156-163): one lane per point.  tilted[i] = {R p, intensity}; mask[i] = inside the height band:
// plane_clip(+, negative = false) keeps distance >= 0, plane_clip(-, negative = true) keeps the points that are NOT at distance >= 0.
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_clip(const float* pts, int n, int stride /* floats */, int ioff /* < 0: none */, FloorParams P, float4* tilted,
                                                          unsigned char* mask, int* bsum) {
  __shared__ int wsum[FLOOR_BLK / 64];
  const int i = blockIdx.x * FLOOR_BLK + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const auto p = pts + (size_t)i * stride;
    const float4 t = floor_rotate(P.R, make_float4(p[0], p[1], p[2], ioff >= 0 ? p[ioff] : 0.f));
    ok = floor_plane_dist(0.f, 0.f, 1.f, P.d_hi, t.x, t.y, t.z) >= 0.f && !(floor_plane_dist(0.f, 0.f, 1.f, P.d_lo, t.x, t.y, t.z) >= 0.f);
    tilted[i] = t;
    mask[i] = ok ? 1 : 0;
  }
  ego_block_counts(ok, wsum, bsum);
}
// ... and their in-order compaction (bsum: scanned by k_scan_bsum, which also left n_clipped in the record)
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_compact(const float4* tilted, const unsigned char* mask, int n, const int* bsum, float4* clip, int* clip_src) {
  __shared__ int wsum[FLOOR_BLK / 64];
  const int i = blockIdx.x * FLOOR_BLK + threadIdx.x;
  const bool ok = i < n && mask[i];
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (ok) clip[slot] = tilted[i], clip_src[slot] = i;
}

// ---- stage 2 (:280-307): the statistic is the KNN_EPI_NORMALZ epilogue of knn_cov_coop_wave (apd_kernels.hpp; launched through
// k_knn_stat_coop of apd_filter.hpp); here the decision and, in the same compaction, the inverse tilt (:169).
__device__ __forceinline__ bool floor_nf_keep(const float* stat, const FloorParams& P, int n_clip, int i) {
  if (i >= n_clip || P.nf_mode == FLOOR_NF_NONE) return false;   // (fewer than k points: PCL's normals are NaN, nothing passes)
  return P.nf_mode == FLOOR_NF_OFF || (double)stat[i] > P.cos_nf;  // std::abs(dot) > std::cos(...), a NaN fails
}
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_nf_count(const float* stat, FloorParams P, const FloorRecord* rec, int* bsum) {
  __shared__ int wsum[FLOOR_BLK / 64];
  ego_block_counts(floor_nf_keep(stat, P, rec->n_clipped, blockIdx.x * FLOOR_BLK + threadIdx.x), wsum, bsum);
}
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_nf_scatter(const float4* clip, const int* clip_src, const float* stat, FloorParams P, const FloorRecord* rec,
                                                                const int* bsum, float4* filt, int* filt_src) {
  __shared__ int wsum[FLOOR_BLK / 64];
  const int i = blockIdx.x * FLOOR_BLK + threadIdx.x;
  const bool ok = floor_nf_keep(stat, P, rec->n_clipped, i);
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (ok) filt[slot] = floor_rotate(P.Ri, clip[i]), filt_src[slot] = clip_src[i];
}

// ---- stage 3 (SampleConsensusModelPlane::computeModelCoefficients): one lane per hypothesis
__global__ __launch_bounds__(64) void k_floor_hypotheses(const float4* filt, const unsigned* words, FloorParams P, const FloorRecord* rec, float4* coef, unsigned char* bad,
                                                         int* samples) {
  const int k = blockIdx.x * 64 + threadIdx.x, m = rec->n_filtered;
  if (k >= P.K || m < P.pts_thresh || m < 3) return;  // (:177; three distinct rows need three points)
  int s[3];
  ego_sample(words + (size_t)k * 3, 3, m, s);
  samples[3 * k] = s[0], samples[3 * k + 1] = s[1], samples[3 * k + 2] = s[2];
  const float4 p0 = filt[s[0]], p1 = filt[s[1]], p2 = filt[s[2]];
  const float ax = __fsub_rn(p1.x, p0.x), ay = __fsub_rn(p1.y, p0.y), az = __fsub_rn(p1.z, p0.z);
  const float bx = __fsub_rn(p2.x, p0.x), by = __fsub_rn(p2.y, p0.y), bz = __fsub_rn(p2.z, p0.z);
  const float rx = __fdiv_rn(ax, bx), ry = __fdiv_rn(ay, by), rz = __fdiv_rn(az, bz);  // dy1dy2 = p1p0 / p2p0
  if (rx == ry && rz == ry) {  // collinear
    bad[k] = 1;
    return;
  }
  float nx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
  float ny = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
  float nz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
  const float norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
  nx = __fdiv_rn(nx, norm), ny = __fdiv_rn(ny, norm), nz = __fdiv_rn(nz, norm);  // (sqrtf and the division: correctly rounded)
  coef[k] = make_float4(nx, ny, nz, -floor_dot3(nx, ny, nz, p0.x, p0.y, p0.z));
}

// ---- stage 4 (countWithinDistance), the hot pass: grid (point tiles of 256) x (groups of 64 hypotheses).  A lane holds its point in
// registers and walks the group's coefficients out of LDS (wave-uniform reads); per hypothesis ballot + popcount per wave, the four
// waves added in LDS, one integer atomicAdd per (block, hypothesis).
__global__ __launch_bounds__(FLOOR_TILE) void k_floor_score(const float4* filt, const float4* coef, const unsigned char* bad, FloorParams P, const FloorRecord* rec, int* n_in) {
  __shared__ float4 sc[FLOOR_GROUP];
  __shared__ int sbad[FLOOR_GROUP];
  __shared__ int wcnt[FLOOR_TILE / 64][FLOOR_GROUP];
  const int m = rec->n_filtered, tid = threadIdx.x, i = blockIdx.x * FLOOR_TILE + tid, k0 = blockIdx.y * FLOOR_GROUP;
  if (m < P.pts_thresh || m < 3 || (int)blockIdx.x * FLOOR_TILE >= m) return;  // (block-uniform)
  const int kn = min(FLOOR_GROUP, P.K - k0);
  if (tid < kn) sc[tid] = coef[k0 + tid], sbad[tid] = bad[k0 + tid];
  __syncthreads();
  const bool live = i < m;
  const float4 p = filt[live ? i : m - 1];
  for (int g = 0; g < kn; g++) {
    const bool in = live && !sbad[g] && floor_inlier(sc[g], p, P.dist_thr);
    const int c = __popcll(__ballot(in));
    if ((tid & 63) == 0) wcnt[tid >> 6][g] = c;
  }
  __syncthreads();
  if (tid < kn) {
    const int c = (wcnt[0][tid] + wcnt[1][tid]) + (wcnt[2][tid] + wcnt[3][tid]);
    if (c) atomicAdd(&n_in[k0 + tid], c);
  }
}

// ---- stage 5 (RandomSampleConsensus::computeModel over the counts, then detect():177-213 and cloud_callback:100-130): ONE block, lane 0
// walks the hypotheses in order.  k = log(1 - probability) / log(1 - w^3) is recomputed whenever a hypothesis has strictly more inliers.
__global__ __launch_bounds__(64) void k_floor_replay(const float4* coef, const unsigned char* bad, const int* n_in, FloorParams P, FloorRecord* rec, FloorState* st) {
  if (threadIdx.x != 0) return;
  const int m = rec->n_filtered;
  int it = 0, skipped = 0, best = -1, n_best = -2147483647, exhausted = 0;
  if (m >= P.pts_thresh && m >= 3) {
    double kk = 1.0;
    const double one_over = 1.0 / (double)m, eps = 2.220446049250313e-16;
    const long long max_skip = (long long)P.max_iter * 10;
    int idx = 0;
    while ((double)it < kk && (long long)skipped < max_skip) {
      if (idx == P.K) {  // PCL would have drawn another sample: the caller has to supply more words
        exhausted = 1;
        break;
      }
      const int k = idx++;
      if (bad[k]) {
        skipped++;
        continue;
      }
      const int c = n_in[k];
      if (c > n_best) {
        n_best = c, best = k;
        const double w = __dmul_rn((double)c, one_over);
        double p_no = 1.0 - __dmul_rn(__dmul_rn(w, w), w);
        p_no = fmax(eps, p_no);
        p_no = fmin(1.0 - eps, p_no);
        kk = P.log_prob / log(p_no);
      }
      it++;
      if (it > P.max_iter) break;
    }
  }
  int reason = FLOOR_OK;
  float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m < P.pts_thresh) reason = FLOOR_FEW_POINTS;        // :177
  else if (best < 0) reason = FLOOR_NO_MODEL;              // computeModel returned false: no inliers (:192)
  else {
    c = coef[best];
    rec->raw[0] = c.x, rec->raw[1] = c.y, rec->raw[2] = c.z, rec->raw[3] = c.w;
    rec->n_inliers = n_best;
    if (n_best < P.pts_thresh) reason = FLOOR_FEW_INLIERS;  // :192
    else if (fabs((double)floor_dot3(c.x, c.y, c.z, P.ref[0], P.ref[1], P.ref[2])) < P.cos_fn) reason = FLOOR_NOT_HORIZONTAL;  // :203-208
    else if (c.z < 0.f) c = make_float4(__fmul_rn(c.x, -1.f), __fmul_rn(c.y, -1.f), __fmul_rn(c.z, -1.f), __fmul_rn(c.w, -1.f));  // :211-213
  }
  const int detected = reason == FLOOR_OK;
  if (detected) st->prev[0] = c.x, st->prev[1] = c.y, st->prev[2] = c.z, st->prev[3] = c.w, st->initialized = 1;  // :102-111
  if (st->initialized) rec->coeffs[0] = st->prev[0], rec->coeffs[1] = st->prev[1], rec->coeffs[2] = st->prev[2], rec->coeffs[3] = st->prev[3];  // :114-118
  else rec->coeffs[0] = 0.f, rec->coeffs[1] = 0.f, rec->coeffs[2] = 1.f, rec->coeffs[3] = 0.f;                                                  // :120-127
  rec->detected = detected, rec->ground_initialized = st->initialized, rec->reject_reason = reason;
  rec->iterations = it, rec->skipped = skipped, rec->winner = best, rec->table_exhausted = exhausted;
}

// ---- the two lists.  Per lane two flags: a = filtered point i is an inlier of the winning model (a detected floor only: floor_points,
// :215-222), b = input point i is not below the remembered floor (:132-134).  Count, scan, scatter -- the scheme of k_ego_emit_*.
__device__ __forceinline__ void floor_flags(const float4* filt, const float* pts, int n, int stride, const FloorParams& P, const FloorRecord* rec, const FloorState* st, int i,
                                            bool& a, bool& b) {
  a = b = false;
  if (rec->detected && i < rec->n_filtered) a = floor_inlier(make_float4(rec->raw[0], rec->raw[1], rec->raw[2], rec->raw[3]), filt[i], P.dist_thr);
  if (i < n) {
    const auto p = pts + (size_t)i * stride;
    const float d = (float)((double)st->prev[3] + P.floor_tol);  // Eigen::Vector4f(..., prev_coeffs.coeffs[3] + floor_tolerance)
    b = floor_plane_dist(st->prev[0], st->prev[1], st->prev[2], d, p[0], p[1], p[2]) >= 0.f;
  }
}
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_emit_count(const float4* filt, const float* pts, int n, int stride, FloorParams P, const FloorRecord* rec,
                                                                const FloorState* st, int* bsum_a, int* bsum_b) {
  __shared__ int wsum[FLOOR_BLK / 64];
  bool a, b;
  floor_flags(filt, pts, n, stride, P, rec, st, blockIdx.x * FLOOR_BLK + threadIdx.x, a, b);
  ego_block_counts(a, wsum, bsum_a);
  ego_block_counts(b, wsum, bsum_b);
}
__global__ __launch_bounds__(SCAN_BLK) void k_floor_emit_scan(int* bsum_a, int* bsum_b, int nb, FloorRecord* rec) {  // ONE block: k_scan_bsum for both
  __shared__ int lds[SCAN_BLK / 64];
  const int tid = threadIdx.x;
  int carry_a = 0, carry_b = 0;
  for (int b0 = 0; b0 < nb; b0 += SCAN_BLK) {
    const int i = b0 + tid;
    int total;
    const int ea = block_exclusive_scan(i < nb ? bsum_a[i] : 0, lds, tid, &total);
    if (i < nb) bsum_a[i] = carry_a + ea;
    carry_a += total;
    const int eb = block_exclusive_scan(i < nb ? bsum_b[i] : 0, lds, tid, &total);
    if (i < nb) bsum_b[i] = carry_b + eb;
    carry_b += total;
  }
  if (tid == 0) rec->n_inlier_list = carry_a, rec->n_under_floor = carry_b;
}
__global__ __launch_bounds__(FLOOR_BLK) void k_floor_emit_scatter(const float4* filt, const int* filt_src, const float* pts, int n, int stride, int ioff, FloorParams P,
                                                                  const FloorRecord* rec, const FloorState* st, const int* bsum_a, const int* bsum_b, float4* in_xyzi,
                                                                  int* in_src, int* in_row, float4* under_xyzi, int* under_src) {
  __shared__ int wsum[FLOOR_BLK / 64];
  const int i = blockIdx.x * FLOOR_BLK + threadIdx.x;
  bool a, b;
  floor_flags(filt, pts, n, stride, P, rec, st, i, a, b);
  const int slot_a = ego_block_slot(a, wsum, bsum_a[blockIdx.x]);
  const int slot_b = ego_block_slot(b, wsum, bsum_b[blockIdx.x]);
  if (a) in_xyzi[slot_a] = filt[i], in_src[slot_a] = filt_src[i], in_row[slot_a] = i;
  if (b) {
    const auto p = pts + (size_t)i * stride;
    under_xyzi[slot_b] = make_float4(p[0], p[1], p[2], ioff >= 0 ? p[ioff] : 0.f), under_src[slot_b] = i;
  }
}

}  // namespace apd
