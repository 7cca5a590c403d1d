// Doppler ego-velocity estimation and moving-point removal on the device: rio::RadarEgoVelocityEstimator::estimate
// (radar_graph_slam/src/radar_ego_velocity_estimator.cpp, include/radar_ego_velocity_estimator.h), the step
// PreprocessingNodelet::cloud_callback runs right before its three filters (preprocessing_nodelet.cpp:708-741):
//   .cpp:75-91    per point: r = |p| (double), azimuth / elevation from std::atan2(float, float), the field-of-view / SNR gate, the
//                 row {x/r, y/r, z/r, v} with v = -doppler * doppler_velocity_correction_factor (fp32);
//   .cpp:99-118   zero velocity: the n0-th smallest |v| (std::nth_element) against thresh_zero_velocity;
//   .cpp:172-250  solve3DFullRansac: ransac_iter_ hypotheses from N_ransac_points shuffled rows each, |y - H v| < inlier_thresh, the
//                 "more than 5 % outliers: regard them as inliers" rule, best inlier / best outlier list kept separately;
//   .cpp:252-303  solve3DFull: v = (H^T H).ldlt().solve(H^T y), C = e^T e (H^T H)^-1 / (rows - 3), sigma = sqrt(diag C) + offsets.
// The reference scores its hypotheses one after another (three of them at its defaults); here all K <= 1024 are scored in one pass
// over the rows (k_ego_score).  Every launch is sized by the scan (n) and K, the kernels read the number of valid rows m from the
// record the earlier kernels left on the device, so the host waits once, for that record.
//
// Deviations, all stated in include/apdgicp_hip.h:
//   - r: ((x x + y y) + z z) in fp64; Eigen's order for Vector3d::norm() is not pinned (it matters only within 1 ulp of min_dist / max_dist);
//   - the reference draws its samples from std::random_device + std::shuffle, which nobody can reproduce: the caller supplies the
//     words and ego_sample() turns them into S distinct rows;
//   - the 3x3 solve is an UNPIVOTED LDL^T in the order written in ego_ldlt3 (Eigen's ldlt() pivots on the largest diagonal entry);
//   - H^T H, H^T y and e^T e of the final fit are fixed-tree block sums (Eigen: its own order): same bits on every run;
//   - n0 is clamped to m - 1 (the reference reads one past the end with allowed_outlier_percentage = 0).
// No floating-point atomics; integer counts use atomicAdd.  Every pointer of this file is a KERNEL ARGUMENT (there is no descriptor table:
// one scan, one record), which the compiler already knows to be global memory, so no G() cast is needed or used here (apd_kernels.hpp:43-45).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/apd_atan2f.h"
#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int EGO_BLK = 1024;      // compaction / one-block kernels: 16 waves
constexpr int EGO_TILE = 256;      // rows of a scoring block, one per lane
constexpr int EGO_GROUP = 64;      // hypotheses of a scoring block
constexpr int EGO_MAX_K = 1024;
constexpr int EGO_MAX_S = 8;
enum { EGO_MODE_NONE = 0, EGO_MODE_ZERO = 1, EGO_MODE_RANSAC = 2, EGO_MODE_ALL = 3 };

struct EgoParams {  // the device's view of apdgicp_ego_velocity_params
  double min_dist, max_dist, az_thr, el_thr, inlier_thresh;
  double sigma_zero[3], sigma_offset[3], max_sigma[3];
  double allowed_outlier_percentage;
  float min_db, factor, thresh_zero;
  int use_ransac, S, K;
};

struct EgoRecord {  // head: apdgicp_ego_velocity_result, byte for byte
  double v[3], sigma[3];
  int success, zero_velocity, sigma_in_bounds, m, n_inlier, n_outlier, best_in, best_out, K, reserved;
  // behind it: what the kernels hand each other
  int mode, merged, n_front, n0;
  unsigned sel_bits;
  int pad_;
};

__device__ __forceinline__ void ego_block_counts(bool a, int* wsum, int* bsum) {  // EGO_BLK threads; bsum[blockIdx.x] = lanes with a
  const int tid = threadIdx.x;
  const int c = __popcll(__ballot(a));
  if ((tid & 63) == 0) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < EGO_BLK / 64; w++) s += wsum[w];
    bsum[blockIdx.x] = s;
  }
  __syncthreads();
}
__device__ __forceinline__ int ego_block_slot(bool a, int* wsum, int block_base) {  // slot of this lane among the lanes with a, in order
  const int tid = threadIdx.x, wave = tid >> 6;
  const unsigned long long m = __ballot(a);
  if ((tid & 63) == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = block_base;
  for (int w = 0; w < wave; w++) before += wsum[w];
  __syncthreads();
  return mbcnt_add(m, before);
}

// ---- stage 1 (.cpp:75-91): one lane per point.  rows_all[i] = {x/r, y/r, z/r, v}, valid[i], bsum[block] = valid points of the block
__global__ __launch_bounds__(EGO_BLK) void k_ego_features(const float* pts, int n, int stride /* floats */, int ioff, int doff, EgoParams P, double4* rows_all,
                                                          unsigned char* valid, int* bsum) {
  __shared__ int wsum[EGO_BLK / 64];
  __shared__ float s_atan[APD_ATAN_TAB_ROWS * APD_ATAN_TAB_STRIDE];  // apd_atan2f's interval table, like the linearize kernels
  atan_tab_to_lds(s_atan, (int)threadIdx.x);
  __syncthreads();
  const int i = blockIdx.x * EGO_BLK + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const auto p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2], intensity = p[ioff], doppler = p[doff];
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    const double r = sqrt((xd * xd + yd * yd) + zd * zd);
    const double az = (double)apd_atan2f_tab(y, x, s_atan);
    const double el = (double)apd_atan2f_tab(sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y))), z, s_atan) - M_PI_2;
    ok = r > P.min_dist && r < P.max_dist && intensity > P.min_db && fabs(az) < P.az_thr && fabs(el) < P.el_thr;  // NaN fails
    const float v = __fmul_rn(-doppler, P.factor);
    rows_all[i] = make_double4(xd / r, yd / r, zd / r, (double)v);
    valid[i] = ok ? 1 : 0;
  }
  ego_block_counts(ok, wsum, bsum);
}
// ... and their in-order compaction (bsum: scanned by k_scan_bsum, which also left m in the record)
__global__ __launch_bounds__(EGO_BLK) void k_ego_compact(const double4* rows_all, const unsigned char* valid, int n, const int* bsum, double4* rows, int* src) {
  __shared__ int wsum[EGO_BLK / 64];
  const int i = blockIdx.x * EGO_BLK + threadIdx.x;
  const bool ok = i < n && valid[i];
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (ok) rows[slot] = rows_all[i], src[slot] = i;
}

// ---- stage 2 (.cpp:99-118): ONE block.  The n0-th smallest |v| by a four-pass 8-bit radix selection on the fp32 bits of |v| (non-negative
// floats order like their bits; a NaN sorts last), histograms in LDS.  Decides what the later kernels do (rec->mode).
__global__ __launch_bounds__(EGO_BLK) void k_ego_zero_velocity(const double4* rows, EgoParams P, EgoRecord* rec) {
  __shared__ int hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_rank;
  const int tid = threadIdx.x, m = rec->m;
  if (m <= 2) {  // "To small valid_targets": no estimate (.cpp:99, 145)
    if (tid == 0) rec->mode = EGO_MODE_NONE, rec->K = P.K;
    return;
  }
  // size_t n = v_dopplers.size() * (1.0 - allowed_outlier_percentage); clamped to m - 1 (the reference: v_dopplers[m] at 0 %)
  int n0 = (int)min((double)(m - 1), max(0.0, (double)m * (1.0 - P.allowed_outlier_percentage)));
  if (tid == 0) s_prefix = 0u, s_rank = n0;
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix, himask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
    for (int i = tid; i < m; i += EGO_BLK) {
      const unsigned b = __float_as_uint(fabsf((float)rows[i].w));
      if ((b & himask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int rank = s_rank, d = 0;
      while (d < 255 && rank >= hist[d]) rank -= hist[d], d++;
      s_rank = rank, s_prefix = prefix | ((unsigned)d << shift);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned bits = s_prefix;
    const bool zero = __uint_as_float(bits) < P.thresh_zero;
    rec->sel_bits = bits, rec->n0 = n0, rec->zero_velocity = zero ? 1 : 0, rec->K = P.K;
    rec->mode = zero ? EGO_MODE_ZERO : !P.use_ransac ? EGO_MODE_ALL : (P.K > 0 && m >= P.S) ? EGO_MODE_RANSAC : EGO_MODE_NONE;
  }
}

// The stand-in for std::shuffle (.cpp:194-198): sample i of a hypothesis is c = w[i] % (m - i) among the rows not picked yet -- for every
// earlier pick t, in ascending order, t <= c moves c up by one -- so the S rows are distinct and every S-subset in every order can be drawn.
__device__ __forceinline__ void ego_sample(const unsigned* w, int S, int m, int* samp) {
  int sorted[EGO_MAX_S];
  for (int i = 0; i < S; i++) {
    int c = (int)(w[i] % (unsigned)(m - i));
    for (int t = 0; t < i; t++)
      if (sorted[t] <= c) c++;
    samp[i] = c;
    int at = i;
    while (at > 0 && sorted[at - 1] > c) sorted[at] = sorted[at - 1], at--;
    sorted[at] = c;
  }
}
// Unpivoted LDL^T of the symmetric 3x3 A = {a00, a01, a02, a11, a12, a22} and the solve of A v = b, in exactly this order:
__device__ __forceinline__ void ego_ldlt3(const double* A, const double* b, double* v) {
  const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
  const double d0 = a00, l10 = a01 / d0, l20 = a02 / d0;
  const double d1 = a11 - l10 * a01;
  const double t = a12 - l20 * a01;
  const double l21 = t / d1;
  const double d2 = (a22 - l20 * a02) - l21 * t;
  const double z0 = b[0], z1 = b[1] - l10 * z0, z2 = (b[2] - l20 * z0) - l21 * z1;
  const double w0 = z0 / d0, w1 = z1 / d1, w2 = z2 / d2;
  v[2] = w2;
  v[1] = w1 - l21 * v[2];
  v[0] = (w0 - l10 * v[1]) - l20 * v[2];
}

// ---- stage 3 (.cpp:190-199): one lane per hypothesis.  H^T H (6 sums) and H^T y (3 sums) over the S rows one after the other in sample order
__global__ __launch_bounds__(64) void k_ego_hypotheses(const double4* rows, const unsigned* words, EgoParams P, const EgoRecord* rec, double* vk, int* samples) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (rec->mode != EGO_MODE_RANSAC || k >= P.K) return;
  int samp[EGO_MAX_S];
  ego_sample(words + (size_t)k * P.S, P.S, rec->m, samp);
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, v[3];
  for (int i = 0; i < P.S; i++) {
    const double4 h = rows[samp[i]];
    samples[(size_t)k * P.S + i] = samp[i];
    A[0] += h.x * h.x, A[1] += h.x * h.y, A[2] += h.x * h.z, A[3] += h.y * h.y, A[4] += h.y * h.z, A[5] += h.z * h.z;
    b[0] += h.x * h.w, b[1] += h.y * h.w, b[2] += h.z * h.w;
  }
  ego_ldlt3(A, b, v);
  vk[3 * k] = v[0], vk[3 * k + 1] = v[1], vk[3 * k + 2] = v[2];
}

__device__ __forceinline__ bool ego_inlier(const double4& h, double v0, double v1, double v2, double thr) {
  return fabs(h.w - ((h.x * v0 + h.y * v1) + h.z * v2)) < thr;  // .cpp:203-209; a NaN is an outlier
}

// ---- stage 4 (.cpp:203-214), the hot pass: grid (row tiles of 256) x (groups of 64 hypotheses).  A lane holds its row in registers and walks
// the group's v_k out of LDS; per hypothesis ballot + popcount per wave, the four waves added in LDS, one integer atomicAdd per block.
__global__ __launch_bounds__(EGO_TILE) void k_ego_score(const double4* rows, const double* vk, EgoParams P, const EgoRecord* rec, int* n_in) {
  __shared__ double sv[3 * EGO_GROUP];
  __shared__ int wcnt[EGO_TILE / 64][EGO_GROUP];
  const int m = rec->m, tid = threadIdx.x, i = blockIdx.x * EGO_TILE + tid, k0 = blockIdx.y * EGO_GROUP;
  if (rec->mode != EGO_MODE_RANSAC || (int)blockIdx.x * EGO_TILE >= m) return;  // (block-uniform)
  const int kn = min(EGO_GROUP, P.K - k0);
  if (tid < 3 * kn) sv[tid] = vk[3 * k0 + tid];
  __syncthreads();
  const bool live = i < m;
  const double4 h = rows[live ? i : m - 1];
  for (int g = 0; g < kn; g++) {
    const bool in = live && ego_inlier(h, sv[3 * g], sv[3 * g + 1], sv[3 * g + 2], P.inlier_thresh);
    const int c = __popcll(__ballot(in));
    if ((tid & 63) == 0) wcnt[tid >> 6][g] = c;
  }
  __syncthreads();
  if (tid < kn) {
    const int c = (wcnt[0][tid] + wcnt[1][tid]) + (wcnt[2][tid] + wcnt[3][tid]);
    if (c) atomicAdd(&n_in[k0 + tid], c);
  }
}

// ---- stage 5 (.cpp:215-233): ONE block, lane k = hypothesis k.  The reference keeps the FIRST hypothesis with strictly more (effective)
// inliers, and separately the first with strictly more (effective) outliers: two arg-max reductions over integer keys.
__global__ __launch_bounds__(EGO_BLK) void k_ego_select(const int* n_in, EgoParams P, EgoRecord* rec) {
  __shared__ unsigned long long red[2][EGO_BLK / 64];
  const int tid = threadIdx.x, m = rec->m;
  if (rec->mode != EGO_MODE_RANSAC) return;
  unsigned long long ki = 0, ko = 0;
  if (tid < P.K) {
    const int in = n_in[tid], out = m - in;
    const bool merge = (double)((float)out / (float)m) > 0.05;  // float(outlier_idx.size()) / (inlier + outlier) > 0.05
    const int in_eff = merge ? m : in, out_eff = merge ? 0 : out;
    ki = ((unsigned long long)in_eff << 32) | (unsigned)(EGO_MAX_K - tid);
    ko = ((unsigned long long)out_eff << 32) | (unsigned)(EGO_MAX_K - tid);
  }
  for (int off = 32; off > 0; off >>= 1) ki = max(ki, __shfl_down(ki, off, 64)), ko = max(ko, __shfl_down(ko, off, 64));
  if ((tid & 63) == 0) red[0][tid >> 6] = ki, red[1][tid >> 6] = ko;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < EGO_BLK / 64; w++) ki = max(ki, red[0][w]), ko = max(ko, red[1][w]);
    const int bi = EGO_MAX_K - (int)(unsigned)ki, bo = EGO_MAX_K - (int)(unsigned)ko;
    const int in = n_in[bi];
    rec->best_in = (ki >> 32) ? bi : -1;
    rec->merged = (ki >> 32) && (double)((float)(m - in) / (float)m) > 0.05 ? 1 : 0;
    rec->best_out = (ko >> 32) ? bo : -1;
  }
}

// ---- the lists (.cpp:114-116, 133-140, 226-233).  Per row two flags: a = the row is in the front part of the inlier list (zero velocity:
// |v| < thresh; no RANSAC: every row; RANSAC: an inlier of best_in), b = the row is an outlier of best_out.  A row that is not `a` goes
// BEHIND the front part, in order, when best_in was merged.  Count, scan, scatter.
__device__ __forceinline__ void ego_flags(const double4* rows, const double* vk, const EgoParams& P, const EgoRecord* rec, int i, bool& a, bool& b) {
  a = b = false;
  if (i >= rec->m) return;
  const int mode = rec->mode;
  if (mode == EGO_MODE_ALL) a = true;
  if (mode == EGO_MODE_ZERO) a = fabsf((float)rows[i].w) < P.thresh_zero;
  if (mode == EGO_MODE_RANSAC) {
    const double4 h = rows[i];
    const int bi = rec->best_in, bo = rec->best_out;
    if (bi >= 0) a = ego_inlier(h, vk[3 * bi], vk[3 * bi + 1], vk[3 * bi + 2], P.inlier_thresh);
    if (bo >= 0) b = !ego_inlier(h, vk[3 * bo], vk[3 * bo + 1], vk[3 * bo + 2], P.inlier_thresh);
  }
}
__global__ __launch_bounds__(EGO_BLK) void k_ego_emit_count(const double4* rows, const double* vk, EgoParams P, const EgoRecord* rec, int* bsum_a, int* bsum_b) {
  __shared__ int wsum[EGO_BLK / 64];
  bool a, b;
  ego_flags(rows, vk, P, rec, blockIdx.x * EGO_BLK + threadIdx.x, a, b);
  ego_block_counts(a, wsum, bsum_a);
  ego_block_counts(b, wsum, bsum_b);
}
__global__ __launch_bounds__(SCAN_BLK) void k_ego_emit_scan(int* bsum_a, int* bsum_b, int nb, EgoRecord* rec) {  // ONE block: k_scan_bsum for both
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
  if (tid == 0) {
    const bool merged = rec->mode == EGO_MODE_RANSAC && rec->merged;
    rec->n_front = carry_a, rec->n_inlier = merged ? rec->m : carry_a, rec->n_outlier = carry_b;
  }
}
// writes the lists and, in the same pass, the clouds: {x, y, z, intensity}, doppler = -v (toRadarPointCloudType, .cpp:41-50), source index
__global__ __launch_bounds__(EGO_BLK) void k_ego_emit_scatter(const double4* rows, const int* src, const double* vk, EgoParams P, const EgoRecord* rec, const int* bsum_a,
                                                              const int* bsum_b, const float* pts, int stride, int ioff, int* in_row, float4* in_xyzi, float* in_dop,
                                                              int* in_src, int* out_row, float4* out_xyzi, float* out_dop, int* out_src) {
  __shared__ int wsum[EGO_BLK / 64];
  const int i = blockIdx.x * EGO_BLK + threadIdx.x, m = rec->m;
  bool a, b;
  ego_flags(rows, vk, P, rec, i, a, b);
  const int slot_a = ego_block_slot(a, wsum, bsum_a[blockIdx.x]);
  const int slot_b = ego_block_slot(b, wsum, bsum_b[blockIdx.x]);
  if (i >= m) return;
  const int s = src[i];
  const auto p = pts + (size_t)s * stride;
  const float4 q = make_float4(p[0], p[1], p[2], p[ioff]);
  const float dop = -(float)rows[i].w;
  const int at = a ? slot_a : (rec->mode == EGO_MODE_RANSAC && rec->merged) ? rec->n_front + (i - slot_a) : -1;
  if (at >= 0) in_row[at] = i, in_xyzi[at] = q, in_dop[at] = dop, in_src[at] = s;
  if (b) out_row[slot_b] = i, out_xyzi[slot_b] = q, out_dop[slot_b] = dop, out_src[slot_b] = s;
}

// fixed tree over the block: lane partials -> shuffles inside the wave -> the 16 wave sums pairwise; every lane gets the result
template <int N>
__device__ __forceinline__ void ego_block_sum(double (&s)[N], double (*red)[EGO_BLK / 64]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = 0; q < N; q++)
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off, 64);
  __syncthreads();
  if (lane == 0)
    for (int q = 0; q < N; q++) red[q][wave] = s[q];
  __syncthreads();
  for (int q = 0; q < N; q++) {
    double t[EGO_BLK / 64];
    for (int w = 0; w < EGO_BLK / 64; w++) t[w] = red[q][w];
    for (int span = 1; span < EGO_BLK / 64; span <<= 1)
      for (int w = 0; w < EGO_BLK / 64; w += 2 * span) t[w] += t[w + span];
    s[q] = t[0];
  }
}

// ---- stage 6 (.cpp:257-293, solve3DFull(..., true)) on the inlier rows in list order, ONE block; also writes the record of the other modes
__global__ __launch_bounds__(EGO_BLK) void k_ego_lsq(const double4* rows, const int* in_row, EgoParams P, EgoRecord* rec) {
  __shared__ double red[9][EGO_BLK / 64];
  const int tid = threadIdx.x, mode = rec->mode, n = rec->n_inlier;
  if (mode == EGO_MODE_NONE || mode == EGO_MODE_ZERO || n == 0) {
    if (tid == 0) {
      const bool zero = mode == EGO_MODE_ZERO;
      for (int q = 0; q < 3; q++) rec->v[q] = 0.0, rec->sigma[q] = zero ? P.sigma_zero[q] : 0.0;
      rec->success = zero ? 1 : 0, rec->sigma_in_bounds = zero ? 1 : 0;
    }
    return;
  }
  double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += EGO_BLK) {
    const double4 h = rows[in_row[i]];
    s[0] += h.x * h.x, s[1] += h.x * h.y, s[2] += h.x * h.z, s[3] += h.y * h.y, s[4] += h.y * h.z, s[5] += h.z * h.z;
    s[6] += h.x * h.w, s[7] += h.y * h.w, s[8] += h.z * h.w;
  }
  ego_block_sum<9>(s, red);
  double v[3];
  ego_ldlt3(s, s + 6, v);
  double e2[1] = {0.0};
  for (int i = tid; i < n; i += EGO_BLK) {
    const double4 h = rows[in_row[i]];
    const double e = ((h.x * v[0] + h.y * v[1]) + h.z * v[2]) - h.w;
    e2[0] += e * e;
  }
  ego_block_sum<1>(e2, red);
  if (tid == 0) {
    const double a00 = s[0], a01 = s[1], a02 = s[2], a11 = s[3], a12 = s[4], a22 = s[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;  // cofactors
    const double c11 = a00 * a22 - a02 * a02, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double dof = (double)(n - 3);
    double sig[3] = {(e2[0] * (c00 / det)) / dof, (e2[0] * (c11 / det)) / dof, (e2[0] * (c22 / det)) / dof};
    int ok = 0;
    if (sig[0] >= 0.0 && sig[1] >= 0.0 && sig[2] >= 0.0) {  // else: the reference leaves diag C in sigma_v_r (.cpp:282-284)
      for (int q = 0; q < 3; q++) sig[q] = sqrt(sig[q]) + P.sigma_offset[q];
      ok = sig[0] < P.max_sigma[0] && sig[1] < P.max_sigma[1] && sig[2] < P.max_sigma[2];
    }
    for (int q = 0; q < 3; q++) rec->v[q] = v[q], rec->sigma[q] = sig[q];
    rec->success = 1, rec->sigma_in_bounds = ok;  // the reference returns true on every path (.cpp:302)
  }
}

}  // namespace apd
