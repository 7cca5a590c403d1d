// Scan ingest and deskew on the device: the two ends of PreprocessingNodelet::cloud_callback
// (radar_graph_slam/apps/preprocessing_nodelet.cpp) that the other stage files leave out:
//   :667-683  the head: per point of the message the power gate (channels[2] > power_threshold), the `== NAN` tests (never true)
//             and the `== INFINITY` tests, then {x, y, z, intensity = power, doppler = channels[0]} pushed in order;
//   :497-506  the same packing without a gate (the hugin callback);
//   :477-480  an optional fixed transform of the packed points;
//   :951-972  deskewing: a = -(float)angular_velocity; per point i of n the quaternion (w = 1, delta_t / 2.0 * a) with
//             delta_t = scan_period * (double)i / n, its Quaternionf::inverse() applied to the point by Quaternion::_transformVector;
//   :796-810  the transform into the base-link frame behind it.
// I1 .. I7 of include/apdgicp_hip.h state every expression.  What belongs to Eigen and is not pinned by the reference tree:
//   - squaredNorm() of the four quaternion coefficients: (x x + y y) + (z z + w w), or ((x x + y y) + z z) + w w with
//     APDGICP_FLAG_XF_LINEAR_CHAIN (the same switch as xf_row: the halving / the left-to-right reduction of the two Eigen generations);
//   - T * p per row: xf_row (apd_kernels.hpp).
// Every operation is rounded on its own: the library is built with -ffp-contract=off (build.py), so no FMA forms; the *_rn spellings
// below only say so where the order matters.  Divisions are IEEE divisions (hipcc's default for fp32 as well).  The compaction is the
// one of the ego-velocity stage (ego_block_counts / ego_block_slot around k_scan_bsum): input order is kept.  No atomics in any of these.
// Behind them, at the end of the file: the polar message of cloud_callback_scan (:331-340, PI1 .. PI5) and the distance histogram that ends
// all three callbacks (:451-461, H1 .. H4; 32-bit integer atomics, so its bytes do not depend on the order of the blocks either).
// Every pointer of this file is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_ego.hpp"
#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int ING_BLK = EGO_BLK;               // compaction kernels: 16 waves, one point per lane (ego_block_counts / ego_block_slot)
constexpr int ING_DESKEW_BLK = 256;
constexpr long long ING_MAX_N = 1ll << 24;     // the largest cloud: int indices, at most 2^14 block sums for k_scan_bsum

struct IngestLanes {  // I1: three byte-strided lanes of one message
  const char* xyz;
  const char* intensity;
  const char* doppler;
  long long xyz_stride, intensity_stride, doppler_stride;  // bytes, multiples of 4
};
struct IngestXf {  // rows 0..2 of a 4x4, row-major: what xf_row reads
  float m[12];
  int on, linear;
};

// I2: kept iff power > threshold (a NaN power fails) and no coordinate equals +infinity (NaN and -infinity are kept)
__device__ __forceinline__ bool ingest_keep(const IngestLanes& L, int i, int n, int gate, float thr) {
  if (i >= n) return false;
  if (!gate) return true;
  const float* p = (const float*)(L.xyz + (size_t)i * L.xyz_stride);
  const float power = *(const float*)(L.intensity + (size_t)i * L.intensity_stride);
  const float inf = __builtin_inff();
  return power > thr && !(p[0] == inf || p[1] == inf || p[2] == inf);
}

__global__ __launch_bounds__(ING_BLK) void k_ing_count(IngestLanes L, int n, int gate, float thr, int* bsum) {
  __shared__ int wsum[ING_BLK / 64];
  const int i = blockIdx.x * ING_BLK + threadIdx.x;
  ego_block_counts(ingest_keep(L, i, n, gate, thr), wsum, bsum);
}
// ... their in-order compaction (bsum: scanned by k_scan_bsum, which also left n_out on the device), I3 and I4 in the same pass
__global__ __launch_bounds__(ING_BLK) void k_ing_scatter(IngestLanes L, int n, int gate, float thr, IngestXf X, const int* bsum, float4* rows, int* index) {
  __shared__ int wsum[ING_BLK / 64];
  const int i = blockIdx.x * ING_BLK + threadIdx.x;
  const bool keep = ingest_keep(L, i, n, gate, thr);
  const int slot = ego_block_slot(keep, wsum, bsum[blockIdx.x]);
  if (!keep) return;
  const float* p = (const float*)(L.xyz + (size_t)i * L.xyz_stride);
  float x = p[0], y = p[1], z = p[2];
  if (X.on) {
    const float tx = xf_row(X.m + 0, x, y, z, X.linear), ty = xf_row(X.m + 4, x, y, z, X.linear), tz = xf_row(X.m + 8, x, y, z, X.linear);
    x = tx, y = ty, z = tz;
  }
  const float power = *(const float*)(L.intensity + (size_t)i * L.intensity_stride);
  const float doppler = *(const float*)(L.doppler + (size_t)i * L.doppler_stride);
  rows[2 * (size_t)slot] = make_float4(x, y, z, power);
  rows[2 * (size_t)slot + 1] = make_float4(doppler, 0.f, 0.f, 0.f);
  index[slot] = i;
}

// (a x b)_k with every product and the difference rounded on their own
__device__ __forceinline__ float ing_cross(float a1, float b2, float a2, float b1) { return __fsub_rn(__fmul_rn(a1, b2), __fmul_rn(a2, b1)); }

struct DeskewParams {
  double scan_period;
  float a[3];   // -(float)angular velocity
  int on;       // 0: ang_vel == NULL, the cloud passes through
};

// I5 - I7: one lane per point; deskew, then the frame transform, {x, y, z, intensity} out
__global__ __launch_bounds__(ING_DESKEW_BLK) void k_ing_deskew(const char* pts, int n, long long stride /* bytes */, int ioff /* floats, < 0: none */, DeskewParams D,
                                                               IngestXf X, float4* out) {
  const int i = blockIdx.x * ING_DESKEW_BLK + threadIdx.x;
  if (i >= n) return;
  const float* p = (const float*)(pts + (size_t)i * stride);
  float vx = p[0], vy = p[1], vz = p[2];
  const float intensity = ioff >= 0 ? p[ioff] : 0.f;
  if (D.on) {
    const double dt = __ddiv_rn(__dmul_rn(D.scan_period, (double)i), (double)n);
    const double h = __ddiv_rn(dt, 2.0);
    const float qx = (float)__dmul_rn(h, (double)D.a[0]), qy = (float)__dmul_rn(h, (double)D.a[1]), qz = (float)__dmul_rn(h, (double)D.a[2]), qw = 1.0f;
    // Quaternionf::inverse(): conjugate / squaredNorm, the zero quaternion when the norm is not > 0 (a NaN rate)
    const float xx = __fmul_rn(qx, qx), yy = __fmul_rn(qy, qy), zz = __fmul_rn(qz, qz), ww = __fmul_rn(qw, qw);
    const float n2 = X.linear ? __fadd_rn(__fadd_rn(__fadd_rn(xx, yy), zz), ww) : __fadd_rn(__fadd_rn(xx, yy), __fadd_rn(zz, ww));
    float cx = 0.f, cy = 0.f, cz = 0.f, cw = 0.f;
    if (n2 > 0.f) cx = __fdiv_rn(-qx, n2), cy = __fdiv_rn(-qy, n2), cz = __fdiv_rn(-qz, n2), cw = __fdiv_rn(qw, n2);
    // Quaternion::_transformVector: uv = c x v; uv += uv; v + cw * uv + c x uv
    float ux = ing_cross(cy, vz, cz, vy), uy = ing_cross(cz, vx, cx, vz), uz = ing_cross(cx, vy, cy, vx);
    ux = __fadd_rn(ux, ux), uy = __fadd_rn(uy, uy), uz = __fadd_rn(uz, uz);
    const float ox = __fadd_rn(__fadd_rn(vx, __fmul_rn(cw, ux)), ing_cross(cy, uz, cz, uy));
    const float oy = __fadd_rn(__fadd_rn(vy, __fmul_rn(cw, uy)), ing_cross(cz, ux, cx, uz));
    const float oz = __fadd_rn(__fadd_rn(vz, __fmul_rn(cw, uz)), ing_cross(cx, uy, cy, ux));
    vx = ox, vy = oy, vz = oz;
  }
  if (X.on) {
    const float tx = xf_row(X.m + 0, vx, vy, vz, X.linear), ty = xf_row(X.m + 4, vx, vy, vz, X.linear), tz = xf_row(X.m + 8, vx, vy, vz, X.linear);
    vx = tx, vy = ty, vz = tz;
  }
  out[i] = make_float4(vx, vy, vz, intensity);
}

// ------------------------------------------------------------------ the polar message: cloud_callback_scan, :331-340 (PI1 .. PI5)
struct PolarLanes {  // PI1: five byte-strided lanes of one RadarScanExtended
  const char *range, *azimuth, *elevation, *snr, *velocity;
  long long range_stride, azimuth_stride, elevation_stride, snr_stride, velocity_stride;  // bytes, multiples of 4
};

// PI3: sine and cosine of an fp32 angle, each the fp64 value rounded once to fp32: sincos_pi for |a| <= pi, the device library's
// fp64 sincos for everything else (a NaN fails the comparison and goes there too)
__device__ __forceinline__ void ing_sincosf(float a, float* s, float* c) {
  const double x = (double)a;
  double sd, cd;
  if (fabs(x) <= 3.14159265358979323846) sincos_pi(x, &sd, &cd);
  else sincos(x, &sd, &cd);
  *s = (float)sd, *c = (float)cd;
}

// one target per lane: {(r ce) ca, (r ce) sa, (-r) se, snr, velocity, 0, 0, 0} and index = i; no gate (PI2)
__global__ __launch_bounds__(ING_BLK) void k_ing_polar(PolarLanes L, int n, float4* rows, int* index) {
  const int i = blockIdx.x * ING_BLK + threadIdx.x;
  if (i >= n) return;
  const float r = *(const float*)(L.range + (size_t)i * L.range_stride);
  const float az = *(const float*)(L.azimuth + (size_t)i * L.azimuth_stride);
  const float el = *(const float*)(L.elevation + (size_t)i * L.elevation_stride);
  const float snr = *(const float*)(L.snr + (size_t)i * L.snr_stride);
  const float vel = *(const float*)(L.velocity + (size_t)i * L.velocity_stride);
  float se, ce, sa, ca;
  ing_sincosf(el, &se, &ce);
  ing_sincosf(az, &sa, &ca);
  const float rc = __fmul_rn(r, ce);
  rows[2 * (size_t)i] = make_float4(__fmul_rn(rc, ca), __fmul_rn(rc, sa), __fmul_rn(-r, se), snr);
  rows[2 * (size_t)i + 1] = make_float4(vel, 0.f, 0.f, 0.f);
  index[i] = i;
}

// ------------------------------------------------------------------ the distance histogram: :451-461, :618-628, :818-828 (H1 .. H4)
constexpr int ING_HIST_BINS = 100;
constexpr int ING_HIST_WORDS = ING_HIST_BINS + 1;  // counts: 100 bins and the ticket of k_ing_hist; sum: 100 bins and the frame counter

// the frame's counts and the ticket back to zero
__global__ __launch_bounds__(128) void k_ing_hist_zero(int* counts) {
  if (threadIdx.x < ING_HIST_WORDS) counts[threadIdx.x] = 0;
}
// H1 per point into the block's LDS bins, the block's non-empty bins into counts; the block that draws the last ticket adds the finished
// counts to the running sum and counts the frame.  Integer atomics only: the result does not depend on the order of the blocks.
__global__ __launch_bounds__(ING_BLK) void k_ing_hist(const char* pts, int n, long long stride /* bytes */, int* counts, long long* sum) {
  __shared__ int bins[ING_HIST_BINS];
  __shared__ int last;
  if (threadIdx.x < ING_HIST_BINS) bins[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * ING_BLK + threadIdx.x;
  if (i < n) {
    const float* p = (const float*)(pts + (size_t)i * stride);
    const float x = p[0], y = p[1], z = p[2];
    const float d = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));  // the range gate's norm (k_flt_gate)
    if (d < (float)ING_HIST_BINS) atomicAdd(&bins[(int)floorf(d)], 1);  // d >= 0 or NaN: finite and floorf(d) < 100
  }
  __syncthreads();
  if (threadIdx.x < ING_HIST_BINS && bins[threadIdx.x]) atomicAdd(counts + threadIdx.x, bins[threadIdx.x]);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd((unsigned*)(counts + ING_HIST_BINS), 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (threadIdx.x < ING_HIST_BINS) sum[threadIdx.x] += atomicAdd(counts + threadIdx.x, 0);  // (read where the other blocks' atomics landed)
  if (threadIdx.x == 0) sum[ING_HIST_BINS] += 1;
}

}  // namespace apd
