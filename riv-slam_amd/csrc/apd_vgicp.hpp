// Voxelized GICP on the device: fast_gicp::FastVGICP (gicp/impl/fast_vgicp_impl.hpp, gicp/fast_vgicp_voxel.hpp), the FAST_VGICP branch of
// select_registration_method() (registrations.cpp:62-70), as a mode of the registration handle.  The semantics are the numbered list
// V1 .. V7 of include/apdgicp_hip.h; the kernels below follow it item by item:
//   k_vg_keys        V1 / V2: the voxel key of every target point in the caller's order, the first offending point
//   (sort)           V3: the map cloud's stable LSD radix sort (apd_map.hpp) over (key, point index) pairs -- k_map_rs_hist / k_map_scan_tiles /
//                    k_scan_bsum and k_map_rs_scatter_pairs, the same scatter with the index as payload.  Equal keys keep the caller's order.
//   k_vg_voxels      V3: one lane per voxel walks its run of the sorted list: fp64 sums in the caller's order, then / count.  A single
//                    voxel that holds every point is one lane adding n points: legal and merely slow.
//   k_vg_linearize   V4 / V5: one source point per lane in the caller's order, 1 / 7 / 27 binary searches over the sorted voxel keys, per
//                    hit RCR = C_voxel + R C_A R^T (no APD term), its inverse, the residual and the 21 + 6 + 1 (+ count) sums
//   k_vg_error       V6: the same cost over the voxel indices and the pose of the last linearize (M is RECOMPUTED from the stored pose with
//                    the same device function, not stored: 4 bytes per (point, offset) instead of 52)
//   k_vg_reduce      the per-block partials added in block order by one lane per sum
// Everything here is fp64 except the stored points, compiled without contraction: written order is evaluated order.  No floating-point
// atomics.  Every pointer is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_kernels.hpp"
#include "apd_map.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr int VG_BLK = 256;             // linearize / error: 4 waves, one source point per lane.  k_vg_linearize keeps 29 fp64 accumulators per lane:
                                        // 138 registers, no scratch, 3 waves per SIMD (the compiler's report); its LDS is 4 x 29 doubles.  Not tuned further.
constexpr int VG_SUMS = 29;             // 21 H (upper triangle, row-major) + 6 b + cost + correspondences
constexpr int VG_RED = 32;              // doubles per block partial
constexpr int VG_LIM = 1 << 20;         // V2: |c| < 2^20 per axis
constexpr int VG_MAX_OFFSETS = 27;

struct VgMap {                          // the voxel map of the target, voxels in ascending key order
  const unsigned long long* keys;       // nv
  const int* count;                     // nv
  const double* mean;                   // nv x 3
  const double* cov;                    // nv x 6: xx, xy, xz, yy, yz, zz
  int nv;
};

// V1: c = floor(x / res - 0.5), a true division
__device__ __forceinline__ double vg_coord(double x, double res) { return floor(__dsub_rn(__ddiv_rn(x, res), 0.5)); }
// V2: the three biased 21-bit coordinates; the caller has checked the range
__device__ __forceinline__ unsigned long long vg_pack(int cx, int cy, int cz) {
  return ((unsigned long long)(unsigned)(cx + VG_LIM) << 42) | ((unsigned long long)(unsigned)(cy + VG_LIM) << 21) | (unsigned long long)(unsigned)(cz + VG_LIM);
}
__device__ __forceinline__ bool vg_in_range(double c) { return fabs(c) < (double)VG_LIM; }  // (false for NaN and infinities)

__global__ void k_vg_keys(const float4* opts, int n, double res, unsigned long long* keys, int* idx, int* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = opts[i];
  const double cx = vg_coord((double)p.x, res), cy = vg_coord((double)p.y, res), cz = vg_coord((double)p.z, res);
  const bool ok = vg_in_range(cx) && vg_in_range(cy) && vg_in_range(cz);
  keys[i] = ok ? vg_pack((int)cx, (int)cy, (int)cz) : 0ull;
  idx[i] = i;
  if (!ok) atomicMin(bad, i);
}

// original index -> position on the curve (the engine keeps covariances in curve order)
__global__ void k_vg_inverse_perm(const int* perm, int n, int* inv) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int o = perm[s];
  if ((unsigned)o < (unsigned)n) inv[o] = s;
}

// V3: the head of every run of equal keys is a voxel (k_map_heads counts them, k_scan_bsum scans the block counts)
__global__ __launch_bounds__(MAP_BLK) void k_vg_voxels(const unsigned long long* keys, const int* sidx, int n, const int* bsum, const float4* opts, const double* cov,
                                                       const int* inv, unsigned long long* vkeys, int* vcount, double* vmean, double* vcov, int cap) {
  __shared__ int wsum[MAP_BLK / 64];
  const long long i = (long long)blockIdx.x * MAP_BLK + threadIdx.x;
  const bool ok = map_head(keys, i, n);
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (!ok || slot < 0 || slot >= cap) return;
  const unsigned long long k = keys[i];
  double mx = 0.0, my = 0.0, mz = 0.0, cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  int cnt = 0;
  for (long long j = i; j < n && keys[j] == k; j++) {
    const int o = sidx[j];
    if ((unsigned)o >= (unsigned)n) continue;
    const float4 p = opts[o];
    const int s = inv[o];
    if ((unsigned)s >= (unsigned)n) continue;
    mx += (double)p.x, my += (double)p.y, mz += (double)p.z;
    cxx += cov[s], cxy += cov[(size_t)n + s], cxz += cov[2 * (size_t)n + s];
    cyy += cov[3 * (size_t)n + s], cyz += cov[4 * (size_t)n + s], czz += cov[5 * (size_t)n + s];
    cnt++;
  }
  const double fn = (double)cnt;
  vkeys[slot] = k, vcount[slot] = cnt;
  double* m = vmean + 3 * (size_t)slot;
  m[0] = mx / fn, m[1] = my / fn, m[2] = mz / fn;
  double* c = vcov + 6 * (size_t)slot;
  c[0] = cxx / fn, c[1] = cxy / fn, c[2] = cxz / fn, c[3] = cyy / fn, c[4] = cyz / fn, c[5] = czz / fn;
}

// the index of `key` among the sorted voxel keys, -1: no such voxel
__device__ __forceinline__ int vg_find(const VgMap& m, unsigned long long key) {
  int lo = 0, hi = m.nv;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (m.keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < m.nv && m.keys[lo] == key ? lo : -1;
}

// V5: the offsets in the order of fast_vgicp_voxel.hpp:17-43.  mode 0: DIRECT1, 1: DIRECT7, 2: DIRECT27 ((i - 1, j - 1, k - 1), k fastest)
__device__ __forceinline__ void vg_offset(int mode, int k, int& ox, int& oy, int& oz) {
  ox = oy = oz = 0;
  if (mode == 1) {
    if (k == 1) ox = 1;
    else if (k == 2) ox = -1;
    else if (k == 3) oy = 1;
    else if (k == 4) oy = -1;
    else if (k == 5) oz = 1;
    else if (k == 6) oz = -1;
  } else if (mode == 2) {
    ox = k / 9 - 1, oy = (k / 3) % 3 - 1, oz = k % 3 - 1;
  }
}

// V4: q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r
__device__ __forceinline__ double vg_xf_row(const Rigid& T, int r, double x, double y, double z) {
  return ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3];
}

__device__ __forceinline__ Sym3 vg_load_cov(const double* cov, int n, int s) {
  return Sym3{cov[s], cov[(size_t)n + s], cov[2 * (size_t)n + s], cov[3 * (size_t)n + s], cov[4 * (size_t)n + s], cov[5 * (size_t)n + s]};
}

// M = (C_voxel + R C_A R^T)^-1 with `RCA` = R C_A R^T of the linearize pose: the one function both kernels call (V6)
__device__ __forceinline__ Sym3 vg_mahalanobis(const VgMap& m, int v, const Sym3& RCA) {
  const double* c = m.cov + 6 * (size_t)v;
  return sym3_inverse(sym3_add(Sym3{c[0], c[1], c[2], c[3], c[4], c[5]}, RCA));
}

// the sums of one block -> part[block][VG_RED]: wave sums (DPP tree), the four waves added in wave order
template <int R>
__device__ __forceinline__ void vg_block_sums(double* acc, double* red /* [VG_BLK / 64][R] */, double* part, int tid) {
  block_reduce<R, VG_BLK>(acc, red, tid);
  if (tid < R) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < VG_BLK / 64; w++) s += red[w * R + tid];
    part[(size_t)blockIdx.x * VG_RED + tid] = s;
  }
}

// Where the offsets of a linearize come from.  REACH: the largest |component| an offset can have.
struct VgModeOffsets {  // V5: DIRECT1 / 7 / 27, computed from k
  static constexpr int REACH = 1;
  int mode;
  __device__ __forceinline__ void get(int k, int& ox, int& oy, int& oz) const { vg_offset(mode, k, ox, oy, oz); }
};
struct VgTableOffsets {  // VC6 (apd_vgicp_cuda.hpp): a table of 3 ints per offset in device memory, read at a wave-uniform index
  static constexpr int REACH = 4;
  const int* tab;
  __device__ __forceinline__ void get(int k, int& ox, int& oy, int& oz) const { ox = tab[3 * k], oy = tab[3 * k + 1], oz = tab[3 * k + 2]; }
};

// V4 / V5: source point i of a linearize at pose T -- its noff voxel indices to corr, its terms onto the 29 sums `acc`.  The one per-point body of
// k_vg_linearize, of the batch tick (apd_vgicp_batch.hpp) and of k_vc_linearize (apd_vgicp_cuda.hpp): the same operations in the same written
// order wherever it is called from.
template <class Offsets>
__device__ __forceinline__ void vg_linearize_point_of(const float4* opts, const double* cov_src, const int* inv_src, int n, const VgMap& map, const Rigid& T, double res,
                                                      const Offsets& offs, int noff, int want_Hb, int* corr, int i, double* acc) {
  const float4 p = opts[i];
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double vx = vg_xf_row(T, 0, x, y, z), vy = vg_xf_row(T, 1, x, y, z), vz = vg_xf_row(T, 2, x, y, z);
  const double cx = vg_coord(vx, res), cy = vg_coord(vy, res), cz = vg_coord(vz, res);
  // A coordinate c with |c| > 2^20 + REACH - 1 cannot come back into range (|c + o| < 2^20) with any offset, |o| <= REACH: such a point
  // misses everything, and so does a q that is not finite.  Inside that bound c + o is exact in an int, and the test per offset below is V2's.
  // (REACH = 1: the bound is 2^20 itself.)
  const bool inr = fabs(cx) <= (double)(VG_LIM + Offsets::REACH - 1) && fabs(cy) <= (double)(VG_LIM + Offsets::REACH - 1) && fabs(cz) <= (double)(VG_LIM + Offsets::REACH - 1);
  const int ix = inr ? (int)cx : 0, iy = inr ? (int)cy : 0, iz = inr ? (int)cz : 0;
  Sym3 RCA{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool have_rca = false;
  for (int k = 0; k < noff; k++) {
    int ox, oy, oz;
    offs.get(k, ox, oy, oz);
    const int ax = ix + ox, ay = iy + oy, az = iz + oz;
    int v = -1;
    if (inr && abs(ax) < VG_LIM && abs(ay) < VG_LIM && abs(az) < VG_LIM) v = vg_find(map, vg_pack(ax, ay, az));  // V2: the range test comes first
    corr[(size_t)i * noff + k] = v;
    if (v < 0) continue;
    if (!have_rca) {
      const int s = min(max(inv_src[i], 0), n - 1);
      RCA = sym3_rotate(T, vg_load_cov(cov_src, n, s));
      have_rca = true;
    }
    const Sym3 Mi = vg_mahalanobis(map, v, RCA);
    const double* mu = map.mean + 3 * (size_t)v;
    const double w = sqrt((double)map.count[v]);
    const double ex = mu[0] - vx, ey = mu[1] - vy, ez = mu[2] - vz;
    const double mex = (Mi.xx * ex + Mi.xy * ey) + Mi.xz * ez;
    const double mey = (Mi.xy * ex + Mi.yy * ey) + Mi.yz * ez;
    const double mez = (Mi.xz * ex + Mi.yz * ey) + Mi.zz * ez;
    acc[27] += w * ((ex * mex + ey * mey) + ez * mez);
    acc[28] += 1.0;
    if (!want_Hb) continue;
    // J = [skew(q) | -I]; MA = M skew(q)
    const double m0x = Mi.xy * vz - Mi.xz * vy, m0y = Mi.yy * vz - Mi.yz * vy, m0z = Mi.yz * vz - Mi.zz * vy;
    const double m1x = Mi.xz * vx - Mi.xx * vz, m1y = Mi.yz * vx - Mi.xy * vz, m1z = Mi.zz * vx - Mi.xz * vz;
    const double m2x = Mi.xx * vy - Mi.xy * vx, m2y = Mi.xy * vy - Mi.yy * vx, m2z = Mi.xz * vy - Mi.yz * vx;
    acc[0] += w * (vz * m0y - vy * m0z);
    acc[1] += w * (vz * m1y - vy * m1z);
    acc[2] += w * (vz * m2y - vy * m2z);
    acc[3] += w * -m0x;
    acc[4] += w * -m0y;
    acc[5] += w * -m0z;
    acc[6] += w * (vx * m1z - vz * m1x);
    acc[7] += w * (vx * m2z - vz * m2x);
    acc[8] += w * -m1x;
    acc[9] += w * -m1y;
    acc[10] += w * -m1z;
    acc[11] += w * (vy * m2x - vx * m2y);
    acc[12] += w * -m2x;
    acc[13] += w * -m2y;
    acc[14] += w * -m2z;
    acc[15] += w * Mi.xx;
    acc[16] += w * Mi.xy;
    acc[17] += w * Mi.xz;
    acc[18] += w * Mi.yy;
    acc[19] += w * Mi.yz;
    acc[20] += w * Mi.zz;
    acc[21] += w * (vz * mey - vy * mez);
    acc[22] += w * (vx * mez - vz * mex);
    acc[23] += w * (vy * mex - vx * mey);
    acc[24] += w * -mex;
    acc[25] += w * -mey;
    acc[26] += w * -mez;
  }
}
__device__ __forceinline__ void vg_linearize_point(const float4* opts, const double* cov_src, const int* inv_src, int n, const VgMap& map, const Rigid& T, double res,
                                                   int mode, int noff, int want_Hb, int* corr, int i, double* acc) {
  vg_linearize_point_of(opts, cov_src, inv_src, n, map, T, res, VgModeOffsets{mode}, noff, want_Hb, corr, i, acc);
}

// T2[0..12): the pose, row-major 3x4.  corr: n x noff voxel indices (-1: miss), written here.
__global__ __launch_bounds__(VG_BLK) void k_vg_linearize(const float4* opts, const double* cov_src, const int* inv_src, int n, VgMap map, const double* T12, double res,
                                                         int mode, int noff, int want_Hb, int* corr, double* part) {
  __shared__ double red[(VG_BLK / 64) * VG_SUMS];
  const int tid = threadIdx.x, i = blockIdx.x * VG_BLK + tid;
  Rigid T;
#pragma unroll
  for (int q = 0; q < 12; q++) T.m[q] = T12[q];
  double acc[VG_SUMS];
#pragma unroll
  for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
  if (i < n) {
    vg_linearize_point(opts, cov_src, inv_src, n, map, T, res, mode, noff, want_Hb, corr, i, acc);
  }
  vg_block_sums<VG_SUMS>(acc, red, part, tid);
}

// V6: source point i at the trial pose T over the voxel indices and the pose T0 of the last linearize -- cost and count onto acc[0], acc[1]
__device__ __forceinline__ void vg_error_point(const float4* opts, const double* cov_src, const int* inv_src, int n, const VgMap& map, const Rigid& T, const Rigid& T0,
                                               int noff, const int* corr, int i, double* acc) {
  const float4 p = opts[i];
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double vx = vg_xf_row(T, 0, x, y, z), vy = vg_xf_row(T, 1, x, y, z), vz = vg_xf_row(T, 2, x, y, z);
  Sym3 RCA{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool have_rca = false;
  for (int k = 0; k < noff; k++) {
    const int v = corr[(size_t)i * noff + k];
    if (v < 0 || v >= map.nv) continue;
    if (!have_rca) {
      RCA = sym3_rotate(T0, vg_load_cov(cov_src, n, min(max(inv_src[i], 0), n - 1)));
      have_rca = true;
    }
    const Sym3 Mi = vg_mahalanobis(map, v, RCA);
    const double* mu = map.mean + 3 * (size_t)v;
    const double w = sqrt((double)map.count[v]);
    const double ex = mu[0] - vx, ey = mu[1] - vy, ez = mu[2] - vz;
    const double mex = (Mi.xx * ex + Mi.xy * ey) + Mi.xz * ez;
    const double mey = (Mi.xy * ex + Mi.yy * ey) + Mi.yz * ez;
    const double mez = (Mi.xz * ex + Mi.yz * ey) + Mi.zz * ez;
    acc[0] += w * ((ex * mex + ey * mey) + ez * mez);
    acc[1] += 1.0;
  }
}

// V6: T12 = the trial pose, T12 + 12 = the pose of the last linearize
__global__ __launch_bounds__(VG_BLK) void k_vg_error(const float4* opts, const double* cov_src, const int* inv_src, int n, VgMap map, const double* T12, int noff,
                                                     const int* corr, double* part) {
  __shared__ double red[(VG_BLK / 64) * 2];
  const int tid = threadIdx.x, i = blockIdx.x * VG_BLK + tid;
  Rigid T, T0;
#pragma unroll
  for (int q = 0; q < 12; q++) T.m[q] = T12[q], T0.m[q] = T12[12 + q];
  double acc[2] = {0.0, 0.0};
  if (i < n) {
    vg_error_point(opts, cov_src, inv_src, n, map, T, T0, noff, corr, i, acc);
  }
  // (the cost goes to slot 27 and the count to slot 28 of the block's row, like k_vg_linearize)
  block_reduce<2, VG_BLK>(acc, red, tid);
  if (tid < 2) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < VG_BLK / 64; w++) s += red[w * 2 + tid];
    part[(size_t)blockIdx.x * VG_RED + 27 + tid] = s;
  }
}

// the block rows added in block order -> out[0..36) H column-major, [36..42) b, [42] cost, [43] correspondences
__global__ __launch_bounds__(64) void k_vg_reduce(const double* part, int nblk, int first, double* out) {
  __shared__ double v[VG_SUMS];
  const int tid = threadIdx.x;
  if (tid < VG_SUMS) {
    double s = 0.0;
    if (tid >= first)
      for (int b = 0; b < nblk; b++) s += part[(size_t)b * VG_RED + tid];
    v[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int q = 0;
    for (int r = 0; r < 6; r++)
      for (int c = r; c < 6; c++, q++) out[r + 6 * c] = v[q], out[c + 6 * r] = v[q];
    for (int r = 0; r < 6; r++) out[36 + r] = v[21 + r];
    out[42] = v[27], out[43] = v[28];
  }
}

}  // namespace apd
