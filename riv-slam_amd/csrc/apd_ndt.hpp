// NDT registration on the device: fast_gicp::NDTCuda (ndt/impl/ndt_cuda_impl.hpp, cuda/ndt_cuda.cu, ndt_compute_derivatives.cu, gaussian_voxelmap.cu,
// covariance_regularization.cu), point-to-distribution (P2D) and distribution-to-distribution (D2D), as a mode of the registration handle.  The
// semantics are the numbered list N1 .. N9 of include/apdgicp_hip.h; the kernels below follow it item by item:
//   k_vg_keys          N1: the voxel key of every point in the caller's order, the first offending point (apd_vgicp.hpp)
//   (sort)             N1: the map cloud's stable LSD radix sort (apd_map.hpp) over (key, point index) pairs; equal keys keep the caller's order
//   k_ndt_voxels       N2 / N3: one lane per voxel walks its run of the sorted list: the fp64 sums S1 and S2 in the caller's order, mean, the raw
//                      covariance (lower triangle of the reference's expression), and in the same lane the MIN_EIG regularisation with the
//                      absolute floor 1e-3.  A single voxel that holds every point is one lane adding n points: legal and merely slow.
//   k_ndt_linearize<D> N5 / N6: one row per lane -- a source voxel in voxel order (D2D) or a source point in the caller's order (P2D) -- 1 / 7 / 27
//                      binary searches over the sorted voxel keys, per hit with count > 6 the matrix M, the residual, the Cauchy weight and
//                      the 21 + 6 + 1 (+ count) sums
//   k_ndt_error<D>     N7: the same cost at the trial pose over the stored voxel indices; M is recomputed from the rotation of the last
//                      linearize pose by the same device function
//   k_vg_reduce        the per-block partials added in block order by one lane per sum (apd_vgicp.hpp)
// The per-row bodies of the two kernels are the device functions nd_linearize_row / nd_error_row: the batch mode's kernel (apd_ndt_batch.hpp)
// calls the same ones.
// Everything here is fp64 except the stored points, compiled without contraction (sym3_eig / sym3_from_eig of apd_math.hpp allow it inside
// themselves and are compared by tolerance): written order is evaluated order.  No floating-point atomics.  Every pointer is a kernel argument.
//
// The compiler's report for gfx950 (-Rpass-analysis=kernel-resource-usage), blocks of 256:
//   k_ndt_linearize<true>   (D2D)  136 VGPRs, no scratch, 3 waves per SIMD, LDS 928 bytes (4 x 29 doubles)
//   k_ndt_linearize<false>  (P2D)  122 VGPRs, no scratch, 4 waves per SIMD, LDS 928 bytes
//   k_ndt_error<true>               74 VGPRs, no scratch, 6 waves per SIMD, LDS 64 bytes
//   k_ndt_error<false>              56 VGPRs, no scratch, 8 waves per SIMD, LDS 64 bytes
//   k_ndt_voxels                    68 VGPRs, no scratch, 7 waves per SIMD, LDS 64 bytes
// Not tuned further: a D2D grid is a handful of blocks (one to two thousand source voxels for an 8k scan) and is bound by its launches.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_kernels.hpp"
#include "apd_map.hpp"
#include "apd_vgicp.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr double ND_MIN_EIG = 1e-3;     // N3: the absolute floor of covariance_regularization.cu:73-87
constexpr int ND_MIN_POINTS = 6;        // N6: a target voxel with count <= 6 contributes nothing (ndt_compute_derivatives.cu:61,132)

// N2 / N3: the head of every run of equal keys is a voxel (k_map_heads counts them, k_scan_bsum scans the block counts)
__global__ __launch_bounds__(MAP_BLK) void k_ndt_voxels(const unsigned long long* keys, const int* sidx, int n, const int* bsum, const float4* opts,
                                                        unsigned long long* vkeys, int* vcount, double* vmean, double* vraw, double* vcov, int cap) {
  __shared__ int wsum[MAP_BLK / 64];
  const long long i = (long long)blockIdx.x * MAP_BLK + threadIdx.x;
  const bool ok = map_head(keys, i, n);
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (!ok || slot < 0 || slot >= cap) return;
  const unsigned long long k = keys[i];
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  int cnt = 0;
  for (long long j = i; j < n && keys[j] == k; j++) {
    const int o = sidx[j];
    if ((unsigned)o >= (unsigned)n) continue;
    const float4 p = opts[o];
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    sx += x, sy += y, sz += z;
    sxx += x * x, sxy += x * y, sxz += x * z, syy += y * y, syz += y * z, szz += z * z;
    cnt++;
  }
  const double fn = (double)cnt;
  const double mx = sx / fn, my = sy / fn, mz = sz / fn;
  // c_rc = (S2_rc - mean_r S1_c) / n for r >= c: the triangle SelfAdjointEigenSolver reads
  Sym3 raw;
  raw.xx = (sxx - mx * sx) / fn;
  raw.xy = (sxy - my * sx) / fn;
  raw.xz = (sxz - mz * sx) / fn;
  raw.yy = (syy - my * sy) / fn;
  raw.yz = (syz - mz * sy) / fn;
  raw.zz = (szz - mz * sz) / fn;
  double w[3], u[9];
  sym3_eig(raw, w, u);
  const Sym3 reg = sym3_from_eig(u, fmax(w[0], ND_MIN_EIG), fmax(w[1], ND_MIN_EIG), fmax(w[2], ND_MIN_EIG));
  vkeys[slot] = k, vcount[slot] = cnt;
  double* m = vmean + 3 * (size_t)slot;
  m[0] = mx, m[1] = my, m[2] = mz;
  double* r = vraw + 6 * (size_t)slot;
  r[0] = raw.xx, r[1] = raw.xy, r[2] = raw.xz, r[3] = raw.yy, r[4] = raw.yz, r[5] = raw.zz;
  double* c = vcov + 6 * (size_t)slot;
  c[0] = reg.xx, c[1] = reg.xy, c[2] = reg.xz, c[3] = reg.yy, c[4] = reg.yz, c[5] = reg.zz;
}

__device__ __forceinline__ Sym3 nd_load_cov(const VgMap& m, int v) {
  const double* c = m.cov + 6 * (size_t)v;
  return Sym3{c[0], c[1], c[2], c[3], c[4], c[5]};
}

// N5: the position of row i -- the mean of source voxel i (D2D) or source point i (P2D)
template <bool D2D>
__device__ __forceinline__ void nd_row(const float4* opts, const VgMap& smap, int i, double& x, double& y, double& z) {
  if (D2D) {
    const double* m = smap.mean + 3 * (size_t)i;
    x = m[0], y = m[1], z = m[2];
  } else {
    const float4 p = opts[i];
    x = (double)p.x, y = (double)p.y, z = (double)p.z;
  }
}

// N6: M = (C_B + R_lin C_A R_lin^T)^-1 (D2D, RCA = R_lin C_A R_lin^T) or C_B^-1 (P2D): the one function both kernels call (N7)
template <bool D2D>
__device__ __forceinline__ Sym3 nd_mahalanobis(const VgMap& m, int v, const Sym3& RCA) {
  const Sym3 cb = nd_load_cov(m, v);
  return sym3_inverse(D2D ? sym3_add(cb, RCA) : cb);
}

// one term of N6 at q = (vx, vy, vz) against target voxel v: cost and count onto acc[27], acc[28], H and b onto acc[0 .. 27) when wanted
template <bool D2D>
__device__ __forceinline__ void nd_term(const VgMap& map, int v, const Sym3& RCA, double res2, double vx, double vy, double vz, int want_Hb, double* acc) {
  const Sym3 Mi = nd_mahalanobis<D2D>(map, v, RCA);
  const double* mu = map.mean + 3 * (size_t)v;
  const double ex = mu[0] - vx, ey = mu[1] - vy, ez = mu[2] - vz;
  const double w = res2 / (res2 + ((ex * ex + ey * ey) + ez * ez));  // Cauchy, k = resolution
  const double mex = (Mi.xx * ex + Mi.xy * ey) + Mi.xz * ez;
  const double mey = (Mi.xy * ex + Mi.yy * ey) + Mi.yz * ez;
  const double mez = (Mi.xz * ex + Mi.yz * ey) + Mi.zz * ez;
  acc[27] += w * ((ex * mex + ey * mey) + ez * mez);
  acc[28] += 1.0;
  if (!want_Hb) return;
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

// N5 / N6, one row: the searches of row i at pose T, its indices into corr (i x noff), its terms onto acc[0 .. 29).  The one function every
// linearize kernel calls (k_ndt_linearize below, k_ndb_points of apd_ndt_batch.hpp): N12 holds by construction.
template <bool D2D>
__device__ __forceinline__ void nd_linearize_row(const float4* opts, const VgMap& smap, const VgMap& map, const Rigid& T, double res, int mode, int noff, int want_Hb,
                                                 int* corr, int i, double* acc) {
  double x, y, z;
  nd_row<D2D>(opts, smap, i, x, y, z);
  const double vx = vg_xf_row(T, 0, x, y, z), vy = vg_xf_row(T, 1, x, y, z), vz = vg_xf_row(T, 2, x, y, z);
  const double cx = vg_coord(vx, res), cy = vg_coord(vy, res), cz = vg_coord(vz, res);
  // a coordinate this far out cannot come back into range with an offset of one; also catches a q that is not finite
  const bool inr = fabs(cx) <= (double)VG_LIM && fabs(cy) <= (double)VG_LIM && fabs(cz) <= (double)VG_LIM;
  const int ix = inr ? (int)cx : 0, iy = inr ? (int)cy : 0, iz = inr ? (int)cz : 0;
  const double res2 = res * res;
  Sym3 RCA{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool have_rca = false;
  for (int k = 0; k < noff; k++) {
    int ox, oy, oz;
    vg_offset(mode, k, ox, oy, oz);
    const int ax = ix + ox, ay = iy + oy, az = iz + oz;
    int v = -1;
    if (inr && abs(ax) < VG_LIM && abs(ay) < VG_LIM && abs(az) < VG_LIM) v = vg_find(map, vg_pack(ax, ay, az));  // the range test comes first
    corr[(size_t)i * noff + k] = v;
    if (v < 0 || map.count[v] <= ND_MIN_POINTS) continue;
    if (D2D && !have_rca) {
      RCA = sym3_rotate(T, nd_load_cov(smap, i));
      have_rca = true;
    }
    nd_term<D2D>(map, v, RCA, res2, vx, vy, vz, want_Hb, acc);
  }
}

// N7, one row: the cost of row i at the trial pose T over its stored indices, M from the rotation of T0 (the pose of the last linearize);
// cost onto acc[27], count onto acc[28]
template <bool D2D>
__device__ __forceinline__ void nd_error_row(const float4* opts, const VgMap& smap, const VgMap& map, const Rigid& T, const Rigid& T0, double res, int noff,
                                             const int* corr, int i, double* acc) {
  double x, y, z;
  nd_row<D2D>(opts, smap, i, x, y, z);
  const double vx = vg_xf_row(T, 0, x, y, z), vy = vg_xf_row(T, 1, x, y, z), vz = vg_xf_row(T, 2, x, y, z);
  const double res2 = res * res;
  Sym3 RCA{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool have_rca = false;
  for (int k = 0; k < noff; k++) {
    const int v = corr[(size_t)i * noff + k];
    if (v < 0 || v >= map.nv || map.count[v] <= ND_MIN_POINTS) continue;
    if (D2D && !have_rca) {
      RCA = sym3_rotate(T0, nd_load_cov(smap, i));
      have_rca = true;
    }
    nd_term<D2D>(map, v, RCA, res2, vx, vy, vz, 0, acc);
  }
}

// the cost and the count of a block's error rows into slots 27 and 28 of the block's row, like a linearize
__device__ __forceinline__ void nd_error_block_sums(const double* acc, double* red, double* part, int tid) {
  double two[2] = {acc[27], acc[28]};
  block_reduce<2, VG_BLK>(two, red, tid);
  if (tid < 2) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < VG_BLK / 64; w++) s += red[w * 2 + tid];
    part[(size_t)blockIdx.x * VG_RED + 27 + tid] = s;
  }
}

// N5 / N6.  T12[0..12): the pose, row-major 3x4.  nrows = smap.nv (D2D) or the number of source points (P2D).  corr: nrows x noff voxel indices
// (-1: miss), written here.
template <bool D2D>
__global__ __launch_bounds__(VG_BLK) void k_ndt_linearize(const float4* opts, VgMap smap, int nrows, VgMap map, const double* T12, double res, int mode, int noff,
                                                          int want_Hb, int* corr, double* part) {
  __shared__ double red[(VG_BLK / 64) * VG_SUMS];
  const int tid = threadIdx.x, i = blockIdx.x * VG_BLK + tid;
  Rigid T;
#pragma unroll
  for (int q = 0; q < 12; q++) T.m[q] = T12[q];
  double acc[VG_SUMS];
#pragma unroll
  for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
  if (i < nrows) nd_linearize_row<D2D>(opts, smap, map, T, res, mode, noff, want_Hb, corr, i, acc);
  vg_block_sums<VG_SUMS>(acc, red, part, tid);
}

// N7: T12 = the trial pose, T12 + 12 = the pose of the last linearize (its rotation is R_lin)
template <bool D2D>
__global__ __launch_bounds__(VG_BLK) void k_ndt_error(const float4* opts, VgMap smap, int nrows, VgMap map, const double* T12, double res, int noff, const int* corr,
                                                      double* part) {
  __shared__ double red[(VG_BLK / 64) * 2];
  const int tid = threadIdx.x, i = blockIdx.x * VG_BLK + tid;
  Rigid T, T0;
#pragma unroll
  for (int q = 0; q < 12; q++) T.m[q] = T12[q], T0.m[q] = T12[12 + q];
  double acc[VG_SUMS];
#pragma unroll
  for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
  if (i < nrows) nd_error_row<D2D>(opts, smap, map, T, T0, res, noff, corr, i, acc);
  nd_error_block_sums(acc, red, part, tid);
}

}  // namespace apd
