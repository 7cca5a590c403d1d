// FastGICPMultiPoints on the device (fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp, "MPI:n" below) as a mode of the registration handle.
// The semantics are the numbered list MP1 .. MP11 of include/apdgicp_hip.h; the kernels below follow it item by item:
//   k_mp_transform     MP2: q = T_f * p over the curve-sorted source, fp32, xf_row's two orders.  A non-finite source point gets the query of
//                      the first finite lane of its wave (it only has to keep the wave's query box finite: its row is emptied below)
//   (rows)             MP3: k_radius_count / k_radius_scan / k_scan_bsum / k_radius_fill / k_radius_sort_rows of apd_search.hpp as they are,
//                      with q as the query cloud and the source's own permutation as qperm
//   k_mp_mask          MP3: the count of a non-finite source point becomes 0 before the scan, so it owns no row
//   k_mp_total         the hits of all rows as one 64-bit word: what the host sizes the row buffer by
//   k_mp_point         MP4 / MP5: one lane per source point walks its sorted row: the weights, the fused mean and covariance in row order,
//                      then RCR, its inverse, l, J and the point's 21 + 6 + 1 sums and its count; block rows in wave order
//   (k_icp_sums)       the block rows added in block order from 0.0, one lane per sum (apd_icp.hpp's kernel: it is generic in the row width)
// Everything behind the rows is fp64, compiled without contraction: written order is evaluated order.  No floating-point atomics, no lane
// reads another lane's state outside the written reduction tree.  Every pointer and every loop bound is a kernel argument.  Long rows make
// the lanes of a wave diverge in k_mp_point; the sums stay in row order regardless (MP4), see docs/experiments.md.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_icp.hpp"
#include "apd_kernels.hpp"
#include "apd_search.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr int MP_BLK = IC_BLK;  // (icp_block_row's block)
constexpr int MP_R = 29;        // [0, 21): H, upper triangle row by row; [21, 27): g; [27]: cost; [28]: rows that took part
constexpr int MP_FUSED = 10;    // per source point: sum_w, mean_B[3], cov_B[6] (xx, xy, xz, yy, yz, zz)
static_assert(MP_BLK % SQ_BLK == 0, "a wave of k_mp_transform must be a block of the searching kernels");

enum { MP_NOT_CONVERGED = 0, MP_CONVERGED = 1, MP_TOO_FEW_ROWS = 2, MP_SINGULAR = 3 };

__device__ __forceinline__ bool mp_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// MP2.  T: row-major 3x4 [R | t], fp64, device
__global__ __launch_bounds__(MP_BLK) void k_mp_transform(const float4* src /* sorted */, int n, const double* T, int xf_linear, float4* q) {
  const int i = blockIdx.x * MP_BLK + threadIdx.x, lane = threadIdx.x & 63;
  const float4 p = src[min(i, n - 1)];
  const bool ok = i < n && mp_finite(p);
  float r0[4], r1[4], r2[4];
#pragma unroll
  for (int c = 0; c < 4; c++) r0[c] = (float)T[c], r1[c] = (float)T[4 + c], r2[c] = (float)T[8 + c];  // MPI:131-133: the fp32 pose
  float x = 0.f, y = 0.f, z = 0.f;
  if (ok) x = xf_row(r0, p.x, p.y, p.z, xf_linear), y = xf_row(r1, p.x, p.y, p.z, xf_linear), z = xf_row(r2, p.x, p.y, p.z, xf_linear);
  const bool fin = ok && isfinite(x) && isfinite(y) && isfinite(z);
  const unsigned long long m = __ballot(fin);
  const int first = m ? __ffsll((long long)m) - 1 : lane;
  const float fx = __shfl(x, first, 64), fy = __shfl(y, first, 64), fz = __shfl(z, first, 64);
  if (i < n) q[i] = fin ? make_float4(x, y, z, 1.f) : make_float4(m ? fx : 0.f, m ? fy : 0.f, m ? fz : 0.f, 0.f);  // .w = 0: no row
}

// MP3: cnt is in the caller's order (k_radius_count wrote cnt[perm[i]])
__global__ void k_mp_mask(const float4* q /* sorted */, const int* perm, int n, int* cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (q[i].w == 0.f) cnt[perm[i]] = 0;
}

// total[0] = sum of cnt[0 .. n) in 64 bits (one block)
__global__ __launch_bounds__(MP_BLK) void k_mp_total(const int* cnt, int n, long long* total) {
  __shared__ long long lds[MP_BLK];
  const int tid = threadIdx.x;
  long long s = 0;
  for (int i = tid; i < n; i += MP_BLK) s += cnt[i];
  lds[tid] = s;
  __syncthreads();
  for (int off = MP_BLK / 2; off > 0; off >>= 1) {
    if (tid < off) lds[tid] += lds[tid + off];
    __syncthreads();
  }
  if (tid == 0) total[0] = lds[0];
}

struct MpCloud {
  const float4* pts;   // source: curve-sorted; target: the caller's order
  const double* cov;   // curve-sorted, six planes of n
  const int* idx;      // source: sorted position -> the caller's index; target: the caller's index -> sorted position
  int n;
  int pad_;
};

// MP4 / MP5 for sorted source position i.  Returns false for an empty row (nothing of v is written).
__device__ __forceinline__ bool mp_point(const MpCloud& S, const MpCloud& Tg, const unsigned long long* row, int len, const Rigid& T, double r, int i, double* fused,
                                         double (&v)[MP_R]) {
  double sw = 0.0, mx = 0.0, my = 0.0, mz = 0.0, cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  for (int e = 0; e < len; e++) {  // MPI:183-192, in row order
    const unsigned long long key = row[e];
    const int j = (int)(unsigned)key;
    if ((unsigned)j >= (unsigned)Tg.n) continue;  // (a key carries an index of the target as set: never taken)
    const float d2 = __uint_as_float((unsigned)(key >> 32));
    const double w = fmax(1e-3, fmin(1.0, 1.0 - (double)sqrtf(d2) / r));
    const float4 t = Tg.pts[j];
    const int s = Tg.idx[j];
    sw += w;
    mx += w * (double)t.x, my += w * (double)t.y, mz += w * (double)t.z;
    cxx += w * Tg.cov[s], cxy += w * Tg.cov[Tg.n + s], cxz += w * Tg.cov[2 * Tg.n + s];
    cyy += w * Tg.cov[3 * Tg.n + s], cyz += w * Tg.cov[4 * Tg.n + s], czz += w * Tg.cov[5 * Tg.n + s];
  }
  if (len <= 0) {
#pragma unroll
    for (int q = 0; q < MP_FUSED; q++) fused[q] = 0.0;
    return false;
  }
  const double bx = mx / sw, by = my / sw, bz = mz / sw;  // MPI:194-195
  const Sym3 cb{cxx / sw, cxy / sw, cxz / sw, cyy / sw, cyz / sw, czz / sw};
  fused[0] = sw, fused[1] = bx, fused[2] = by, fused[3] = bz;
  fused[4] = cb.xx, fused[5] = cb.xy, fused[6] = cb.xz, fused[7] = cb.yy, fused[8] = cb.yz, fused[9] = cb.zz;
  const float4 p = S.pts[i];
  const double ax = (double)p.x, ay = (double)p.y, az = (double)p.z;
  const double tx = ((T.m[0] * ax + T.m[1] * ay) + T.m[2] * az) + T.m[3];  // MPI:197
  const double ty = ((T.m[4] * ax + T.m[5] * ay) + T.m[6] * az) + T.m[7];
  const double tz = ((T.m[8] * ax + T.m[9] * ay) + T.m[10] * az) + T.m[11];
  const double dx = bx - tx, dy = by - ty, dz = bz - tz;  // MPI:198
  const Sym3 ca{S.cov[i], S.cov[S.n + i], S.cov[2 * S.n + i], S.cov[3 * S.n + i], S.cov[4 * S.n + i], S.cov[5 * S.n + i]};
  const Sym3 M = sym3_inverse(sym3_add(cb, sym3_rotate(T, ca)));  // MPI:199-202
  const double l[3] = {(M.xx * dx + M.xy * dy) + M.xz * dz, (M.xy * dx + M.yy * dy) + M.yz * dz, (M.xz * dx + M.yz * dy) + M.zz * dz};  // MPI:203
  const double Mr[3][3] = {{M.xx, M.xy, M.xz}, {M.xy, M.yy, M.yz}, {M.xz, M.yz, M.zz}};
  double J[3][6];  // MPI:205-209: M * [skew(Ta) | -I]
#pragma unroll
  for (int a = 0; a < 3; a++) {
    J[a][0] = Mr[a][1] * tz - Mr[a][2] * ty;
    J[a][1] = Mr[a][2] * tx - Mr[a][0] * tz;
    J[a][2] = Mr[a][0] * ty - Mr[a][1] * tx;
    J[a][3] = -Mr[a][0], J[a][4] = -Mr[a][1], J[a][5] = -Mr[a][2];
  }
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) v[o++] = (J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b];
#pragma unroll
  for (int a = 0; a < 6; a++) v[21 + a] = (J[0][a] * l[0] + J[1][a] * l[1]) + J[2][a] * l[2];
  v[27] = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];
  v[28] = 1.0;
  return true;
}

// fused: [n][MP_FUSED] in the caller's order; part: [blocks][MP_R]
__global__ __launch_bounds__(MP_BLK) void k_mp_point(MpCloud S, MpCloud Tg, const unsigned long long* rows, const int* cnt, const int* pos, const int* bsum, const double* T12,
                                                     double r, double* fused, double* part) {
  __shared__ double lds[(MP_BLK / 64) * MP_R];
  const int tid = threadIdx.x, i = blockIdx.x * MP_BLK + tid;
  double v[MP_R];
#pragma unroll
  for (int q = 0; q < MP_R; q++) v[q] = 0.0;
  if (i < S.n) {
    Rigid T;
#pragma unroll
    for (int q = 0; q < 12; q++) T.m[q] = T12[q];
    const int o = S.idx[i], len = cnt[o];
    const unsigned long long* row = rows + ((size_t)pos[o] + (size_t)bsum[o / SCAN_BLK]);
    double w[MP_R];
    if (mp_point(S, Tg, row, len, T, r, i, fused + (size_t)o * MP_FUSED, w)) {
#pragma unroll
      for (int q = 0; q < MP_R; q++) v[q] = w[q];
    }
  }
  icp_block_row<MP_R>(v, lds, tid, part + (size_t)blockIdx.x * MP_R);
}

}  // namespace apd
