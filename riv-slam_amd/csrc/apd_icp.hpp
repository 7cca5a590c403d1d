// Point-to-point ICP on the device (pcl::IterativeClosestPoint, PCL 1.10 as published: registration/impl/icp.hpp, correspondence_estimation.hpp,
// default_convergence_criteria.hpp, transformation_estimation_svd.hpp over Eigen's umeyama) as a mode of the registration handle.  The semantics
// are the numbered list IC1 .. IC10 of include/apdgicp_hip.h; the kernels below follow it item by item:
//   k_icp_init         IC1: W0 = guess * source (or the source itself) in the source's curve order, .w = 1 for a finite point, else {0, 0, 0, 0}
//   k_icp_transform    IC1: W = T_k * W in place, fp32, xf_row's two orders; T_k is read from the device record, it never visits the host
//   (forward search)   IC2: the engine's own exact search (launch_nn + the per-point pass that settles the index) with W in place of the sorted
//                      source at the identity pose: 1 * x + 0 * y + 0 * z + 0 is x in either order, so the search sees W itself
//   k_boxes            IC3: the chunk and group boxes of W, recomputed every iteration (apd_sort.hpp's kernel, min / max of the fp32 coordinates)
//   k_icp_recip<P>     IC3: one lane per forward match (i, j): is any other point of W nearer to target[j] than W[i], or as near with a lower
//                      index in the caller's order?  P = true walks W's group and chunk boxes (lb_point_box: a bound in the distance's own fp32
//                      order, strict comparison, so ties survive); P = false is the LDS-tiled brute force, the cross-check
//                      (APDGICP_ICP_RECIP_MODE=brute).  Both evaluate sqdist1(target, W), the forward search's expression, so the reciprocal
//                      distance of a surviving pair IS the forward one and passes the gate with it.
//   k_icp_pairs        IC2 / IC3 / IC5: gate, the match per point, and per block the eight first-pass sums (sum d2, sum p, sum q, count)
//   k_icp_sums         the block rows of either pass added in block order from 0.0, one lane per sum
//   k_icp_cross        IC5: second pass, the nine sums of (q - qm)(p - pm)^T per block
//   k_icp_step         IC4 .. IC7 in one lane: the nine sums, the 3x3 SVD (one-sided Jacobi), R, t, the fp32 T_k, the product, the criteria;
//                      writes one record
// Reductions: a wave's values through the DPP tree of apd_kernels.hpp (wave_sum_to_lane63), waves through LDS in wave order, blocks in block
// order.  No floating-point atomics.  Compiled without contraction: written order is evaluated order.  Every pointer is a kernel argument.
// Launches per iteration: 2 (search) + 3 (pairs, sums, cross) + 1 (step) + 1 (transform), + 3 with reciprocal correspondences; none depends on n.
// Every kernel body is a device function (icp_init_point .. icp_step_wave): the batch handle's kernels (apd_icp_batch.hpp, IC11 .. IC16) call the
// same ones with the pair in the grid, which is what makes a batch pair's bytes the single handle's.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_kernels.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr int IC_BLK = 256;
constexpr int IC_R1 = 8;  // first pass: sum d2, sum p (3), sum q (3), count
constexpr int IC_R2 = 9;  // second pass: sum (q - qm)_r (p - pm)_c, row-major
constexpr int IC_TILE = 1024;

enum { IC_NOT_CONVERGED = 0, IC_ITERATIONS = 1, IC_TRANSFORM = 2, IC_ABS_MSE = 3, IC_REL_MSE = 4, IC_NO_CORRESPONDENCES = 5 };

struct IcpConsts {
  double thr2;       // max_correspondence_distance^2, the product in fp64 (IC2)
  double trans_eps;  // transformation_epsilon, compared with the SQUARED translation (IC7)
  double rot_thr;    // rotation_epsilon if > 0, else 1 - transformation_epsilon
  double mse_abs, mse_rel;
  int max_iterations, min_corr, max_similar, accumulate;  // accumulate = 0: the probe (IC2 .. IC5 only)
};

// the one record of an iteration: written by k_icp_step, copied to pinned memory, read by the host behind its one wait
struct IcpRecord {
  float T_k[16];      // column-major, this iteration's step (identity when none was estimated)
  float final_T[16];  // column-major, the product so far (IC6)
  double sums[16];    // [0] sum d2, [1..3] sum p, [4..6] sum q, [7..15] sum (q - qm)(p - pm)^T row-major (q: target, p: W)
  double mse, prev_mse;
  long long n_corr;
  int iterations, similar, state, converged, stop, estimated;
};

// IC1 for one point: W0[i] = T * src[i] (null T: the source itself), .w = 1 for a finite point, else {0, 0, 0, 0}
__device__ __forceinline__ void icp_init_point(const float4* src /* sorted */, const float* T16 /* column-major, device; null: W0 = source */, int xf_linear, float4* W, int i) {
  const float4 p = src[i];
  const bool ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  float x = p.x, y = p.y, z = p.z;
  if (T16 && ok) {
    const float r0[4] = {T16[0], T16[4], T16[8], T16[12]}, r1[4] = {T16[1], T16[5], T16[9], T16[13]}, r2[4] = {T16[2], T16[6], T16[10], T16[14]};
    x = xf_row(r0, p.x, p.y, p.z, xf_linear), y = xf_row(r1, p.x, p.y, p.z, xf_linear), z = xf_row(r2, p.x, p.y, p.z, xf_linear);
  }
  W[i] = ok ? make_float4(x, y, z, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void k_icp_init(const float4* src /* sorted */, int n, const float* T16 /* column-major, device; null: W0 = source */, int xf_linear, float4* W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  icp_init_point(src, T16, xf_linear, W, i);
}

// IC1 for one point: W[i] = T_k * W[i] in place
__device__ __forceinline__ void icp_transform_point(float4* W, const float* T /* column-major, device */, int xf_linear, int i) {
  const float4 p = W[i];
  if (p.w == 0.f) return;
  const float r0[4] = {T[0], T[4], T[8], T[12]}, r1[4] = {T[1], T[5], T[9], T[13]}, r2[4] = {T[2], T[6], T[10], T[14]};
  W[i] = make_float4(xf_row(r0, p.x, p.y, p.z, xf_linear), xf_row(r1, p.x, p.y, p.z, xf_linear), xf_row(r2, p.x, p.y, p.z, xf_linear), 1.f);
}

__global__ void k_icp_transform(float4* W, int n, const IcpRecord* rec, int xf_linear) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  icp_transform_point(W, rec->T_k, xf_linear, i);
}

// forward match of sorted source position i as the engine's search left it: target index (sorted) or -1, after validity and the gate
__device__ __forceinline__ int icp_forward(const float4 w, const float4 nn, float d, double thr2) {
  const int j = __float_as_int(nn.w);
  return (w.w != 0.f && j >= 0 && !((double)d > thr2)) ? j : -1;  // IC2: rejected iff (double)d2 > thr2, equality kept
}

// beaten[i] = 1: some point of W other than i is the nearest point of W to i's forward match (IC3)
// (the body of block bx of k_icp_recip: taken by whole blocks)
template <bool PRUNED>
__device__ __forceinline__ void icp_recip_block(const float4* W, int n, const int* perm, const Box* cbox, const Box* gbox, const float4* nnpt, const float* sqd, double thr2,
                                                unsigned char* beaten, int bx) {
  const int tid = threadIdx.x, i = bx * IC_BLK + tid;
  const bool in = i < n;
  const float4 w = in ? W[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 q = in ? nnpt[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
  const float r = in ? sqd[i] : 0.f;
  bool active = in && icp_forward(w, q, r, thr2) >= 0;
  const int oi = in ? perm[i] : 0;
  bool lost = false;
  if constexpr (PRUNED) {
    const int ngr = (n + kGroupPts - 1) / kGroupPts, nch = (n + kChunk - 1) / kChunk;
    for (int g = 0; g < ngr; g++) {
      if (!__ballot(active && !lost)) break;
      const Box gb = gbox[g];
      if (!__ballot(active && !lost && !(lb_point_box(gb, q.x, q.y, q.z) > r))) continue;
      const int c1 = min((g + 1) * kGroupChunks, nch);
      for (int c = g * kGroupChunks; c < c1; c++) {
        const Box cb = cbox[c];
        if (!__ballot(active && !lost && !(lb_point_box(cb, q.x, q.y, q.z) > r))) continue;
        const int k1 = min((c + 1) * kChunk, n);
        for (int k = c * kChunk; k < k1; k++) {  // (every lane looks: a lane whose bound excluded the chunk finds nothing there)
          const float4 t = W[k];
          const float d = sqdist1(q.x, q.y, q.z, t.x, t.y, t.z);
          if (t.w != 0.f && k != i && (d < r || (d == r && perm[k] < oi))) lost = true;
        }
      }
    }
  } else {
    __shared__ float4 tile[IC_TILE];
    for (int k0 = 0; k0 < n; k0 += IC_TILE) {
      __syncthreads();
      for (int e = tid; e < IC_TILE; e += IC_BLK) {
        float4 t = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));  // .w: the caller's index, -1: not a point of W
        if (k0 + e < n) {
          t = W[k0 + e];
          t.w = __int_as_float(t.w != 0.f ? perm[k0 + e] : -1);
        }
        tile[e] = t;
      }
      __syncthreads();
      const int m = min(IC_TILE, n - k0);
      if (active && !lost)
        for (int e = 0; e < m; e++) {
          const float4 t = tile[e];
          const float d = sqdist1(q.x, q.y, q.z, t.x, t.y, t.z);
          const int ok = __float_as_int(t.w);
          if (ok >= 0 && ok != oi && (d < r || (d == r && ok < oi))) lost = true;
        }
    }
  }
  if (in) beaten[i] = lost ? 1 : 0;
}

template <bool PRUNED>
__global__ __launch_bounds__(IC_BLK) void k_icp_recip(const float4* W, int n, const int* perm, const Box* cbox, const Box* gbox, const float4* nnpt, const float* sqd,
                                                      double thr2, unsigned char* beaten) {
  icp_recip_block<PRUNED>(W, n, perm, cbox, gbox, nnpt, sqd, thr2, beaten, (int)blockIdx.x);
}

// wave -> LDS -> the block's row: R sums of this block in wave order
template <int R>
__device__ __forceinline__ void icp_block_row(double (&v)[R], double* lds, int tid, double* row) {
  block_reduce<R, IC_BLK>(v, lds, tid);
  if (tid < R) {
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < IC_BLK / 64; wv++) s += lds[wv * R + tid];
    row[tid] = s;
  }
}

// (the body of block bx of k_icp_pairs: taken by whole blocks)
__device__ __forceinline__ void icp_pairs_block(const float4* W, int n, const float4* nnpt, const float* sqd, const unsigned char* beaten /* or null */, double thr2, int* match,
                                                float* dsq, double* part, int bx) {
  __shared__ double lds[(IC_BLK / 64) * IC_R1];
  const int tid = threadIdx.x, i = bx * IC_BLK + tid;
  double v[IC_R1] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (i < n) {
    const float4 w = W[i], q = nnpt[i];
    const float d = sqd[i];
    int j = icp_forward(w, q, d, thr2);
    if (j >= 0 && beaten && beaten[i]) j = -1;
    match[i] = j;
    dsq[i] = w.w != 0.f ? d : __builtin_nanf("");
    if (j >= 0) v[0] = (double)d, v[1] = (double)w.x, v[2] = (double)w.y, v[3] = (double)w.z, v[4] = (double)q.x, v[5] = (double)q.y, v[6] = (double)q.z, v[7] = 1.0;
  }
  icp_block_row<IC_R1>(v, lds, tid, part + (size_t)bx * IC_R1);
}

__global__ __launch_bounds__(IC_BLK) void k_icp_pairs(const float4* W, int n, const float4* nnpt, const float* sqd, const unsigned char* beaten /* or null */, double thr2,
                                                      int* match, float* dsq, double* part) {
  icp_pairs_block(W, n, nnpt, sqd, beaten, thr2, match, dsq, part, (int)blockIdx.x);
}

// out[r] = the rows' column r added in block order from 0.0 (one block of 64, R <= 64)
__device__ __forceinline__ void icp_sums_lane(const double* part, int nblk, int R, double* out, int r) {
  if (r >= R) return;
  double s = 0.0;
  for (int b = 0; b < nblk; b++) s += part[(size_t)b * R + r];
  out[r] = s;
}

__global__ __launch_bounds__(64) void k_icp_sums(const double* part, int nblk, int R, double* out) {
  icp_sums_lane(part, nblk, R, out, (int)threadIdx.x);
}

// (the body of block bx of k_icp_cross: taken by whole blocks)
__device__ __forceinline__ void icp_cross_block(const float4* W, int n, const float4* nnpt, const int* match, const double* sum1, double* part, int bx) {
  __shared__ double lds[(IC_BLK / 64) * IC_R2];
  const int tid = threadIdx.x, i = bx * IC_BLK + tid;
  double v[IC_R2] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double cnt = sum1[7];
  if (i < n && cnt > 0.0 && match[i] >= 0) {
    const float4 w = W[i], q = nnpt[i];
    const double px = (double)w.x - sum1[1] / cnt, py = (double)w.y - sum1[2] / cnt, pz = (double)w.z - sum1[3] / cnt;
    const double qx = (double)q.x - sum1[4] / cnt, qy = (double)q.y - sum1[5] / cnt, qz = (double)q.z - sum1[6] / cnt;
    v[0] = qx * px, v[1] = qx * py, v[2] = qx * pz, v[3] = qy * px, v[4] = qy * py, v[5] = qy * pz, v[6] = qz * px, v[7] = qz * py, v[8] = qz * pz;
  }
  icp_block_row<IC_R2>(v, lds, tid, part + (size_t)bx * IC_R2);
}

__global__ __launch_bounds__(IC_BLK) void k_icp_cross(const float4* W, int n, const float4* nnpt, const int* match, const double* sum1, double* part) {
  icp_cross_block(W, n, nnpt, match, sum1, part, (int)blockIdx.x);
}

// IC5: R = U S V^T of the 3x3 A (row-major) by a one-sided Jacobi SVD: columns of G = A V are rotated until they are orthogonal, their norms
// are the singular values.  With u0, u1 the two leading left vectors and u2 = u0 x u1, U S V^T with S = diag(1, 1, sign(det U det V)) is
// u0 v0^T + u1 v1^T + det(V) u2 v2^T whatever sign an SVD gives its third pair.  Rank 1: u1 is completed deterministically (R is not unique
// there); A = 0: R = I.
APD_HD void icp_rotation(const double* A, double* R) {
  double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int q = 0; q < 9; q++) G[q] = A[q];
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double al = 0, be = 0, ga = 0;
      for (int r = 0; r < 3; r++) al += G[3 * r + p] * G[3 * r + p], be += G[3 * r + q] * G[3 * r + q], ga += G[3 * r + p] * G[3 * r + q];
      if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int r = 0; r < 3; r++) {
        const double gp = G[3 * r + p], gq = G[3 * r + q], vp = V[3 * r + p], vq = V[3 * r + q];
        G[3 * r + p] = c * gp - s * gq, G[3 * r + q] = s * gp + c * gq;
        V[3 * r + p] = c * vp - s * vq, V[3 * r + q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double sg[3];
  for (int c = 0; c < 3; c++) sg[c] = sqrt(G[c] * G[c] + G[3 + c] * G[3 + c] + G[6 + c] * G[6 + c]);
  int o0 = 0, o1 = 1, o2 = 2;  // columns by descending singular value
  if (sg[o1] > sg[o0]) { const int t = o0; o0 = o1, o1 = t; }
  if (sg[o2] > sg[o0]) { const int t = o0; o0 = o2, o2 = t; }
  if (sg[o2] > sg[o1]) { const int t = o1; o1 = o2, o2 = t; }
  for (int q = 0; q < 9; q++) R[q] = (q % 4 == 0) ? 1.0 : 0.0;
  if (!(sg[o0] > 0.0)) return;
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
  for (int r = 0; r < 3; r++) u0[r] = G[3 * r + o0] / sg[o0], v0[r] = V[3 * r + o0], v1[r] = V[3 * r + o1], v2[r] = V[3 * r + o2];
  if (sg[o1] > 1e-300 && sg[o1] > 1e-15 * sg[o0]) {
    for (int r = 0; r < 3; r++) u1[r] = G[3 * r + o1] / sg[o1];
  } else {  // rank 1: the axis least aligned with u0, made orthogonal to it
    const int a = fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2]) ? 0 : fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2;
    double e[3] = {0, 0, 0};
    e[a] = 1.0;
    double nn = 0;
    for (int r = 0; r < 3; r++) u1[r] = e[r] - u0[a] * u0[r], nn += u1[r] * u1[r];
    nn = sqrt(nn);
    for (int r = 0; r < 3; r++) u1[r] /= nn;
  }
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  const double detV = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v0[1] * (v1[0] * v2[2] - v1[2] * v2[0]) + v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
  const double sgn = detV < 0.0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (u0[r] * v0[c] + u1[r] * v1[c]) + sgn * u2[r] * v2[c];
}

// IC4 .. IC7 on the record: sums[0 .. 7] and the nine cross sums are in; everything else of the record is the state before this iteration
APD_HD void icp_step_record(IcpRecord& rec, const double* sum1, const double* cross, const IcpConsts& c) {
  for (int q = 0; q < 7; q++) rec.sums[q] = sum1[q];
  for (int q = 0; q < 9; q++) rec.sums[7 + q] = cross[q];
  const double cnt = sum1[7];
  rec.n_corr = (long long)cnt;
  rec.mse = cnt > 0.0 ? sum1[0] / cnt : 0.0;
  for (int q = 0; q < 16; q++) rec.T_k[q] = (q % 5 == 0) ? 1.f : 0.f;
  rec.estimated = 0, rec.converged = 0, rec.stop = 1;
  if (rec.n_corr < (long long)c.min_corr) {  // IC4
    rec.state = IC_NO_CORRESPONDENCES;
    return;
  }
  rec.state = IC_NOT_CONVERGED;
  double A[9], R[9], t[3];
  for (int q = 0; q < 9; q++) A[q] = cross[q] / cnt;
  icp_rotation(A, R);
  const double pm[3] = {sum1[1] / cnt, sum1[2] / cnt, sum1[3] / cnt}, qm[3] = {sum1[4] / cnt, sum1[5] / cnt, sum1[6] / cnt};
  for (int r = 0; r < 3; r++) t[r] = qm[r] - ((R[3 * r] * pm[0] + R[3 * r + 1] * pm[1]) + R[3 * r + 2] * pm[2]);
  bool finite = true;
  for (int r = 0; r < 3; r++) {
    for (int cc = 0; cc < 3; cc++) rec.T_k[r + 4 * cc] = (float)R[3 * r + cc], finite = finite && isfinite(rec.T_k[r + 4 * cc]);
    rec.T_k[r + 12] = (float)t[r], finite = finite && isfinite(rec.T_k[r + 12]);
  }
  if (!finite) return;  // IC5: the loop stops, converged = 0
  rec.estimated = 1;
  if (!c.accumulate) return;
  float F[16];  // IC6: final = T_k * final, ((a0 b0 + a1 b1) + a2 b2) + a3 b3
  for (int r = 0; r < 4; r++)
    for (int cc = 0; cc < 4; cc++)
      F[r + 4 * cc] = ((rec.T_k[r] * rec.final_T[4 * cc] + rec.T_k[r + 4] * rec.final_T[4 * cc + 1]) + rec.T_k[r + 8] * rec.final_T[4 * cc + 2]) + rec.T_k[r + 12] * rec.final_T[4 * cc + 3];
  for (int q = 0; q < 16; q++) rec.final_T[q] = F[q];
  rec.iterations += 1;
  // IC7
  if (rec.iterations >= c.max_iterations) {
    rec.state = IC_ITERATIONS, rec.converged = 1;
    return;
  }
  bool similar = false;
  const double cosa = 0.5 * ((((double)rec.T_k[0] + (double)rec.T_k[5]) + (double)rec.T_k[10]) - 1.0);
  const double tsq = ((double)rec.T_k[12] * (double)rec.T_k[12] + (double)rec.T_k[13] * (double)rec.T_k[13]) + (double)rec.T_k[14] * (double)rec.T_k[14];
  if (cosa >= c.rot_thr && tsq <= c.trans_eps) {
    if (rec.similar >= c.max_similar) {
      rec.state = IC_TRANSFORM, rec.converged = 1;
      return;
    }
    similar = true;
  }
  if (fabs(rec.mse - rec.prev_mse) < c.mse_abs) {
    if (rec.similar >= c.max_similar) {
      rec.state = IC_ABS_MSE, rec.converged = 1;
      return;
    }
    similar = true;
  }
  if (fabs(rec.mse - rec.prev_mse) / rec.prev_mse < c.mse_rel) {
    if (rec.similar >= c.max_similar) {
      rec.state = IC_REL_MSE, rec.converged = 1;
      return;
    }
    similar = true;
  }
  rec.similar = similar ? rec.similar + 1 : 0;
  rec.prev_mse = rec.mse;
  rec.stop = 0;
}

// one wave: the nine cross sums in block order from 0.0, then IC4 .. IC7 in lane 0, which is the only lane to return true (the record is written)
__device__ __forceinline__ bool icp_step_wave(const double* part2, int nblk, const double* sum1, IcpRecord* rec, const IcpConsts& c) {
  __shared__ double cross[IC_R2];
  const int r = threadIdx.x;
  if (r < IC_R2) {
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += part2[(size_t)b * IC_R2 + r];
    cross[r] = s;
  }
  __syncthreads();
  if (r != 0) return false;
  IcpRecord l = *rec;
  icp_step_record(l, sum1, cross, c);
  *rec = l;
  return true;
}

__global__ __launch_bounds__(64) void k_icp_step(const double* part2, int nblk, const double* sum1, IcpRecord* rec, IcpConsts c) {
  (void)icp_step_wave(part2, nblk, sum1, rec, c);
}

// getters: the caller's indexing
__global__ void k_icp_export(const int* match, const float* dsq, const int* perm_src, const int* perm_tgt, int n, int* out_match, float* out_sq) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int o = perm_src[s], j = match[s];
  out_match[o] = j >= 0 ? perm_tgt[j] : -1;
  out_sq[o] = dsq[s];
}
__global__ void k_icp_export_w(const float4* W, const int* perm_src, int n, float* out3) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const float4 w = W[s];
  float* o = out3 + 3ll * perm_src[s];
  const float nan = __builtin_nanf("");
  o[0] = w.w != 0.f ? w.x : nan, o[1] = w.w != 0.f ? w.y : nan, o[2] = w.w != 0.f ? w.z : nan;
}

}  // namespace apd
