// fast_gicp::FastVGICPCuda (gicp/impl/fast_vgicp_cuda_impl.hpp, cuda/fast_vgicp_cuda.cu), the FAST_VGICP_CUDA branch of
// select_registration_method() (registrations.cpp:51-61), as a mode of the registration handle.  The semantics are the numbered list
// VC1 .. VC10 of include/apdgicp_hip.h; the kernels follow it item by item:
//   k_vcb_knn_raw     VC1 / VC2: the engine's exact k-NN (knn_cov_coop_wave) with the KNN_EPI_RAWSUM epilogue -- the covariance of
//                     covariance_estimation.cu:26-34 over the 20 neighbours in rank order, per point in the caller's order
//   k_vcb_regularize  VC3: one lane per point -- eigen-decomposition (sym3_eig), the planarity flag of PLANE, the regularised covariance; the
//                     kept points of every block counted (ego_block_counts)
//   k_vcb_scan        VC4: scan_bsum_block of apd_voxel.hpp over the block counts; the total is n_kept
//   k_vcb_scatter     VC4: kept points, their covariances and their original indices to slot order (ego_block_slot): the caller's order is kept
//   These four take the cloud from a table (VcbSlot) indexed by blockIdx.y, grid (ceil(max n / per block), clouds): the single handle launches
//   them over one cloud, the batch handle (VC11) over every uncached slot of a batch, so both prepare a cloud with the same instructions.
//   (map)             VC5: k_vg_keys / the pair sort / k_vg_voxels of apd_vgicp.hpp over the kept target points
//   k_vc_linearize    VC6 / VC7: vg_linearize_point_of over the offset table, one kept source point per lane
//   (error, reduce)   VC8: k_vg_error and k_vg_reduce of apd_vgicp.hpp as they are -- they read stored indices, not offsets
// fp64 except the stored points, compiled without contraction.  No floating-point atomics.  Every pointer is a kernel argument or in a table that is one.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_ego.hpp"
#include "apd_kernels.hpp"
#include "apd_vgicp.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr int VC_K = 20;                 // VC1: setCorrespondenceRandomness is a no-op (fast_vgicp_cuda_impl.hpp:38)
constexpr int VC_BLK = EGO_BLK;          // regularize / scatter: 16 waves, one point per lane (ego_block_counts / ego_block_slot)
constexpr int VC_MAX_RADIUS = 4;         // VC6: DIRECT_RADIUS up to 4 -> offsets of magnitude <= VgTableOffsets::REACH
constexpr int VC_MAX_OFFSETS = 257;      // ... and at most this many of them
constexpr double VC_PLANE_RATIO = 0.1;   // covariance_regularization.cu:26-31: kept iff lambda1 > 0.1 lambda2
static_assert(VC_MAX_RADIUS <= VgTableOffsets::REACH, "the linearize range test covers the largest offset");

// VC3: raw[6 i ..] -> flag[i], reg[6 i ..] (both in the caller's order), bsum[block] = kept points of the block.  The body of one block.
__device__ __forceinline__ void vc_regularize_block(const double* raw, int n, int method, unsigned char* flag, double* reg, int* bsum, int* wsum) {
  const int i = blockIdx.x * VC_BLK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const double* r = raw + 6 * (size_t)i;
    const Sym3 C{r[0], r[1], r[2], r[3], r[4], r[5]};
    Sym3 out;
    if (method == APDGICP_REG_PLANE) {
      double w[3], u[9];
      sym3_eig(C, w, u);                       // descending: w[0] = lambda2, w[1] = lambda1, w[2] = lambda0
      keep = w[1] > VC_PLANE_RATIO * w[0];     // (false for a NaN)
      out = sym3_from_eig(u, 1.0, 1.0, 1e-3);  // the 1e-3 on the smallest eigenvalue's vector
    } else {                                   // MIN_EIG / FROBENIUS: no filter (the setter refuses everything else)
      keep = true;
      (void)regularize_cov(method, C, out);
    }
    flag[i] = keep ? 1 : 0;
    double* o = reg + 6 * (size_t)i;
    o[0] = out.xx, o[1] = out.xy, o[2] = out.xz, o[3] = out.yy, o[4] = out.yz, o[5] = out.zz;
  }
  ego_block_counts(keep, wsum, bsum);
}

// VC4: bsum scanned (scan_bsum_block), *total = n_kept.  kcov: [6][n_kept] like the engine's covariances, so that k_vg_voxels and the
// linearize read it as they read those; ident[j] = j stands where those kernels expect the original-index -> curve-position table.
__device__ __forceinline__ void vc_scatter_block(const float4* opts, const double* reg, const unsigned char* flag, int n, const int* bsum, const int* total, float4* kpts,
                                                 double* kcov, int* kept_index, int* ident, int* wsum) {
  const int i = blockIdx.x * VC_BLK + threadIdx.x;
  const bool ok = i < n && flag[i];
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  const int nk = *total;
  if (!ok || slot < 0 || slot >= nk || nk > n) return;
  kpts[slot] = opts[i];
  const double* r = reg + 6 * (size_t)i;
#pragma unroll
  for (int q = 0; q < 6; q++) kcov[(size_t)q * nk + slot] = r[q];
  kept_index[slot] = i;
  ident[slot] = slot;
}

// ---- the preparation, the slot in the grid: a single handle prepares a list of one cloud, a batch handle every uncached slot of a batch
struct VcbSlot {                         // what the preparation of one slot reads and writes: one hop from blockIdx.y
  const float4* opts;                    // the slot's points, the caller's order (Engine::Cloud::opts)
  double* raw;                           // [n][6]  VC2, the caller's order
  double* reg6;                          // [n][6]  VC3, the caller's order
  unsigned char* flag;                   // [n]     kept?
  int* bsum;                             // [ceil(n / VC_BLK)] block counts, then their exclusive scan
  int* total;                            // the slot's word of the kept counts
  float4* kpts;                          // [n_kept] (sized for n)
  double* kcov;                          // [6][n_kept] (sized for n)
  int* kept;                             // [n_kept] original indices
  int* ident;                            // [n_kept] j -> j
  int n, pad_;
};

// VC1 / VC2 for slots[y], whose cloud is clouds[cloud_ids[y]]
template <int L>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(APD_KNN_WPE, 8))) void k_vcb_knn_raw(const CloudDesc* clouds, const int* cloud_ids, const VcbSlot* slots, int k,
                                                                                                         int* err_flag, unsigned long long* stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long knn_smem[];
  unsigned bx, by;
  xcd_remap(bx, by);
  const CloudDesc c = clouds[cloud_ids[by]];
  knn_cov_coop_wave<L, KNN_EPI_RAWSUM>(c, bx, (int)threadIdx.x, knn_smem, k, 0, err_flag, stats, 0, nullptr, slots[by].raw);  // (returns when bx is beyond c.n)
}

__global__ __launch_bounds__(VC_BLK) void k_vcb_regularize(const VcbSlot* slots, int method) {
  __shared__ int wsum[VC_BLK / 64];
  const VcbSlot s = slots[blockIdx.y];
  if ((int)(blockIdx.x * VC_BLK) >= s.n) return;  // (the whole block: nothing behind this is reached by a part of it)
  vc_regularize_block(s.raw, s.n, method, s.flag, s.reg6, s.bsum, wsum);
}

__global__ __launch_bounds__(SCAN_BLK) void k_vcb_scan(const VcbSlot* slots) {
  __shared__ int lds[SCAN_BLK / 64];
  const VcbSlot s = slots[blockIdx.x];
  scan_bsum_block(s.bsum, (s.n + VC_BLK - 1) / VC_BLK, s.total, lds);
}

__global__ __launch_bounds__(VC_BLK) void k_vcb_scatter(const VcbSlot* slots) {
  __shared__ int wsum[VC_BLK / 64];
  const VcbSlot s = slots[blockIdx.y];
  if ((int)(blockIdx.x * VC_BLK) >= s.n) return;
  vc_scatter_block(s.opts, s.reg6, s.flag, s.n, s.bsum, s.total, s.kpts, s.kcov, s.kept, s.ident, wsum);
}

// VC6 / VC7: as k_vg_linearize, the offsets from a table of noff x 3 ints
__global__ __launch_bounds__(VG_BLK) void k_vc_linearize(const float4* kpts, const double* kcov, const int* ident, int n, VgMap map, const double* T12, double res,
                                                         const int* __restrict__ offsets, int noff, int want_Hb, int* corr, double* part) {
  __shared__ double red[(VG_BLK / 64) * VG_SUMS];
  const int tid = threadIdx.x, i = blockIdx.x * VG_BLK + tid;
  Rigid T;
#pragma unroll
  for (int q = 0; q < 12; q++) T.m[q] = T12[q];
  double acc[VG_SUMS];
#pragma unroll
  for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
  if (i < n) {
    vg_linearize_point_of(kpts, kcov, ident, n, map, T, res, VgTableOffsets{offsets}, noff, want_Hb, corr, i, acc);
  }
  vg_block_sums<VG_SUMS>(acc, red, part, tid);
}

}  // namespace apd
