// FAST_VGICP_CUDA as a mode of the BATCH handle.  The semantics are VC11 .. VC16 of include/apdgicp_hip.h.  Two groups of kernels:
//
// Preparation (VC11), the slot in the grid -- one launch sequence prepares every uncached slot of a batch, nothing in it waits for the host:
//   k_vcb_knn_raw     VC1 / VC2: knn_cov_coop_wave with the KNN_EPI_RAWSUM epilogue, grid (ceil(max n / queries per wave), slots); the cloud
//                     comes from cloud_ids[y], the output pointer from the slot table; a wave beyond its slot's n returns inside the wave function
//   k_vcb_regularize  VC3: vc_regularize_block of apd_vgicp_cuda.hpp, grid (ceil(max n / VC_BLK), slots)
//   k_vcb_scan        VC4: scan_bsum_block of apd_voxel.hpp, one block per slot; the total goes to the slot's word of ONE array of kept counts
//   k_vcb_scatter     VC4: vc_scatter_block
// The bodies are the device functions the single handle's kernels call, so a slot's prepared cloud is the single handle's, bit for bit.
//
// Tick (VC13 / VC16), two launches:
//   k_vcb_points      grid (ceil(max n_kept / VG_BLK), pairs): k_vgb_points of apd_vgicp_batch.hpp with the offsets from a table (VC6) -- NEED_LIN:
//                     vg_linearize_point_of over VgTableOffsets at x0, NEED_ERR: vg_error_point at xi over the frozen indices and x0.  DIRECT1 / 7 /
//                     27 come through the same table, as on the single handle (k_vc_linearize).
//   k_vgb_step        of apd_vgicp_batch.hpp as it is; the pair table (VgbPair) carries the kept points, their covariances ([6][n_kept]), the
//                     identity index table and n_kept where the VGICP mode carries the whole cloud
// fp64 without contraction, no floating-point atomics, every pointer a kernel argument or in a table that is one.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_vgicp_batch.hpp"
#include "apd_vgicp_cuda.hpp"

namespace apd {

#pragma clang fp contract(off)

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

// The per-point pass of a tick: k_vgb_points with VgTableOffsets where that one has VgModeOffsets.  (One block body for both kernels was
// tried: it moved k_vgb_points' register allocation, and existing kernels keep their instruction streams -- docs/experiments.md.)
// corr: [pair][corr_stride] ints (n_kept x noff of the pair in front), part: [pair][nblk_max][VG_RED]; offsets: noff x 3 ints
__global__ __launch_bounds__(VG_BLK) void k_vcb_points(const VgbPair* pairs, const PairState* st, double res, const int* __restrict__ offsets, int noff, int* corr,
                                                       size_t corr_stride, double* part, int nblk_max) {
  __shared__ double red[(VG_BLK / 64) * VG_SUMS];
  const int pair = blockIdx.y, tid = threadIdx.x;
  const int status = st[pair].status;
  if (status == ST_DONE) return;
  const VgbPair pd = pairs[pair];
  const int n = pd.n;
  if ((int)(blockIdx.x * VG_BLK) >= n) return;
  const int i = blockIdx.x * VG_BLK + tid;
  const VgMap map = vgb_load_map(pd.map);
  int* pc = corr + (size_t)pair * corr_stride;
  double* pp = part + (size_t)pair * nblk_max * VG_RED;
  const Rigid T0 = st[pair].x0;
  if (status == ST_NEED_LIN) {
    double acc[VG_SUMS];
#pragma unroll
    for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
    if (i < n) vg_linearize_point_of(pd.opts, pd.cov, pd.inv, n, map, T0, res, VgTableOffsets{offsets}, noff, 1, pc, i, acc);
    vg_block_sums<VG_SUMS>(acc, red, pp, tid);
  } else {
    const Rigid T = st[pair].xi;
    double acc[2] = {0.0, 0.0};
    if (i < n) vg_error_point(pd.opts, pd.cov, pd.inv, n, map, T, T0, noff, pc, i, acc);
    block_reduce<2, VG_BLK>(acc, red, tid);
    if (tid < 2) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < VG_BLK / 64; w++) s += red[w * 2 + tid];
      pp[(size_t)blockIdx.x * VG_RED + 27 + tid] = s;
    }
  }
}

}  // namespace apd
