// FAST_VGICP_CUDA as a mode of the BATCH handle.  The semantics are VC11 .. VC16 of include/apdgicp_hip.h.  The preparation (VC11) is the
// mode's one preparation, the slot-indexed kernels of apd_vgicp_cuda.hpp: one launch sequence prepares every uncached slot of a batch.  This
// file holds the tick.
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
