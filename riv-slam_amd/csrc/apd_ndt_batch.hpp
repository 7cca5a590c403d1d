// NDT (P2D / D2D) as a mode of the BATCH handle: the per-row arithmetic of apd_ndt.hpp (nd_linearize_row / nd_error_row, the same device
// functions the single handle's kernels call) under the per-pair optimiser state machine and the two-launch tick of apd_vgicp_batch.hpp.  The
// semantics are N10 .. N15 of include/apdgicp_hip.h.  One tick:
//   k_ndb_points<D2D>  grid (ceil(max n_src / VG_BLK), pairs): reads the pair's status -- NEED_LIN: the linearize row at x0, NEED_ERR: the error
//                      row at xi over the frozen indices and the pose x0 of the last linearize, DONE or a block at or beyond the pair's row
//                      count: return.  In D2D the row count is the source slot's voxel count, one load of a device word per block.
//   k_ndb_step         grid (pairs), one wave: the first ceil(rows / VG_BLK) block rows of the pair -- exactly those the blocks of this tick
//                      wrote -- added in block order from 0.0, then N8 or the GN / LM step (vgb_step_pair)
// k_vgb_init and k_vgb_records serve this mode as they are.  The maps are the single handle's (k_vg_keys .. k_ndt_voxels, unchanged) in
// buffers sized for as many voxels as the slot has points, the voxel count left on the device.  fp64 without contraction, no floating-point
// atomics, every pointer a kernel argument or in a table that is one, nothing talks across blocks inside a launch.
//
// The compiler's report for gfx950 (-Rpass-analysis=kernel-resource-usage), blocks of 256:
//   k_ndb_points<true>   (D2D)  138 VGPRs, no scratch, 3 waves per SIMD, LDS 928 bytes (4 x 29 doubles)
//   k_ndb_points<false>  (P2D)  120 VGPRs, no scratch, 4 waves per SIMD, LDS 928 bytes
//   k_ndb_step                   70 VGPRs, no scratch, 7 waves per SIMD, LDS 1664 bytes
// The merged kernel holds both branches without spilling (the single handle's k_ndt_linearize is at 136 / 122), so the error branch is not a
// kernel of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_ndt.hpp"
#include "apd_vgicp_batch.hpp"

namespace apd {

#pragma clang fp contract(off)

struct NdbPair {                         // everything the tick reads of one pair: one hop from the pair index
  const float4* opts;                    // source points, the caller's order (Engine::Cloud::opts)
  int n, pad_;                           // source points
  VgbMap smap;                           // of the pair's source slot (D2D; P2D: null pointers, never read)
  VgbMap map;                            // of the pair's target slot
};

// rows of a pair: source voxels (D2D, the device word; never more than the slot has points) or source points (P2D)
template <bool D2D>
__device__ __forceinline__ int ndb_rows(const NdbPair& pd) {
  return D2D ? min(*pd.smap.nv, pd.n) : pd.n;
}

// corr: [pair][corr_stride] ints (rows x noff of the pair in front), part: [pair][nblk_max][VG_RED]
template <bool D2D>
__global__ __launch_bounds__(VG_BLK) void k_ndb_points(const NdbPair* pairs, const PairState* st, double res, int mode, int noff, int* corr, size_t corr_stride,
                                                       double* part, int nblk_max) {
  __shared__ double red[(VG_BLK / 64) * VG_SUMS];
  const int pair = blockIdx.y, tid = threadIdx.x;
  const int status = st[pair].status;
  if (status == ST_DONE) return;
  const NdbPair pd = pairs[pair];
  const int nrows = ndb_rows<D2D>(pd);
  if ((int)(blockIdx.x * VG_BLK) >= nrows) return;
  const int i = blockIdx.x * VG_BLK + tid;
  const VgMap map = vgb_load_map(pd.map);
  const VgMap smap = D2D ? vgb_load_map(pd.smap) : VgMap{nullptr, nullptr, nullptr, nullptr, 0};
  int* pc = corr + (size_t)pair * corr_stride;
  double* pp = part + (size_t)pair * nblk_max * VG_RED;
  const Rigid T0 = st[pair].x0;
  double acc[VG_SUMS];
#pragma unroll
  for (int r = 0; r < VG_SUMS; r++) acc[r] = 0.0;
  if (status == ST_NEED_LIN) {
    if (i < nrows) nd_linearize_row<D2D>(pd.opts, smap, map, T0, res, mode, noff, 1, pc, i, acc);
    vg_block_sums<VG_SUMS>(acc, red, pp, tid);
  } else {
    const Rigid T = st[pair].xi;
    if (i < nrows) nd_error_row<D2D>(pd.opts, smap, map, T, T0, res, noff, pc, i, acc);
    nd_error_block_sums(acc, red, pp, tid);
  }
}

// d2d: the pair's rows are its source slot's voxels
__global__ __launch_bounds__(64) void k_ndb_step(const NdbPair* pairs, PairState* st, Consts cst, const double* part, int nblk_max, int d2d, ResultRec* out, int* done) {
  const int pair = blockIdx.x;
  const int rows = d2d ? ndb_rows<true>(pairs[pair]) : ndb_rows<false>(pairs[pair]);
  vgb_step_pair(pair, (rows + VG_BLK - 1) / VG_BLK, st, cst, part, nblk_max, out, done);
}

}  // namespace apd
