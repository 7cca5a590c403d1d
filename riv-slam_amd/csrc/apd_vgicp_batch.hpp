// Voxelized GICP as a mode of the BATCH handle: the per-point arithmetic of apd_vgicp.hpp (vg_linearize_point / vg_error_point, the same device
// functions the single handle's kernels call) under the per-pair optimiser state machine of apd_kernels.hpp (PairState, lm_after_gather,
// lm_decide_after_sum, step_done).  The semantics are V8 .. V12 of include/apdgicp_hip.h.  One tick is two launches:
//   k_vgb_points   grid (ceil(max n_src / VG_BLK), pairs): reads the pair's status -- NEED_LIN: the linearize body at x0, NEED_ERR: the error
//                  body at xi over the frozen indices and the pose x0 of the last linearize, DONE or a block beyond the pair's n: return
//   k_vgb_step     grid (pairs), one wave: the pair's block rows added in block order from 0.0 (k_vg_reduce's order), then the GN / LM step in
//                  one lane; a pair that finishes writes its record and bumps the done counter
// Nothing inside a launch talks to another block, so there is no fence and no arrival counter; a pair's record depends on nothing but the pair
// (V11).  The voxel maps are the single handle's (k_vg_keys .. k_vg_voxels, unchanged) with the voxel count left on the device: VgbMap::nv.
// fp64 without contraction, no floating-point atomics, every pointer a kernel argument or in a table that is one.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_vgicp.hpp"

namespace apd {

#pragma clang fp contract(off)

struct VgbMap {                          // a slot's voxel map; buffers sized for nv <= n, the count itself stays on the device
  const unsigned long long* keys;
  const int* count;
  const double* mean;
  const double* cov;
  const int* nv;
};

struct VgbPair {                         // everything the tick reads of one pair: one hop from the pair index
  const float4* opts;                    // source points, the caller's order (Engine::Cloud::opts)
  const double* cov;                     // source covariances, curve order (Engine::Cloud::cov)
  const int* inv;                        // source: original index -> position on the curve
  int n, pad_;
  VgbMap map;                            // of the pair's target slot
};

__device__ __forceinline__ VgMap vgb_load_map(const VgbMap& m) { return VgMap{m.keys, m.count, m.mean, m.cov, *m.nv}; }

// L:56-59 for every pair, and the done counter of this align
__global__ void k_vgb_init(PairState* st, const Rigid* guesses, int npairs, int max_iterations, int* done) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) *done = 0;
  if (p >= npairs) return;
  init_pair_state(st[p], guesses + p, max_iterations);
}

// corr: [pair][corr_stride] ints (n x noff of the pair in front), part: [pair][nblk_max][VG_RED]
__global__ __launch_bounds__(VG_BLK) void k_vgb_points(const VgbPair* pairs, const PairState* st, double res, int mode, int noff, int* corr, size_t corr_stride,
                                                       double* part, int nblk_max) {
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
    if (i < n) vg_linearize_point(pd.opts, pd.cov, pd.inv, n, map, T0, res, mode, noff, 1, pc, i, acc);
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

// the step of one pair by one wave, shared by every batch mode that ticks this way (k_vgb_step, k_ndb_step of apd_ndt_batch.hpp): the first
// nblk block rows of the pair added in block order from 0.0, then V7 / N8 or the GN / LM step in lane 0
__device__ __forceinline__ void vgb_step_pair(int pair, int nblk, PairState* st, const Consts& cst, const double* part, int nblk_max, ResultRec* out, int* done) {
  __shared__ PairState ls;
  __shared__ double v[32], ws[48];
  const int tid = threadIdx.x;
  const int status = st[pair].status;
  if (status == ST_DONE) return;
  const double* rows = part + (size_t)pair * nblk_max * VG_RED;
  if (tid < VG_SUMS && (status == ST_NEED_LIN || tid >= 27)) {
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += rows[(size_t)b * VG_RED + tid];
    v[tid] = s;
  }
  for (int q = tid; q < (int)(sizeof(PairState) / 8); q += 64) ((double*)&ls)[q] = ((const double*)&st[pair])[q];
  __syncthreads();
  if (tid == 0) {
    if (status == ST_NEED_LIN) {
      fill_from_sums(ls, v);
      ls.n_matched = (int)fmin(v[28], 2147483647.0);  // (the int32 field saturates, as on the single handle)
      if (v[28] == 0.0) {  // V7 / N8: no correspondence, no contributing term -- the loop ends here, the pose so far stands
        ls.n_lin += 1;
        ls.status = ST_DONE;
      } else {
        lm_after_gather(ls, cst, ws, nullptr);
      }
    } else {
      lm_decide_after_sum(ls, v[27], cst, ws, nullptr);
    }
    if (ls.status == ST_DONE) {
      out[pair] = result_record(ls);
      atomicAdd(done, 1);
    }
  }
  __syncthreads();
  for (int q = tid; q < (int)(sizeof(PairState) / 8); q += 64) ((double*)&st[pair])[q] = ((const double*)&ls)[q];
}

__global__ __launch_bounds__(64) void k_vgb_step(const VgbPair* pairs, PairState* st, Consts cst, const double* part, int nblk_max, ResultRec* out, int* done) {
  const int pair = blockIdx.x;
  vgb_step_pair(pair, (pairs[pair].n + VG_BLK - 1) / VG_BLK, st, cst, part, nblk_max, out, done);
}

// max_iterations <= 0: no tick runs, every pair's record is that of its initial state
__global__ void k_vgb_records(const PairState* st, int npairs, ResultRec* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < npairs) out[p] = result_record(st[p]);
}

}  // namespace apd
