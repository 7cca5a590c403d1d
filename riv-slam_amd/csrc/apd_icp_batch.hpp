// Point-to-point ICP as a mode of the BATCH handle: the per-point and per-step arithmetic of apd_icp.hpp (icp_init_point .. icp_step_wave, the
// same device functions the single handle's kernels call) with the pair in the grid and the loop on the device.  The semantics are IC11 .. IC16
// of include/apdgicp_hip.h.  One tick of the whole batch:
//   (forward search)   the engine's exact search over a pair table whose source is the pair's W at the identity pose; PairState::n_lin stays 0,
//                      so every search is cold (W moves while the pose stays the identity: a kept neighbour would be unproven), and a pair whose
//                      status is DONE is skipped by the search itself
//   k_icb_boxes x 2    reciprocal, pruned: the chunk and group boxes of every running pair's W, grid (boxes, pairs)
//   k_icb_recip<P>     reciprocal: grid (blocks, pairs)
//   k_icb_pairs        grid (blocks, pairs): gate, match, the eight first-pass sums per block
//   k_icb_sums         grid (pairs), one wave: the pair's OWN ceil(n / 256) rows in block order from 0.0 (the row buffer has one stride for all
//                      pairs and keeps the rows of earlier, larger aligns behind them)
//   k_icb_cross        grid (blocks, pairs)
//   k_icb_step         grid (pairs), one wave: the one-lane step on the pair's IcpRecord, its trace entry; a pair that stops writes its result
//                      record, becomes DONE and bumps the done counter.  It also says whether THIS tick's T_k is to be applied (IcbAux::apply_tick)
//   k_icb_transform    grid (blocks, pairs): W = T_k * W for the pairs whose step of this very tick estimated one -- the last iteration
//                      included, the ticks enqueued behind a pair's end excluded: T_k is applied exactly once per iteration
// Every block of a DONE pair returns on reading its status.  7 launches per tick forward, 10 reciprocal (8 with the brute reciprocal search), none
// of which depends on the number of pairs or points.  Nothing inside a launch talks to another block; no floating-point atomics; compiled without
// contraction.  Every pointer is a kernel argument or in a table that is one.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_icp.hpp"
#include "apd_sort.hpp"

namespace apd {

#pragma clang fp contract(off)

struct IcbPair {            // what is the pair's own: one hop from the pair index
  const float4* src;        // the source slot's points, curve order (Engine::Cloud::pts): read once, by k_icb_winit
  const int* perm;          // the source slot's curve position -> caller's index
  float4* W;                // the pair's working cloud, n points in the source's curve order
  Box* cbox;                // W's chunk and group boxes (reciprocal search)
  Box* gbox;
  int n, pad_;
};

struct IcbAux {
  int apply_tick;           // the tick whose k_icb_transform applies the record's T_k (-1: none)
  int n_trace;              // iterations of this align so far
};

struct IcbTrace {           // one iteration, as apdgicp_icp_get_trace returns it
  float T_k[16];
  long long n_corr;
  double mse;
  int similar, pad_;
};

struct IcbTab {             // the per-pair arrays of an align: [pair] or [pair][stride]
  const IcbPair* pairs;
  PairState* st;            // the engine's: status (NEED_LIN / DONE), x0 = identity, n_lin = 0
  IcpRecord* rec;           // [pair]
  IcbAux* aux;              // [pair]
  IcbTrace* trace;          // [pair][trace_cap]
  const float4* nnpt;       // [pair][nstride]  the engine's search results (Work::nnpt / sqd)
  const float* sqd;
  int* match;               // [pair][nstride]
  float* dsq;
  unsigned char* beaten;
  double* part;             // [pair][nblk_max][IC_R2]: the rows of either pass
  double* sum1;             // [pair][IC_R1]
  int nstride, nblk_max, trace_cap, pad_;
};

__device__ __forceinline__ bool icb_identity16(const float* T) {
  bool id = true;
#pragma unroll
  for (int q = 0; q < 16; q++) id = id && T[q] == ((q % 5 == 0) ? 1.f : 0.f);
  return id;
}

// per pair: the search state (identity pose, cold, running), the record started at the guess, no trace; the done counter of this align
__global__ void k_icb_init(IcbTab t, const float* guess16 /* [pair][16], column-major */, int npairs, int* done) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) *done = 0;
  if (p >= npairs) return;
  init_pair_state(t.st[p], nullptr, 1);
  IcpRecord r;
  for (int q = 0; q < 16; q++) r.T_k[q] = (q % 5 == 0) ? 1.f : 0.f, r.final_T[q] = guess16[16 * p + q], r.sums[q] = 0.0;
  r.mse = 0.0, r.prev_mse = 1.7976931348623157e308;  // DBL_MAX
  r.n_corr = 0;
  r.iterations = 0, r.similar = 0, r.state = IC_NOT_CONVERGED, r.converged = 0, r.stop = 0, r.estimated = 0;
  t.rec[p] = r;
  t.aux[p] = IcbAux{-1, 0};
}

// IC1 / IC11: W0 of every pair from its source slot and its guess (the source itself when the guess is the identity)
__global__ void k_icb_winit(const IcbPair* pairs, const float* guess16, int xf_linear) {
  const int pair = blockIdx.y;
  const IcbPair pd = pairs[pair];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pd.n) return;
  const float* T = guess16 + 16 * (size_t)pair;
  icp_init_point(pd.src, icb_identity16(T) ? nullptr : T, xf_linear, pd.W, i);
}

// which: 0 the chunk boxes, 1 the group boxes
__global__ void k_icb_boxes(IcbTab t, int which) {
  const int pair = blockIdx.y;
  if (t.st[pair].status == ST_DONE) return;
  const IcbPair pd = t.pairs[pair];
  const int per = which ? (int)kGroupPts : (int)kChunk;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (pd.n + per - 1) / per) return;
  box_of_points(pd.W, pd.n, per, which ? pd.gbox : pd.cbox, c);
}

template <bool PRUNED>
__global__ __launch_bounds__(IC_BLK) void k_icb_recip(IcbTab t, double thr2) {
  const int pair = blockIdx.y;
  if (t.st[pair].status == ST_DONE) return;
  const IcbPair pd = t.pairs[pair];
  if ((int)(blockIdx.x * IC_BLK) >= pd.n) return;
  const size_t o = (size_t)pair * t.nstride;
  icp_recip_block<PRUNED>(pd.W, pd.n, pd.perm, pd.cbox, pd.gbox, t.nnpt + o, t.sqd + o, thr2, t.beaten + o, (int)blockIdx.x);
}

__global__ __launch_bounds__(IC_BLK) void k_icb_pairs(IcbTab t, int recip, double thr2) {
  const int pair = blockIdx.y;
  if (t.st[pair].status == ST_DONE) return;
  const IcbPair pd = t.pairs[pair];
  if ((int)(blockIdx.x * IC_BLK) >= pd.n) return;
  const size_t o = (size_t)pair * t.nstride;
  icp_pairs_block(pd.W, pd.n, t.nnpt + o, t.sqd + o, recip ? t.beaten + o : nullptr, thr2, t.match + o, t.dsq + o, t.part + (size_t)pair * t.nblk_max * IC_R2, (int)blockIdx.x);
}

__global__ __launch_bounds__(64) void k_icb_sums(IcbTab t) {
  const int pair = blockIdx.x;
  if (t.st[pair].status == ST_DONE) return;
  const int nblk = (t.pairs[pair].n + IC_BLK - 1) / IC_BLK;
  icp_sums_lane(t.part + (size_t)pair * t.nblk_max * IC_R2, nblk, (int)IC_R1, t.sum1 + (size_t)pair * IC_R1, (int)threadIdx.x);
}

__global__ __launch_bounds__(IC_BLK) void k_icb_cross(IcbTab t) {
  const int pair = blockIdx.y;
  if (t.st[pair].status == ST_DONE) return;
  const IcbPair pd = t.pairs[pair];
  if ((int)(blockIdx.x * IC_BLK) >= pd.n) return;
  const size_t o = (size_t)pair * t.nstride;
  icp_cross_block(pd.W, pd.n, t.nnpt + o, t.match + o, t.sum1 + (size_t)pair * IC_R1, t.part + (size_t)pair * t.nblk_max * IC_R2, (int)blockIdx.x);
}

__global__ __launch_bounds__(64) void k_icb_step(IcbTab t, IcpConsts c, int tick, ResultRec* out, int* done) {
  const int pair = blockIdx.x;
  if (t.st[pair].status == ST_DONE) return;  // (the whole wave)
  const int nblk = (t.pairs[pair].n + IC_BLK - 1) / IC_BLK;
  IcpRecord* rec = t.rec + pair;
  if (!icp_step_wave(t.part + (size_t)pair * t.nblk_max * IC_R2, nblk, t.sum1 + (size_t)pair * IC_R1, rec, c)) return;
  // lane 0, behind the step
  IcbAux a = t.aux[pair];
  if (a.n_trace < t.trace_cap) {
    IcbTrace& e = t.trace[(size_t)pair * t.trace_cap + a.n_trace];
    for (int q = 0; q < 16; q++) e.T_k[q] = rec->T_k[q];
    e.n_corr = rec->n_corr, e.mse = rec->mse, e.similar = rec->similar, e.pad_ = 0;
  }
  a.n_trace += 1;
  a.apply_tick = rec->estimated ? tick : -1;
  t.aux[pair] = a;
  if (rec->stop) {  // IC8
    ResultRec r;
    for (int q = 0; q < 16; q++) r.T[q] = rec->final_T[q];
    r.final_cost = rec->mse;
    r.converged = rec->converged;
    r.iterations = rec->iterations, r.n_linearize = rec->iterations;
    r.n_compute_error = 0, r.lm_failed = 0;
    r.n_matched = (int)(rec->n_corr < 2147483647ll ? rec->n_corr : 2147483647ll);
    out[pair] = r;
    t.st[pair].status = ST_DONE;
    atomicAdd(done, 1);
  }
}

__global__ void k_icb_transform(IcbTab t, int tick, int xf_linear) {
  const int pair = blockIdx.y;
  if (t.aux[pair].apply_tick != tick) return;
  const IcbPair pd = t.pairs[pair];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pd.n) return;
  icp_transform_point(pd.W, t.rec[pair].T_k, xf_linear, i);
}

// getters of one pair: apd_icp.hpp's k_icp_export / k_icp_export_w serve as they are

}  // namespace apd
