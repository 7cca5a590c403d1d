// libapdgicp_hip.so -- the C ABI declared in include/apdgicp_hip.h, on top of apd::Engine.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC (see build.py)
#include <cstddef>
#include <functional>
#include <cmath>
#include <limits>
#include <memory>
#include <new>

#include "apd_engine.hpp"
#include "apd_voxel.hpp"
#include "apd_filter.hpp"
#include "apd_ego.hpp"
#include "apd_floor.hpp"
#include "apd_map.hpp"
#include "apd_scan_context.hpp"
#include "apd_vgicp.hpp"
#include "apd_vgicp_batch.hpp"
#include "apd_vgicp_cuda.hpp"
#include "apd_vgicp_cuda_batch.hpp"
#include "apd_ndt.hpp"
#include "apd_ndt_batch.hpp"
#include "apd_icp.hpp"
#include "apd_icp_batch.hpp"
#include "apd_gicp_mp.hpp"
#include "apd_dbscan.hpp"
#include "apd_ingest.hpp"
#include "apd_approx_voxel.hpp"
#include "apd_search.hpp"

using namespace apd;

// Exclusive scan of v[0 .. n) in place, enqueued on stream: tiles of SCAN_BLK * SCAN_ITEMS, then their sums (tile_sums: one int per tile, left
// scanned); *total = the sum of all.
static int scan_tiles(int64_t n) { return (int)((n + SCAN_BLK * SCAN_ITEMS - 1) / (SCAN_BLK * SCAN_ITEMS)); }
static void enqueue_exclusive_scan(hipStream_t stream, int* v, int n, int* tile_sums, int* total) {
  const int nt = scan_tiles(n);
  hipLaunchKernelGGL(k_map_scan_tiles, dim3(nt), dim3(SCAN_BLK), 0, stream, v, n, tile_sums);
  hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, stream, tile_sums, nt, total);
}

// The stable LSD radix sort of apd_map.hpp, 8 bits per pass, over u64 keys or (key, int) pairs.  The caller sizes the scratch (ensure), writes
// the keys into keys_a (pairs: their values into val_a) in stream order and enqueues the passes (enqueue_radix_sort).
struct RadixDims {
  int nblk, entries, nsb;  // blocks of MAP_RS_TILE keys; histogram entries of a pass; scan tiles of that histogram
};
static RadixDims radix_dims(int n) {
  const int nblk = (int)(((int64_t)n + MAP_RS_TILE - 1) / MAP_RS_TILE);
  return RadixDims{nblk, 256 * nblk, scan_tiles(256ll * nblk)};
}
struct RadixScratch {
  DevBuf keys_a, keys_b, val_a, val_b, hist, tile_sums;  // tile_sums: nsb ints, then the word that takes the total of a pass's scan (nobody reads it)
  // sized for n keys (pairs: and n values).  With `grows` given it only says whether that would replace a buffer and replaces none: the caller
  // waits for the stream first, then calls again without.
  int ensure(int n, bool pairs, bool* grows = nullptr) {
    const RadixDims d = radix_dims(n);
    const size_t kb = (size_t)n * 8, vb = pairs ? (size_t)n * 4 : 0, hb = (size_t)d.entries * 4, tb = ((size_t)d.nsb + 1) * 4;
    if (grows) {
      *grows = kb > keys_a.cap || kb > keys_b.cap || vb > val_a.cap || vb > val_b.cap || hb > hist.cap || tb > tile_sums.cap;
      return 0;
    }
    APD_TRY(keys_a.ensure(kb));
    APD_TRY(keys_b.ensure(kb));
    APD_TRY(val_a.ensure(vb));
    APD_TRY(val_b.ensure(vb));
    APD_TRY(hist.ensure(hb));
    return tile_sums.ensure(tb);
  }
};
struct RadixSorted {  // where the sorted keys and values ended (vals: null without pairs), and the launches that took
  unsigned long long* keys;
  int* vals;
  int launches;
};
// `passes` passes from bit 0 over the n keys in s.keys_a, s sized for n (and for pairs) by the caller.  Enqueues only, never waits.
static RadixSorted enqueue_radix_sort(hipStream_t stream, RadixScratch& s, int n, int passes, bool pairs) {
  const RadixDims d = radix_dims(n);
  unsigned long long *ka = s.keys_a.as<unsigned long long>(), *kb = s.keys_b.as<unsigned long long>();
  int *va = pairs ? s.val_a.as<int>() : nullptr, *vb = pairs ? s.val_b.as<int>() : nullptr, *hist = s.hist.as<int>(), *sums = s.tile_sums.as<int>();
  for (int p = 0; p < passes; p++) {
    hipLaunchKernelGGL(k_map_rs_hist, dim3(d.nblk), dim3(MAP_RS_BLK), 0, stream, ka, n, 8 * p, d.nblk, hist);
    enqueue_exclusive_scan(stream, hist, d.entries, sums, sums + d.nsb);
    if (pairs) hipLaunchKernelGGL(k_map_rs_scatter_pairs, dim3(d.nblk), dim3(MAP_RS_BLK), 0, stream, ka, va, kb, vb, n, 8 * p, d.nblk, hist, sums);
    else hipLaunchKernelGGL(k_map_rs_scatter, dim3(d.nblk), dim3(MAP_RS_BLK), 0, stream, ka, kb, n, 8 * p, d.nblk, hist, sums);
    std::swap(ka, kb), std::swap(va, vb);
  }
  return RadixSorted{ka, va, 4 * passes};
}

// The scratch of one voxel-map build (k_vg_keys, the pair sort, k_map_heads): one per handle, used by whichever voxel mode is on.  Builds
// follow each other in stream order.  bsum: the head count of every block of MAP_BLK sorted keys.
struct VoxSortScratch {
  RadixScratch radix;
  DevBuf bsum;
  int ensure(int n, bool* grows = nullptr) {  // (grows: as RadixScratch::ensure)
    const size_t hb = (size_t)(n + MAP_BLK - 1) / MAP_BLK * 4;
    APD_TRY(radix.ensure(n, true, grows));
    if (grows) {
      *grows = *grows || hb > bsum.cap;
      return 0;
    }
    return bsum.ensure(hb);
  }
};

// The buffers of one voxel map, voxels in ascending key order (vraw: NDT only).  What the map was made from stays with its owner, per mode.
struct VoxMapBufs {
  DevBuf vkeys, vcount, vmean, vraw, vcov;
  int ensure(size_t voxels, bool raw) {
    APD_TRY(vkeys.ensure(voxels * 8));
    APD_TRY(vcount.ensure(voxels * 4));
    APD_TRY(vmean.ensure(voxels * 24));
    if (raw) APD_TRY(vraw.ensure(voxels * 48));
    return vcov.ensure(voxels * 48);
  }
  VgMap map(int nv) const { return VgMap{vkeys.as<unsigned long long>(), vcount.as<int>(), vmean.as<double>(), vcov.as<double>(), nv}; }
  VgbMap map(const int* nv_word) const { return VgbMap{vkeys.as<unsigned long long>(), vcount.as<int>(), vmean.as<double>(), vcov.as<double>(), nv_word}; }
};

static int n_offsets(int neighbor_search) { return neighbor_search == APDGICP_VGICP_DIRECT27 ? 27 : neighbor_search == APDGICP_VGICP_DIRECT7 ? 7 : 1; }

// The frozen state of the last linearize of whichever voxel mode is on (V6 / VC8 / N7): the voxel indices it found (rows x noff ints), the
// block rows of the reduction, the pose pair on the device and the 44 doubles read back.  ONE per handle (apdgicp_handle::lin): set_mode()
// clears `have` on every transition, so nothing in here ever has to outlive a mode switch.  What a linearize was made FROM stays with the
// mode, as identity stamps (lin_src_gen, lin_build, ...), and so does the test that those still name what the handle holds.
struct FrozenLin {
  bool have = false;
  int rows = 0, noff = 0;
  double T_lin[12];
  DevBuf corr, part, T, out;
};

// apdgicp_set_vgicp: the voxel map of the target and what the last linearize was made from (include/apdgicp_hip.h, V1 .. V7).  The scratch of
// a map build and the frozen state are the handle's (apdgicp_handle::sort, apdgicp_handle::lin).
struct VgState {
  apdgicp_vgicp_params prm{1.0, APDGICP_VGICP_DIRECT1, APDGICP_VGICP_ADDITIVE};
  // What the cached pieces were made FROM, by identity: apdgicp_handle::cloud_gen names the points of a slot (and their order on the curve),
  // Engine::Cloud::cov_gen one writing of a cloud's covariances.  A piece is used only while those still name what the handle holds, so no call
  // that replaces a cloud or recomputes covariances -- with the mode on or off, through whichever entry point -- can leave a stale piece in use.
  bool map_built = false;      // the map: target points map_tgt_gen, their covariances map_cov_gen, map_res, map_mode
  uint64_t map_tgt_gen = 0, map_cov_gen = 0;
  double map_res = 0.0;
  int map_mode = 0;
  uint64_t inv_src_gen = 0;    // inv_s: the inverse of the permutation of source points inv_src_gen, inv_n entries
  int inv_n = 0;
  uint64_t lin_src_gen = 0, lin_src_cov_gen = 0;  // apdgicp_handle::lin: a linearize of source lin_src_gen with covariances lin_src_cov_gen against map number lin_build
  int64_t lin_build = 0;
  int64_t n_vox = 0, builds = 0;
  VoxMapBufs buf;
  DevBuf scal, inv_t, inv_s;
  VgMap map() const { return buf.map((int)n_vox); }
};

// VC1 .. VC4 of one cloud, on either handle kind: a pure function of (points, regularisation), cached by identity
struct VcPrepared {
  bool ready = false;
  uint64_t pts_gen = 0;          // which setting of the cloud's points it was made from (apdgicp_handle::cloud_gen / Engine::Cloud::pts_gen)
  int reg = 0;
  int64_t id = 0;                // which preparation this is (the owner's preps when it was made): names it for the map and the frozen state
  int n = 0, n_kept = 0;
  DevBuf raw, reg6, flag, bsum, kpts, kcov, kept, ident;  // raw / reg6 / flag: per point of the cloud; the rest sized for n kept points
};

// VC6: the offsets of p (checked by the caller), 3 ints each
static void vc_offsets(const apdgicp_vgicp_cuda_params& p, std::vector<int32_t>& out) {
  out.clear();
  auto push = [&](int i, int j, int k) { out.push_back(i), out.push_back(j), out.push_back(k); };
  if (p.neighbor_search == APDGICP_VGICP_DIRECT1) {
    push(0, 0, 0);
  } else if (p.neighbor_search == APDGICP_VGICP_DIRECT7) {  // VC:55-64
    push(0, 0, 0), push(1, 0, 0), push(-1, 0, 0), push(0, 1, 0), push(0, -1, 0), push(0, 0, 1), push(0, 0, -1);
  } else if (p.neighbor_search == APDGICP_VGICP_DIRECT27) {  // VC:66-75
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) push(i - 1, j - 1, k - 1);
  } else {  // VC:77-90
    const int range = (int)std::ceil(p.search_radius);
    for (int i = -range; i <= range; i++)
      for (int j = -range; j <= range; j++)
        for (int k = -range; k <= range; k++)
          if (std::sqrt((double)(i * i + j * j + k * k)) <= p.search_radius + 1e-3) push(i, j, k);
  }
}

// VC6: the offset table (3 ints per offset), what it was made from, and its device copy
struct VcOffsets {
  std::vector<int32_t> host;
  int search = -1;
  double radius = 0.0;
  CachedTable dev;
  int count() const { return (int)(host.size() / 3); }
  void clear() { host.clear(); }
  int ensure(const apdgicp_vgicp_cuda_params& prm, hipStream_t stream) {
    if (host.empty() || search != prm.neighbor_search || radius != prm.search_radius) {
      vc_offsets(prm, host);
      search = prm.neighbor_search, radius = prm.search_radius;
    }
    return dev.upload(host.data(), host.size() * sizeof(int32_t), stream);
  }
};

// apdgicp_set_vgicp_cuda: per cloud the prepared cloud (kept points, their covariances, their original indices), the voxel map of the
// prepared target and what the last linearize was made from (include/apdgicp_hip.h, VC1 .. VC10).  The scratch of a map build, the frozen
// state and the Hessian of the last align are the handle's (apdgicp_handle::sort, ::lin, ::final_H).
struct VcState {
  apdgicp_vgicp_cuda_params prm{1.0, APDGICP_VGICP_DIRECT1, 1.5, APDGICP_REG_PLANE, APDGICP_NN_CPU_PARALLEL_KDTREE};
  VcPrepared pc[2];              // [source, target]; swapped with the clouds
  int64_t preps = 0;
  bool map_built = false;        // the map: prepared target map_prep_id at map_res
  int64_t map_prep_id = 0;
  double map_res = 0.0;
  int64_t n_vox = 0, builds = 0;
  VcOffsets offs;
  int64_t lin_src_id = 0, lin_build = 0;  // apdgicp_handle::lin: a linearize of prepared source lin_src_id against map number lin_build
  VoxMapBufs buf;
  CachedTable prep_tab[2], prep_ids[2];  // per cloud, the VcbSlot table and the cloud id of its preparation: uploaded again only when a pointer or n changes
  DevBuf scal;                   // ints: [0, 4) a map build, [4 + which] n_kept of cloud `which`'s preparation
  VgMap map() const { return buf.map((int)n_vox); }
};

// apdgicp_set_ndt: the voxel maps of target and source and what the last linearize was made from (include/apdgicp_hip.h, N1 .. N9).  The
// scratch of a map build, the frozen state and the Hessian of the last align are the handle's (apdgicp_handle::sort, ::lin, ::final_H).
struct NdState {
  struct Map {                 // one cloud's map: a pure function of (points, resolution), cached by identity like VgState's
    bool built = false;
    uint64_t pts_gen = 0;      // apdgicp_handle::cloud_gen of the points it was made from
    double res = 0.0;
    int64_t id = 0;            // which build this is (NdState::builds when it was made): names the map for the frozen state
    int nv = 0;
    VoxMapBufs buf;
    VgMap map() const { return buf.map(nv); }
  };
  apdgicp_ndt_params prm{1.0, APDGICP_NDT_D2D, APDGICP_VGICP_DIRECT7};
  Map maps[2];                 // [source, target]; swapped with the clouds
  int64_t builds = 0;
  uint64_t lin_src_gen = 0;    // apdgicp_handle::lin: a linearize of source lin_src_gen against map lin_tgt_id (and, D2D, over the rows of map lin_src_id)
  int64_t lin_tgt_id = 0, lin_src_id = 0;
  int lin_mode = 0;
  DevBuf scal;
};

// apdgicp_set_icp: the working cloud W (in the source's curve order), its boxes, the matches and the record of the last iteration
// (include/apdgicp_hip.h, IC1 .. IC10).  The forward search runs through the engine's own buffers (Work::nnpt / sqd).
struct IcState {
  apdgicp_icp_params prm{1, 0, 3, 0, -std::numeric_limits<double>::max(), 0.0, 1e-12};
  bool brute = false;          // APDGICP_ICP_RECIP_MODE=brute (read when the handle is created): the reciprocal search without its boxes
  bool have = false;           // W / match / dsq describe source points have_src_gen (n_have of them) against target points have_tgt_gen
  uint64_t have_src_gen = 0, have_tgt_gen = 0;
  int n_have = 0;
  int state = APDGICP_ICP_NOT_CONVERGED;
  int64_t launches = 0, waits = 0;  // of the last align
  std::vector<float> tr_T;     // the trace of the last align: 16 floats per iteration
  std::vector<int64_t> tr_n;
  std::vector<double> tr_mse;
  std::vector<int32_t> tr_sim;
  DevBuf W, cbox, gbox, beaten, match, dsq, part, sum1, rec, dT;
  PinnedBuf h_rec;             // mirror of rec: one IcpRecord
};

// apdgicp_set_gicp_mp: the queries, the rows of the last linearize (counts, offsets and keys in buffers of its OWN, so that a Q call between two
// linearizes changes nothing here), the fused distributions, the block rows and the trace of the last align (include/apdgicp_hip.h,
// MP1 .. MP11).  The Hessian of the last linearize is the handle's (apdgicp_handle::final_H).
struct MpState {
  apdgicp_gicp_mp_params prm{1, 0, 0.5};
  bool have = false;           // cnt / pos / bsum / keys / fused describe source points have_src_gen (n_have of them) against target points have_tgt_gen
  uint64_t have_src_gen = 0, have_tgt_gen = 0;
  int n_have = 0;
  int64_t total = 0;           // entries of all rows of that linearize
  uint64_t inv_tgt_gen = 0;    // inv_t: the inverse of the permutation of target points inv_tgt_gen, inv_n entries
  int inv_n = 0;
  int state = APDGICP_GICP_MP_NOT_CONVERGED;
  int64_t launches = 0, waits = 0;  // of the last align
  std::vector<double> tr_pose, tr_cost, tr_delta;  // the trace of the last align: 16 / 1 / 6 doubles per iteration
  std::vector<int64_t> tr_n;
  DevBuf q, cnt, pos, bsum, visit, keys, inv_t, fused, part, out, T, tot;
  // apdgicp_gicp_mp_set_profiling: events at the phase boundaries of a linearize (tests/measure/bench_gicp_mp.py), read behind its last wait
  bool profiling = false;
  hipEvent_t ev[8] = {};
  double phase_ms[6] = {0, 0, 0, 0, 0, 0};  // transform, count (+ mask, total), scan, fill, row sort, per-point kernel (+ sums)
  ~MpState() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Which pipeline a handle runs: its own APD-GICP / plain GICP kernels, or one of the modes switched on through apdgicp_[batch_]set_*.
// One value per handle, written by set_mode() alone ("Mode transitions").
enum class Mode { APD, VGICP, VGICP_CUDA, NDT, ICP, GICP_MP };

struct apdgicp_handle {
  Engine eng;   // declared first, so destroyed last: its stream still exists while the members below free their buffers
  VgState vg;   // (freed by its members' destructors, behind the wait of ~apdgicp_handle)
  VcState vc;   // (likewise)
  NdState nd;   // (likewise)
  IcState ic;   // (likewise)
  MpState mp;   // (likewise)
  VoxSortScratch sort;  // (likewise) the scratch of a voxel-map build of whichever voxel mode is on
  FrozenLin lin;        // (likewise) the frozen state of the last linearize of whichever voxel mode is on
  double final_H[36];   // FAST_VGICP_CUDA and NDT: the Hessian of the last align in the mode, on the host (identity until then, and again when either is entered); FastGICPMultiPoints: of the last linearize
  Mode mode = Mode::APD;
  apdgicp_handle() { reset_final_H(); }
  void reset_final_H() {
    for (int q = 0; q < 36; q++) final_H[q] = (q % 7 == 0) ? 1.0 : 0.0;
  }
  ~apdgicp_handle() {
    if (eng.stream) (void)hipStreamSynchronize(eng.stream);  // the voxel kernels run there; the members are freed once this body has run
  }
  uint64_t cloud_epoch = 0, cloud_gen[2] = {0, 0};  // cloud_gen[slot]: which setting of points the slot holds (0: none); swapped with the clouds
  bool pair_ready = false;   // work buffers / descriptors match the current source+target
  bool have_corr = false;    // correspondences_/mahalanobis_ hold a linearize result
  int n_src_at_corr = 0;
  // apdgicp_set_trace: the trace of the last apdgicp_align_host_loop (apdgicp_align leaves its own on the device, Engine::d_trace)
  bool trace_from_host_loop = false;
  std::vector<double> tr_lambda, tr_rho, tr_y0, tr_yi, tr_dnorm, tr_poses;  // poses: 16 doubles each, column-major
};

// What every voxel mode of a batch handle owns per cloud slot and per handle: the slots' voxel maps and their device words, the count of
// builds.  Each mode has its OWN table (VgbState::vox, NdbState::vox, VcbState::vox), so that a mode's cached maps survive a switch to another
// mode and back; what a slot's map was made from stays with the mode, slot by slot, in a list of the same length (its `slots`).
struct VoxSlots {
  struct Slot {
    int nv = 0;                // host copy of the voxel count (the kernels read the device word)
    VoxMapBufs buf;            // sized for nv <= n
  };
  std::vector<Slot> slots;
  DevBuf scal;                 // per slot {first bad point, voxel count, radix scratch word, -}: 4 ints
  int scal_slots = 0;
  int64_t builds = 0;
  int* words(int slot) const { return scal.as<int>() + 4 * (size_t)slot; }
  VgbMap map(int slot) const { return slots[slot].buf.map(words(slot) + 1); }
  void release() {  // apdgicp_batch_clear: the maps go with the clouds
    slots.clear();
    scal.release();
    scal_slots = 0;
  }
};

// apdgicp_batch_set_vgicp (include/apdgicp_hip.h, V8 .. V12): per cloud slot the voxel map and the inverse permutation, cached by identity like
// VgState's pieces.  The scratch of a map build, the state of the device loop and what an align leaves (pair table, frozen indices, block rows)
// are the handle's (apdgicp_batch::sort, ::loop, ::run).
struct VgbState {
  struct Slot {                // (its map: vox.slots, same index)
    bool map_built = false;    // the map: points map_pts_gen, covariances map_cov_gen, map_res, map_mode
    uint64_t map_pts_gen = 0, map_cov_gen = 0;
    double map_res = 0.0;
    int map_mode = 0;
    uint64_t inv_pts_gen = 0;  // inv: the inverse of the permutation of points inv_pts_gen (0: none)
    DevBuf inv;
  };
  apdgicp_vgicp_params prm{1.0, APDGICP_VGICP_DIRECT1, APDGICP_VGICP_ADDITIVE};
  std::vector<Slot> slots;
  VoxSlots vox;
  void release() { slots.clear(), vox.release(); }  // apdgicp_batch_clear
};

// apdgicp_batch_set_ndt (include/apdgicp_hip.h, N10 .. N15): per cloud slot the NDT voxel map, cached by identity like NdState's.  Scratch,
// device-loop state and what an align leaves: the handle's, as for VgbState.
struct NdbState {
  struct Slot {                // (its map: vox.slots, same index)
    bool built = false;        // the map: points pts_gen, resolution res
    uint64_t pts_gen = 0;
    double res = 0.0;
  };
  apdgicp_ndt_params prm{1.0, APDGICP_NDT_D2D, APDGICP_VGICP_DIRECT7};
  std::vector<Slot> slots;
  VoxSlots vox;
  void release() { slots.clear(), vox.release(); }  // apdgicp_batch_clear
};

// apdgicp_batch_set_icp (include/apdgicp_hip.h, IC11 .. IC16): per align the working clouds of all pairs (one buffer, a slice per pair), their
// boxes, matches, block rows and records.  Nothing is kept per cloud slot.  The state of the device loop is the handle's (apdgicp_batch::loop).
struct IcbState {
  apdgicp_icp_params prm{1, 0, 3, 0, -std::numeric_limits<double>::max(), 0.0, 1e-12};
  bool brute = false;          // APDGICP_ICP_RECIP_MODE=brute (read when the handle is created), as on the single handle
  // what the getters may read: the last align in this mode, while no cloud slot has been written since (epoch: Engine::pts_epoch at the align)
  bool have = false;
  uint64_t have_epoch = 0;
  std::vector<int> src, tgt, n_src;      // per pair of that align: slots and source size
  std::vector<size_t> w_off;             // ... and where its W starts (points)
  int nstride = 0, trace_cap = 0;
  int64_t launches = 0, waits = 0, ticks = 0;  // of the last align
  DevBuf W, cbox, gbox, beaten, match, dsq, part, sum1, rec, aux, trace, guess;
  CachedTable pairs, nn_pairs;  // IcbPair per pair; the engine's PairDesc with W as the source
  void release() {  // apdgicp_batch_clear
    have = false;
    W.release(), cbox.release(), gbox.release(), beaten.release(), match.release(), dsq.release(), part.release(), sum1.release(), rec.release(), aux.release(),
        trace.release(), guess.release(), pairs.dev.release(), nn_pairs.dev.release();
  }
};

// apdgicp_batch_set_vgicp_cuda (include/apdgicp_hip.h, VC11 .. VC16): per cloud slot the prepared cloud of VC1 .. VC4 and, for targets, the voxel
// map of its kept points, both cached by identity like VcState's.  Scratch, device-loop state and what an align leaves: the handle's, as for
// VgbState.
struct VcbState {
  struct Slot {                // (its map: vox.slots, same index)
    VcPrepared pc;
    bool map_built = false;    // the map: preparation map_prep_id at map_res
    int64_t map_prep_id = 0;
    double map_res = 0.0;
  };
  apdgicp_vgicp_cuda_params prm{1.0, APDGICP_VGICP_DIRECT1, 1.5, APDGICP_REG_PLANE, APDGICP_NN_CPU_PARALLEL_KDTREE};
  std::vector<Slot> slots;
  VoxSlots vox;
  int64_t preps = 0;
  int64_t prep_waits = 0, map_waits = 0;  // host waits spent preparing clouds / building maps since the handle was created
  double phase_ms[3] = {0, 0, 0};         // of the last align: preparation, map builds, ticks by the host clock (meaningful with profiling on)
  DevBuf nk;                   // per slot: the kept count of its preparation
  int nk_slots = 0;
  VcOffsets offs;
  // what apdgicp_batch_vgicp_cuda_get_correspondences may read of apdgicp_batch::run: the last align in this mode, while no cloud slot has
  // been written since (cleared by every enabling call of the setter, so never another mode's indices)
  bool have = false;
  uint64_t have_epoch = 0;
  std::vector<int> have_nk;    // per pair of that align: kept source points
  CachedTable prep_tab, prep_ids;
  void release() {  // apdgicp_batch_clear: the prepared clouds and the maps go with the clouds
    slots.clear(), vox.release();
    have = false;
    nk.release(), prep_tab.dev.release(), prep_ids.dev.release();
    nk_slots = 0;
  }
};

// What an align of a voxel mode of a batch handle leaves, whichever mode ran it (only one align runs at a time): the pair table, per pair the
// frozen voxel indices of its last linearize and the block rows of the reduction.
struct VoxRun {
  DevBuf corr, part;
  CachedTable pairs;
  size_t corr_stride = 0;      // of the last align: ints between two pairs' indices, offsets per row
  int noff = 0;
  void release() { corr.release(), part.release(), pairs.dev.release(); }  // apdgicp_batch_clear
};

// The device optimiser loop of a batch handle (V12 / N15 / IC15), whichever mode runs it: the done counter the step kernels count into, the
// pinned words the host reads, the events of the last two chunks.
struct DeviceLoop {
  DevBuf done;
  PinnedBuf h_words;           // ints: [0, 2) the done counter as of the last two chunks, [2] the error flag, [4 ...) the scal words of a build
  hipEvent_t ev[2] = {nullptr, nullptr};
  int chunk = 0;               // ticks per enqueued chunk (create time: APDGICP_VGB_CHUNK, default kVgbChunk)
  int last_ticks = 0, last_chunks = 0, last_waits = 0;  // of the last run (waits: event and stream waits of the host)
  void drop_events() {
    for (hipEvent_t& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  void release() {  // apdgicp_batch_clear
    done.release(), h_words.release();
    drop_events();
  }
  ~DeviceLoop() { drop_events(); }
};

struct apdgicp_batch {
  Engine eng;   // declared first, so destroyed last: its stream still exists while the members below free their buffers
  VgbState vg;  // (freed by its members' destructors, behind the wait of ~apdgicp_batch)
  NdbState nd;  // (likewise)
  IcbState ic;  // (likewise)
  VcbState vc;  // (likewise)
  VoxSortScratch sort;  // (likewise) the scratch of a voxel-map build of whichever voxel mode is on
  VoxRun run;           // (likewise) the pair table, frozen indices and block rows of the last align of whichever voxel mode ran it
  Mode mode = Mode::APD;
  DeviceLoop loop;      // (likewise; its events by its own destructor)
  int64_t slot_pairs[2] = {0, 0};  // pairs of the last two enqueued batches (by ticket parity)
  void release_voxel_modes() {  // apdgicp_batch_clear
    vg.release();
    nd.release();
    ic.release();
    vc.release();
    run.release();
    sort = VoxSortScratch{};
    loop.release();
  }
  ~apdgicp_batch() {
    if (eng.stream) {
      (void)hipSetDevice(eng.device);
      (void)hipStreamSynchronize(eng.stream);
    }
  }
};

struct apdgicp_submap {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevBuf stage, cat, keys, pos, bsum, out, scal;  // scal: box6[6], total, err
  CachedTable jobs;
  PinnedBuf h_scal;  // mirror of {total, err}: 2 ints
  int method = APDGICP_DOWNSAMPLE_VOXELGRID;  // apdgicp_submap_set_downsample_method: sticky
  RadixScratch av_sort;                       // APPROX_VOXELGRID (apd_approx_voxel.hpp): the (hash, point) pair sort,
  DevBuf av_evict, av_tiles, av_head, av_words;  // the eviction flags and their scan, the run heads, AV_WORDS ints
  int64_t n_last = 0;
  bool last_is_cat = false;  // no downsampling: the result is the concatenation itself
  ~apdgicp_submap() {
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_scan_filter {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  apdgicp_scan_filter_params prm;
  apdgicp_submap* vox = nullptr;  // step 2 with a leaf: the voxel grid of the submap target, on this object's stream
  Engine* eng = nullptr;          // step 3: packs, sorts and boxes the cloud of step 2 like a registration cloud (created when first needed)
  DevBuf stage, gated, dense, stat, kept, out, bsum, scal;  // scal: int counts[4] {gate, compaction, output, -}, double {mean, stddev, thr}
  PinnedBuf h_scal;               // mirror of scal + the engine's error flag
  const float* result = nullptr;
  int64_t counts[4] = {0, 0, 0, 0};
  int64_t n_stat = 0;
  double mean = 0, stddev = 0, thr = 0;
  ~apdgicp_scan_filter() {
    if (stream) (void)hipStreamSynchronize(stream);
    delete eng;
    delete vox;
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_ego_velocity {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  apdgicp_ego_velocity_params prm;
  DevBuf stage, rows_all, valid, rows, src, bsum, words, vk, n_in, samples, rec;
  DevBuf in_row, in_xyzi, in_dop, in_src, out_row, out_xyzi, out_dop, out_src;
  PinnedBuf h_rec;  // mirror of rec: one EgoRecord
  int64_t n_last = 0;
  int K_last = 0, S_last = 0;
  bool ran = false;
  EgoRecord* record() { return h_rec.as<EgoRecord>(); }
  ~apdgicp_ego_velocity() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_floor {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  apdgicp_floor_params prm;
  Engine* eng = nullptr;  // the normal filter: packs, sorts and boxes the clipped cloud like a registration cloud (created when first needed)
  DevBuf stage, tilted, mask, clip, clip_src, stat, filt, filt_src, bsum, words, coef, bad, n_in, samples, rec, state;
  DevBuf in_xyzi, in_src, in_row, under_xyzi, under_src;
  PinnedBuf h_rec;  // mirror of rec + the engine's error flag
  int64_t n_last = 0;
  int K_last = 0;
  bool ran = false, stat_valid = false;
  FloorRecord* record() { return h_rec.as<FloorRecord>(); }
  ~apdgicp_floor() {
    if (stream) (void)hipStreamSynchronize(stream);
    delete eng;
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_map_cloud {
  struct Keyframe {
    DevBuf pts;  // float4 {x, y, z, intensity}
    int64_t n = 0;
  };
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::vector<Keyframe> kfs;
  RadixScratch sort;  // of the voxel keys (keys only)
  DevBuf stage, pushed, bsum, bmin, out, state;
  CachedTable jobs;
  PinnedBuf h_state;  // mirror of state: one MapState
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  apdgicp_map_cloud_stats info;
  const float* result = nullptr;
  int64_t n_last = 0;
  void forget() {
    result = nullptr, n_last = 0;
    memset(&info, 0, sizeof(info));  // (sort_kind: always 0, the radix sort)
  }
  ~apdgicp_map_cloud() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_scan_context {
  apdgicp_scan_context_params prm;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int cap = 0, size = 0;  // descriptors the four database buffers hold / in use
  DevBuf desc, ring_key, sector_key, col_norm;
  DevBuf stage, hi1, lo1, inv1, rec, hi2, lo2, inv2, out;
  CachedTable qtab, cand;
  PinnedBuf h_out;  // ScRec records
  std::vector<uint32_t> seen;  // per id: the call that listed it last (duplicate check)
  uint32_t epoch = 0;
  ScDb db() const { return ScDb{desc.as<float>(), ring_key.as<float>(), sector_key.as<double>(), col_norm.as<double>()}; }
  ScDb slot(int id) const {
    const size_t R = (size_t)prm.num_ring, S = (size_t)prm.num_sector;
    return ScDb{desc.as<float>() + id * R * S, ring_key.as<float>() + id * R, sector_key.as<double>() + id * S, col_norm.as<double>() + id * S};
  }
  ~apdgicp_scan_context() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_dbscan {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  apdgicp_dbscan_params prm;
  RadixScratch sort;  // the three pair sorts of a run, one after the other
  DevBuf stage, stage_dop, pts, dop, gkeys, spts, cnt, core, score, parent, root, seed, nextra, size, ncore, rank_of, cseed, csize, tsum, mcount, msum, offsets, members,
      labels, table, scal;
  PinnedBuf h_scal;  // mirror of scal: DB_WORDS ints
  int64_t n_last = 0, K_last = 0, M_last = 0;
  bool ran = false;
  int64_t launches = 0;   // of the last run (tests/measure/bench_dbscan.py)
  bool profiling = false; // apdgicp_dbscan_set_profiling: events at the phase boundaries, one more wait at the end of a run
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double phase_ms[5] = {0, 0, 0, 0, 0};  // sort (cells, sort, sorted copy) / count / union + flatten / border / output
  ~apdgicp_dbscan() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

struct apdgicp_scan_ingest {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  apdgicp_scan_ingest_params prm;
  DevBuf stage_xyz, stage_int, stage_dop, rows, index, bsum, scal;  // run: the staged lanes of a host message, the output, scal: int n_out
  DevBuf stage_cloud, desk;                                           // deskew: the staged host cloud, the output
  PinnedBuf h_scal;                                                   // mirror of scal
  int64_t n_rows = 0, n_desk = 0;
  int64_t launches = 0, waits = 0;  // of the last run / run_polar / deskew / histogram_add (tests/measure/bench_scan_ingest.py, bench_polar_ingest.py)
  DevBuf stage_polar[5];            // run_polar: the staged lanes of a host message (one array of structures: [0] alone)
  DevBuf stage_hist, hist, hist_sum;  // histogram: the staged host cloud; int counts[100] + ticket; int64 sum[100] + frames (H2)
  bool hist_live = false;           // hist / hist_sum exist and hist_sum was zeroed on the stream
  ~apdgicp_scan_ingest() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

constexpr int kSrc = 0, kTgt = 1;
const char* cloud_name(int which) { return which == kSrc ? "source" : "target"; }

// What the error texts call a mode and the setter that switches it on, indexed by Mode.
struct ModeText {
  const char *name, *setter;
};
constexpr ModeText kModeText[] = {{"APD-GICP", ""}, {"voxelized GICP", "set_vgicp"}, {"FAST_VGICP_CUDA", "set_vgicp_cuda"}, {"NDT", "set_ndt"}, {"point-to-point ICP", "set_icp"}, {"FastGICPMultiPoints", "set_gicp_mp"}};
// a getter of mode m on a handle that is in another one: "NDT is off (apdgicp_batch_set_ndt)"
int mode_is_off(Mode m, bool batch) {
  const ModeText& t = kModeText[(int)m];
  return fail(APDGICP_ERR_NO_INPUT, std::string(t.name) + " is off (apdgicp_" + (batch ? "batch_" : "") + t.setter + ")");
}
// align_enqueue / align_collect / pump on a batch handle in mode m (not APD)
int no_pipeline(Mode m) {
  const ModeText& t = kModeText[(int)m];
  return fail(APDGICP_ERR_UNSUPPORTED, std::string(t.name) + " on a batch handle (apdgicp_batch_" + t.setter + ") runs one batch at a time: align_enqueue / align_collect / pump are not offered");
}

void identity16(float* g) {
  memset(g, 0, 16 * sizeof(float));
  g[0] = g[5] = g[10] = g[15] = 1.f;
}

// guess16: the initial guess the caller is about to align with (column-major; null: identity).  It goes into the pair
// table so that the guess buffer is uploaded once per call, not once with a placeholder and once with the real one.
int ensure_pair(apdgicp_handle* h, const float* guess16 = nullptr) {
  Engine& e = h->eng;
  if (e.clouds.size() < 2 || e.clouds[kSrc].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "source cloud is not set");
  if (e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
  const bool need_cov = h->mode != Mode::ICP;  // IC9: the ICP mode searches only, clouds of any size
  if (h->pair_ready && (!need_cov || (e.clouds[kSrc].cov_valid && e.clouds[kTgt].cov_valid))) return 0;
  apdgicp_pair p;
  p.source_cloud = kSrc;
  p.target_cloud = kTgt;
  if (guess16) memcpy(p.guess, guess16, sizeof(p.guess));
  else identity16(p.guess);
  APD_TRY(e.setup_pairs(&p, 1, true, false, need_cov));
  h->pair_ready = true;
  h->have_corr = false;
  return 0;
}


void rigid_to_colmajor(const Rigid& r, double* T) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) T[i + 4 * j] = r.m[4 * i + j];
  T[3] = T[7] = T[11] = 0.0;
  T[15] = 1.0;
}

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(APDGICP_ERR_INTERNAL, "out of host memory");
  } catch (...) {
    return fail(APDGICP_ERR_INTERNAL, "unexpected C++ exception");
  }
}

// order-preserving compaction of src[0..n): count, scan of the block counts (total -> *d_total), scatter
template <int PRED>
int scan_filter_compact(apdgicp_scan_filter* f, const float4* src, const float* stat, double thr, const double* thr_ptr, int n, float4* dst,
                               unsigned char* kept, int* d_total) {
  const int nb = (n + FLT_BLK - 1) / FLT_BLK;
  hipLaunchKernelGGL(k_flt_count<PRED>, dim3(nb), dim3(FLT_BLK), 0, f->stream, src, stat, thr, thr_ptr, n, f->bsum.as<int>());
  hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, f->stream, f->bsum.as<int>(), nb, d_total);
  hipLaunchKernelGGL(k_flt_scatter<PRED>, dim3(nb), dim3(FLT_BLK), 0, f->stream, src, stat, thr, thr_ptr, n, f->bsum.as<int>(), dst, n, kept);
  APD_HIP(hipGetLastError());
  return 0;
}

// ---- voxel maps: what voxelized GICP and NDT share, on single and batch handles (kernels: apd_vgicp.hpp, apd_map.hpp)
constexpr int kVgBadNone = 0x7f7f7f7f;  // (what hipMemsetAsync(0x7f) leaves: above every point index)

struct VoxSorted {  // what enqueue_voxel_sort leaves for k_vg_voxels / k_ndt_voxels (and, in s.bsum, the voxel offset of every head block)
  unsigned long long* keys;
  int* idx;
  unsigned nhb;
};

// The build chain up to the voxel kernel, on s (sized for n by the caller).  Enqueues only, never waits: the four scal words reset, the voxel
// keys of pts[0 .. n) (scal[0]: the first point that has none), the (key, index) pairs sorted, the voxels counted (scal[1]).
int enqueue_voxel_sort(hipStream_t stream, VoxSortScratch& s, const float4* pts, int n, double resolution, int* scal, VoxSorted* sorted) {
  const unsigned nhb = (unsigned)((n + MAP_BLK - 1) / MAP_BLK), nb256 = (unsigned)((n + 255) / 256);
  APD_HIP(hipMemsetAsync(scal, 0x7f, 16, stream));
  hipLaunchKernelGGL(k_vg_keys, dim3(nb256), dim3(256), 0, stream, pts, n, resolution, s.radix.keys_a.as<unsigned long long>(), s.radix.val_a.as<int>(), scal);
  const RadixSorted r = enqueue_radix_sort(stream, s.radix, n, 8, true);  // 63 key bits, 8 per pass
  hipLaunchKernelGGL(k_map_heads, dim3(nhb), dim3(MAP_BLK), 0, stream, r.keys, n, s.bsum.as<int>());
  hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, stream, s.bsum.as<int>(), (int)nhb, scal + 1);
  *sorted = VoxSorted{r.keys, r.vals, nhb};
  return 0;
}

// a build whose scal[0] names a point (what: "voxelized GICP: target point 7", "NDT: point 7 of cloud slot 2")
int voxel_key_range_error(const std::string& what, double resolution) {
  return fail(APDGICP_ERR_INVALID_ARG, what + " is not finite or lies outside the voxel key range (|c| < 2^20 at resolution " + std::to_string(resolution) + ")");
}

// A single handle's build up to the voxel kernel: waits before the scratch may be replaced, sorts pts[0 .. n), waits again to read the voxel
// count *nv.  prefix: "voxelized GICP: " / "NDT: " / "FAST_VGICP_CUDA: "; point_name(j) words point j for the caller ("target point 7"),
// called on the error path only.
template <class PointName>
int handle_sort_voxels(apdgicp_handle* h, const float4* pts, int n, double resolution, DevBuf& scal, const char* prefix, PointName&& point_name, VoxSorted* sorted,
                       int* nv) {
  Engine& e = h->eng;
  APD_HIP(hipStreamSynchronize(e.stream));  // (buffers below, and the caller's after this, may be replaced)
  APD_TRY(h->sort.ensure(n));
  APD_TRY(scal.ensure(16));
  APD_TRY(enqueue_voxel_sort(e.stream, h->sort, pts, n, resolution, scal.as<int>(), sorted));
  APD_HIP(hipGetLastError());
  int hs[4];
  APD_HIP(hipMemcpyAsync(hs, scal.p, sizeof(hs), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  if (hs[0] != kVgBadNone) return voxel_key_range_error(std::string(prefix) + point_name(hs[0]), resolution);
  if (hs[1] < 1 || hs[1] > n) return fail(APDGICP_ERR_INTERNAL, std::string(prefix) + "inconsistent voxel count");
  *nv = hs[1];
  return 0;
}
// (a whole cloud slot: the point's index is the caller's)
int handle_sort_voxels(apdgicp_handle* h, int which, double resolution, DevBuf& scal, const char* prefix, VoxSorted* sorted, int* nv) {
  const Engine::Cloud& c = h->eng.clouds[which];
  return handle_sort_voxels(
      h, c.opts.as<float4>(), c.n, resolution, scal, prefix, [&](int j) { return std::string(cloud_name(which)) + " point " + std::to_string(j); }, sorted, nv);
}

// the getters' read-back of a map of nv voxels: keys unpacked into coordinates, covariances expanded from 6 to 9 (every output may be null)
int read_voxels(hipStream_t stream, const VoxMapBufs& m, int64_t nv, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* raw_covs_n6,
                double* covs_n9) {
  if (capacity < nv) return fail(APDGICP_ERR_INVALID_ARG, "capacity is below the voxel count");
  std::vector<unsigned long long> keys(coords_n3 ? nv : 0);
  std::vector<double> c6(covs_n9 ? 6 * nv : 0);
  if (coords_n3) APD_HIP(hipMemcpyAsync(keys.data(), m.vkeys.p, nv * 8, hipMemcpyDeviceToHost, stream));
  if (counts) APD_HIP(hipMemcpyAsync(counts, m.vcount.p, nv * 4, hipMemcpyDeviceToHost, stream));
  if (means_n3) APD_HIP(hipMemcpyAsync(means_n3, m.vmean.p, nv * 24, hipMemcpyDeviceToHost, stream));
  if (raw_covs_n6) APD_HIP(hipMemcpyAsync(raw_covs_n6, m.vraw.p, nv * 48, hipMemcpyDeviceToHost, stream));
  if (covs_n9) APD_HIP(hipMemcpyAsync(c6.data(), m.vcov.p, nv * 48, hipMemcpyDeviceToHost, stream));
  APD_HIP(hipStreamSynchronize(stream));
  for (int64_t i = 0; i < nv && coords_n3; i++) {
    const unsigned long long k = keys[i];
    coords_n3[3 * i] = (int32_t)((k >> 42) & 0x1fffff) - VG_LIM, coords_n3[3 * i + 1] = (int32_t)((k >> 21) & 0x1fffff) - VG_LIM, coords_n3[3 * i + 2] = (int32_t)(k & 0x1fffff) - VG_LIM;
  }
  for (int64_t i = 0; i < nv && covs_n9; i++) {
    const double* c = &c6[6 * i];
    double* o = covs_n9 + 9 * i;
    o[0] = c[0], o[1] = c[1], o[2] = c[2], o[3] = c[1], o[4] = c[3], o[5] = c[4], o[6] = c[2], o[7] = c[4], o[8] = c[5];
  }
  return 0;
}

// room for the frozen indices and the block rows of a linearize, waiting first when either buffer would be replaced
int ensure_corr_part(Engine& e, DevBuf& corr, DevBuf& part, size_t corr_bytes, size_t part_bytes) {
  if (corr_bytes > corr.cap || part_bytes > part.cap) APD_HIP(hipStreamSynchronize(e.stream));
  APD_TRY(corr.ensure(corr_bytes));
  return part.ensure(part_bytes);
}

void colmajor_to_rows12(const double* T16, double* r12) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) r12[4 * i + j] = T16[i + 4 * j];
}

// The head of a single handle's linearize at T (column-major 4x4) over `rows` rows of `noff` offsets: the frozen state is void until the
// mode says otherwise, its buffers sized (behind a wait when the indices or the block rows are replaced), the pose on the device.
int lin_begin(Engine& e, FrozenLin& f, int rows, int noff, const double* T16) {
  const int nblk = (rows + VG_BLK - 1) / VG_BLK;
  f.have = false;
  APD_TRY(ensure_corr_part(e, f.corr, f.part, (size_t)rows * noff * 4, (size_t)nblk * VG_RED * 8));
  APD_TRY(f.T.ensure(24 * sizeof(double)));
  APD_TRY(f.out.ensure(64 * sizeof(double)));
  f.rows = rows, f.noff = noff;
  colmajor_to_rows12(T16, f.T_lin);
  APD_HIP(hipMemcpyAsync(f.T.p, f.T_lin, 12 * sizeof(double), hipMemcpyHostToDevice, e.stream));
  return 0;
}

// The head of a single handle's compute_error at T (the caller has found the frozen state current): the new pose, then the pose of the linearize
int err_begin(Engine& e, const FrozenLin& f, const double* T16) {
  APD_HIP(hipSetDevice(e.device));
  double t24[24];
  colmajor_to_rows12(T16, t24);
  memcpy(t24 + 12, f.T_lin, 12 * sizeof(double));
  APD_HIP(hipMemcpyAsync(f.T.p, t24, sizeof(t24), hipMemcpyHostToDevice, e.stream));
  return 0;
}

// The body of the three apdgicp_*_get_correspondences (the caller has checked its mode and that the frozen state is its own and current):
// rows x noff voxel indices.  rows_msg: what the mode calls a wrong n_rows.  (No row: FAST_VGICP_CUDA without a kept source point.)
int read_frozen_corr(Engine& e, const FrozenLin& f, int32_t* voxel_index, int64_t n_rows, const char* rows_msg) {
  if (n_rows != f.rows) return fail(APDGICP_ERR_INVALID_ARG, rows_msg);
  if (f.rows == 0) return 0;
  APD_HIP(hipMemcpyAsync(voxel_index, f.corr.p, (size_t)n_rows * f.noff * 4, hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  return 0;
}

// The tail of a single handle's linearize (offset 0) and compute_error (offset 27): the block rows reduced, the 44 doubles read with a wait.
int reduce_and_read(Engine& e, const FrozenLin& f, int offset, double* H, double* b, double* cost, int* matched) {
  hipLaunchKernelGGL(k_vg_reduce, dim3(1), dim3(64), 0, e.stream, f.part.as<double>(), (f.rows + VG_BLK - 1) / VG_BLK, offset, f.out.as<double>());
  APD_HIP(hipGetLastError());
  APD_HIP(hipMemcpyAsync(e.h_probe.p, f.out.p, 44 * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  if (H && b) {
    memcpy(H, e.h_probe.p, 36 * sizeof(double));
    memcpy(b, e.h_probe.as<double>() + 36, 6 * sizeof(double));
  }
  if (cost) *cost = e.h_probe.as<double>()[42];
  if (matched) *matched = (int)std::min(e.h_probe.as<double>()[43], 2147483647.0);  // (apdgicp_result::n_matched is an int32: saturates, see the header)
  return 0;
}

// ---- voxelized GICP (include/apdgicp_hip.h V1 .. V7; kernels: apd_vgicp.hpp)
// V1 .. V3: the voxel map of the target.  Needs the target only; its covariances are computed here when they are missing.
int vg_build_map(apdgicp_handle* h) {
  Engine& e = h->eng;
  VgState& v = h->vg;
  if (e.clouds.size() < 2 || e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
  if (v.prm.voxel_mode == APDGICP_VGICP_MULTIPLICATIVE) return fail(APDGICP_ERR_UNSUPPORTED, "voxelized GICP: MULTIPLICATIVE accumulation is not offered");
  APD_TRY(e.compute_covariances({kTgt}));
  Engine::Cloud& c = e.clouds[kTgt];
  if (v.map_built && v.map_tgt_gen == h->cloud_gen[kTgt] && v.map_cov_gen == c.cov_gen && v.map_res == v.prm.resolution && v.map_mode == v.prm.voxel_mode) return 0;
  const int n = c.n;
  APD_HIP(hipSetDevice(e.device));
  v.map_built = h->lin.have = false;
  VoxSorted s;
  int nv = 0;
  APD_TRY(handle_sort_voxels(h, kTgt, v.prm.resolution, v.scal, "voxelized GICP: ", &s, &nv));
  APD_TRY(v.inv_t.ensure((size_t)n * 4));
  APD_TRY(v.buf.ensure((size_t)nv, false));
  hipLaunchKernelGGL(k_vg_inverse_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, c.perm.as<int>(), n, v.inv_t.as<int>());
  hipLaunchKernelGGL(k_vg_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, n, h->sort.bsum.as<int>(), c.opts.as<float4>(), c.cov.as<double>(), v.inv_t.as<int>(),
                     v.buf.vkeys.as<unsigned long long>(), v.buf.vcount.as<int>(), v.buf.vmean.as<double>(), v.buf.vcov.as<double>(), nv);
  APD_HIP(hipGetLastError());
  v.n_vox = nv;
  v.map_built = true, v.map_tgt_gen = h->cloud_gen[kTgt], v.map_cov_gen = c.cov_gen, v.map_res = v.prm.resolution, v.map_mode = v.prm.voxel_mode;
  v.builds++;
  return 0;
}

// the pair, the map and the source's inverse permutation: everything k_vg_linearize reads
int vg_prepare(apdgicp_handle* h) {
  Engine& e = h->eng;
  VgState& v = h->vg;
  APD_TRY(ensure_pair(h));  // (both clouds sorted, both covariances there)
  APD_TRY(vg_build_map(h));
  const Engine::Cloud& s = e.clouds[kSrc];
  if (!v.inv_s.p || v.inv_src_gen != h->cloud_gen[kSrc] || v.inv_n != s.n || (size_t)s.n * 4 > v.inv_s.cap) {
    v.inv_n = 0;
    if ((size_t)s.n * 4 > v.inv_s.cap) APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(v.inv_s.ensure((size_t)s.n * 4));
    hipLaunchKernelGGL(k_vg_inverse_perm, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, e.stream, s.perm.as<int>(), s.n, v.inv_s.as<int>());
    APD_HIP(hipGetLastError());
    v.inv_src_gen = h->cloud_gen[kSrc], v.inv_n = s.n;
  }
  return 0;
}

// linearize (V:119-180) at T (column-major 4x4)
int vg_linearize(apdgicp_handle* h, const double* T16, double* H, double* b, double* cost, int* matched) {
  APD_TRY(vg_prepare(h));
  Engine& e = h->eng;
  VgState& v = h->vg;
  FrozenLin& f = h->lin;
  const Engine::Cloud& s = e.clouds[kSrc];
  const int n = s.n, noff = n_offsets(v.prm.neighbor_search), nblk = (n + VG_BLK - 1) / VG_BLK;
  APD_TRY(lin_begin(e, f, n, noff, T16));
  const int want = H && b ? 1 : 0;
  hipLaunchKernelGGL(k_vg_linearize, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), s.cov.as<double>(), v.inv_s.as<int>(), n, v.map(), f.T.as<double>(),
                     v.prm.resolution, (int)v.prm.neighbor_search, noff, want, f.corr.as<int>(), f.part.as<double>());
  APD_TRY(reduce_and_read(e, f, 0, H, b, cost, matched));
  f.have = true;
  v.lin_src_gen = h->cloud_gen[kSrc], v.lin_src_cov_gen = s.cov_gen, v.lin_build = v.builds;
  return 0;
}

// compute_error (V:183-204): the voxel indices and the pose of the last linearize (V6)
int vg_error(apdgicp_handle* h, const double* T16, double* cost) {
  Engine& e = h->eng;
  VgState& v = h->vg;
  const FrozenLin& f = h->lin;
  if (e.clouds.size() < 2) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize");
  const Engine::Cloud &s = e.clouds[kSrc], &t = e.clouds[kTgt];
  // the frozen state must still describe what the handle holds: the same source points and covariances, the same map of the same target
  const bool frozen_ok = f.have && s.n > 0 && s.n == f.rows && s.cov_valid && v.lin_src_gen == h->cloud_gen[kSrc] && v.lin_src_cov_gen == s.cov_gen &&
                         v.inv_src_gen == h->cloud_gen[kSrc] && v.inv_n == s.n && v.map_built && v.lin_build == v.builds && t.cov_valid &&
                         v.map_tgt_gen == h->cloud_gen[kTgt] && v.map_cov_gen == t.cov_gen && v.map_res == v.prm.resolution && v.map_mode == v.prm.voxel_mode;
  if (!frozen_ok) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize of the clouds, covariances and voxel map the handle holds now");
  const int n = s.n, nblk = (n + VG_BLK - 1) / VG_BLK;
  APD_TRY(err_begin(e, f, T16));
  hipLaunchKernelGGL(k_vg_error, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), s.cov.as<double>(), v.inv_s.as<int>(), n, v.map(), f.T.as<double>(), f.noff,
                     f.corr.as<int>(), f.part.as<double>());
  return reduce_and_read(e, f, 27, nullptr, nullptr, cost, nullptr);
}

// The reference's own control flow (L:55-173) on the host over two callables: lin(T16, H, b, &y0, &matched) and err(T16, &yi), the two
// virtuals of LsqRegistration.  stop_on_empty (V7 of the voxelized mode): a linearize without a correspondence ends the loop.
template <typename Lin, typename Err>
int host_loop(apdgicp_handle* h, const float guess[16], apdgicp_result* out, Lin&& lin, Err&& err, bool stop_on_empty, double* final_H_out = nullptr) {
  Engine& e = h->eng;
  const apdgicp_params& p = e.params;
  float g[16];
  if (guess) memcpy(g, guess, sizeof(g));
  else identity16(g);
  Rigid x0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) x0.m[4 * i + j] = (double)g[i + 4 * j];  // L:56
  double lambda = -1.0;                                                   // L:58
  bool converged = false;
  int nr_iterations = 0, n_lin = 0, n_err = 0, failed = 0, matched = 0;
  double final_H[36];
  for (int q = 0; q < 36; q++) final_H[q] = (q % 7 == 0) ? 1.0 : 0.0;
  double y0 = 0.0;
  h->tr_lambda.clear(), h->tr_rho.clear(), h->tr_y0.clear(), h->tr_yi.clear(), h->tr_dnorm.clear(), h->tr_poses.clear();
  h->trace_from_host_loop = true;
  for (int it = 0; it < p.max_iterations && !converged; it++) {  // L:67
    nr_iterations = it;
    double T16[16], H[36], b[6], d[6];
    rigid_to_colmajor(x0, T16);
    APD_TRY(lin(T16, H, b, &y0, &matched));
    n_lin++;
    if (stop_on_empty && matched == 0) break;
    Rigid delta = rigid_identity();
    bool ok = false;
    if (p.optimizer == APDGICP_OPT_GN) {  // L:107-123
      solve6_spd(H, 0.0, b, d);
      delta = make_delta(d);
      x0 = rigid_mul(delta, x0);
      memcpy(final_H, H, sizeof(H));
      ok = true;
    } else {  // L:127-173
      if (lambda < 0.0) {
        double mx = 0.0;
        for (int q = 0; q < 6; q++) mx = std::max(mx, std::fabs(H[q + 6 * q]));
        lambda = p.lm_init_lambda_factor * mx;
      }
      double nu = 2.0;
      for (int in = 0; in < p.lm_max_iterations; in++) {
        solve6_spd(H, lambda, b, d);
        delta = make_delta(d);
        const Rigid xi = rigid_mul(delta, x0);
        double yi = 0.0;
        rigid_to_colmajor(xi, T16);
        APD_TRY(err(T16, &yi));
        n_err++;
        double den = 0.0;
        for (int q = 0; q < 6; q++) den += d[q] * (lambda * d[q] - b[q]);
        const double rho = (y0 - yi) / den;
        if (e.trace_on) {
          double nn = 0.0;
          for (int q = 0; q < 6; q++) nn += d[q] * d[q];
          h->tr_lambda.push_back(lambda), h->tr_rho.push_back(rho), h->tr_y0.push_back(y0), h->tr_yi.push_back(yi), h->tr_dnorm.push_back(std::sqrt(nn));
        }
        if (rho < 0) {
          if (is_converged(delta, p.rotation_epsilon, p.transformation_epsilon)) {
            ok = true;
            break;
          }
          lambda = nu * lambda;
          nu = 2 * nu;
          continue;
        }
        x0 = xi;
        const double t = 2 * rho - 1;
        lambda = lambda * std::max(1.0 / 3.0, 1 - t * t * t);
        memcpy(final_H, H, sizeof(H));
        ok = true;
        break;
      }
    }
    if (!ok) {
      failed = 1;
      break;
    }
    if (e.trace_on) {
      double P[16];
      rigid_to_colmajor(x0, P);
      h->tr_poses.insert(h->tr_poses.end(), P, P + 16);
    }
    converged = is_converged(delta, p.rotation_epsilon, p.transformation_epsilon);
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) out->T[i + 4 * j] = (float)x0.m[4 * i + j];
  out->T[3] = out->T[7] = out->T[11] = 0.f;
  out->T[15] = 1.f;
  out->final_cost = y0;
  out->converged = converged;
  out->iterations = nr_iterations;
  out->n_linearize = n_lin;
  out->n_compute_error = n_err;
  out->lm_failed = failed;
  out->n_matched = matched;
  h->have_corr = n_lin > 0;
  // keep getFinalHessian() coherent with this path (final_H_out: the caller keeps it on the host, there may be no pair state on the device)
  if (final_H_out) {
    memcpy(final_H_out, final_H, sizeof(final_H));
    return 0;
  }
  APD_HIP(hipMemcpyAsync((char*)e.d_state.p + offsetof(PairState, final_H), final_H, sizeof(final_H), hipMemcpyHostToDevice, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  return 0;
}

// The host loop of a voxel mode over its linearize and its compute_error: a linearize without a correspondence ends it (V7 / VC9 / N8).
// final_H_out: see host_loop.
using LinFn = int (*)(apdgicp_handle*, const double*, double*, double*, double*, int*);
using ErrFn = int (*)(apdgicp_handle*, const double*, double*);
int voxel_host_loop(apdgicp_handle* h, const float guess[16], apdgicp_result* out, LinFn lin, ErrFn err, double* final_H_out) {
  return host_loop(
      h, guess, out, [&](const double* T, double* H, double* b, double* y0, int* m) { return lin(h, T, H, b, y0, m); },
      [&](const double* T, double* yi) { return err(h, T, yi); }, true, final_H_out);
}

int vg_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  APD_TRY(vg_prepare(h));
  return voxel_host_loop(h, guess, out, vg_linearize, vg_error, nullptr);
}

// ---- FAST_VGICP_CUDA (include/apdgicp_hip.h VC1 .. VC10; kernels: apd_vgicp_cuda.hpp)
int check_vgicp_cuda_params(const apdgicp_vgicp_cuda_params* p) {
  if (!p) return 0;
  if (!(p->resolution > 0.0) || !std::isfinite(p->resolution)) return fail(APDGICP_ERR_INVALID_ARG, "FAST_VGICP_CUDA: the resolution must be finite and positive");
  if (p->neighbor_search < APDGICP_VGICP_DIRECT1 || p->neighbor_search > APDGICP_VGICP_CUDA_DIRECT_RADIUS)
    return fail(APDGICP_ERR_INVALID_ARG, "FAST_VGICP_CUDA: unknown neighbour search method");
  if (p->neighbor_search == APDGICP_VGICP_CUDA_DIRECT_RADIUS && !(std::isfinite(p->search_radius) && p->search_radius >= 0.0 && p->search_radius <= (double)VC_MAX_RADIUS))
    return fail(APDGICP_ERR_INVALID_ARG, "FAST_VGICP_CUDA: the DIRECT_RADIUS radius must be finite with 0 <= r <= 4 (voxels)");
  if (p->regularization == APDGICP_REG_NONE || p->regularization == APDGICP_REG_NORMALIZED_MIN_EIG)
    return fail(APDGICP_ERR_UNSUPPORTED, "FAST_VGICP_CUDA: NONE and NORMALIZED_MIN_EIG are unimplemented in the reference (it goes on with raw covariances) and not offered");
  if (p->regularization != APDGICP_REG_MIN_EIG && p->regularization != APDGICP_REG_PLANE && p->regularization != APDGICP_REG_FROBENIUS)
    return fail(APDGICP_ERR_INVALID_ARG, "FAST_VGICP_CUDA: unknown regularization method");
  if (p->nn_method == APDGICP_NN_GPU_RBF_KERNEL) return fail(APDGICP_ERR_UNSUPPORTED, "FAST_VGICP_CUDA: GPU_RBF_KERNEL covariances are not offered");
  if (p->nn_method != APDGICP_NN_CPU_PARALLEL_KDTREE && p->nn_method != APDGICP_NN_GPU_BRUTEFORCE)
    return fail(APDGICP_ERR_INVALID_ARG, "FAST_VGICP_CUDA: unknown nearest neighbour method");
  return 0;
}

// One cloud of a preparation: its index in the engine's cloud list, where the prepared cloud goes, the device word that takes its kept count.
struct VcJob {
  int cloud;
  VcPrepared* pc;
  int* total;
};

// VC1 .. VC4 of every listed cloud (sorted, its descriptor uploaded, VC_K points or more), enqueued on the engine's stream with no wait in
// between: the slot in the grid, the queries per wave by the points of all of them (as Engine::launch_knn).  A buffer that exists and is too
// small may still be read by what is enqueued, so the stream is waited for once before one goes (*waited).  Reading the kept counts and the
// k-NN error flag back, and marking the clouds ready, is the caller's: each handle kind has its own pinned words and its own count of waits.
int vc_enqueue_prepare(Engine& e, const std::vector<VcJob>& jobs, int regularization, CachedTable& d_tab, CachedTable& d_ids, bool* waited) {
  const int count = (int)jobs.size();
  bool replaces = false;
  int nmax = 0;
  long long total = 0;
  for (const VcJob& j : jobs) {
    const VcPrepared& pc = *j.pc;
    const size_t n = (size_t)e.clouds[j.cloud].n, nb = (n + VC_BLK - 1) / VC_BLK;
    auto small = [](const DevBuf& d, size_t bytes) { return d.cap != 0 && bytes > d.cap; };
    replaces |= small(pc.raw, n * 48) || small(pc.reg6, n * 48) || small(pc.flag, n) || small(pc.bsum, nb * 4) || small(pc.kpts, n * 16) || small(pc.kcov, n * 48) ||
                small(pc.kept, n * 4) || small(pc.ident, n * 4);
    nmax = std::max(nmax, e.clouds[j.cloud].n), total += e.clouds[j.cloud].n;
  }
  *waited = replaces;
  if (replaces) APD_HIP(hipStreamSynchronize(e.stream));
  std::vector<VcbSlot> tab((size_t)count);
  std::vector<int> ids((size_t)count);
  for (int q = 0; q < count; q++) {
    VcPrepared& pc = *jobs[q].pc;
    const size_t n = (size_t)e.clouds[jobs[q].cloud].n, nb = (n + VC_BLK - 1) / VC_BLK;
    pc.ready = false;
    APD_TRY(pc.raw.ensure(n * 48));
    APD_TRY(pc.reg6.ensure(n * 48));
    APD_TRY(pc.flag.ensure(n));
    APD_TRY(pc.bsum.ensure(nb * 4));
    APD_TRY(pc.kpts.ensure(n * 16));  // (the buffers behind the compaction are sized for n kept points -- the count is not known yet)
    APD_TRY(pc.kcov.ensure(n * 48));
    APD_TRY(pc.kept.ensure(n * 4));
    APD_TRY(pc.ident.ensure(n * 4));
    tab[q] = VcbSlot{e.clouds[jobs[q].cloud].opts.as<float4>(), pc.raw.as<double>(), pc.reg6.as<double>(), pc.flag.as<unsigned char>(), pc.bsum.as<int>(), jobs[q].total,
                     pc.kpts.as<float4>(), pc.kcov.as<double>(), pc.kept.as<int>(), pc.ident.as<int>(), (int)n, 0};
    ids[q] = jobs[q].cloud;
  }
  APD_TRY(d_tab.upload(tab.data(), tab.size() * sizeof(VcbSlot), e.stream));
  APD_TRY(d_ids.upload(ids.data(), ids.size() * sizeof(int), e.stream));
  const CloudDesc* desc = e.d_desc.as<CloudDesc>();
  const VcbSlot* dt = d_tab.as<VcbSlot>();
  int* eflag = e.d_errflag.as<int>();
  unsigned long long* stats = e.d_stats.as<unsigned long long>();
  const int qpw = total >= 100000 ? 16 : total >= 40000 ? 8 : 4;
  const dim3 kgrid((unsigned)((nmax + qpw - 1) / qpw), (unsigned)count), bgrid((unsigned)((nmax + VC_BLK - 1) / VC_BLK), (unsigned)count);
  if (qpw == 16) hipLaunchKernelGGL(k_vcb_knn_raw<4>, kgrid, dim3(64), knn_coop_lds_bytes(qpw), e.stream, desc, d_ids.as<int>(), dt, VC_K, eflag, stats);
  else if (qpw == 8) hipLaunchKernelGGL(k_vcb_knn_raw<8>, kgrid, dim3(64), knn_coop_lds_bytes(qpw), e.stream, desc, d_ids.as<int>(), dt, VC_K, eflag, stats);
  else hipLaunchKernelGGL(k_vcb_knn_raw<16>, kgrid, dim3(64), knn_coop_lds_bytes(qpw), e.stream, desc, d_ids.as<int>(), dt, VC_K, eflag, stats);
  hipLaunchKernelGGL(k_vcb_regularize, bgrid, dim3(VC_BLK), 0, e.stream, dt, regularization);
  hipLaunchKernelGGL(k_vcb_scan, dim3((unsigned)count), dim3(SCAN_BLK), 0, e.stream, dt);
  hipLaunchKernelGGL(k_vcb_scatter, bgrid, dim3(VC_BLK), 0, e.stream, dt);
  APD_HIP(hipGetLastError());
  return 0;
}

// the k-NN error flag a preparation's read-back brought home
int vc_knn_flag_error(Engine& e, int flag) {
  APD_HIP(hipMemsetAsync(e.d_errflag.p, 0, sizeof(int), e.stream));
  return fail(APDGICP_ERR_INTERNAL, "FAST_VGICP_CUDA k-NN: " + Engine::errflag_text(flag));
}

// VC4 for the getters: the kept count of a prepared cloud and, with kept_index given, the original indices
int read_kept(hipStream_t stream, const VcPrepared& pc, int64_t* n_kept, int32_t* kept_index, int64_t capacity) {
  *n_kept = pc.n_kept;
  if (!kept_index || pc.n_kept == 0) return 0;
  if (capacity < pc.n_kept) return fail(APDGICP_ERR_INVALID_ARG, "capacity is below the kept count");
  APD_HIP(hipMemcpyAsync(kept_index, pc.kept.p, (size_t)pc.n_kept * 4, hipMemcpyDeviceToHost, stream));
  APD_HIP(hipStreamSynchronize(stream));
  return 0;
}

// VC2 / VC3 for the getters: per kept point the raw covariance (6 doubles) and the regularised one (9), either may be null
int read_prepared_covariances(hipStream_t stream, const VcPrepared& pc, double* raw_n6, double* reg_n9, int64_t capacity) {
  const int64_t nk = pc.n_kept;
  if (capacity < nk) return fail(APDGICP_ERR_INVALID_ARG, "capacity is below the kept count");
  if (nk == 0) return 0;
  std::vector<double> all(raw_n6 ? (size_t)pc.n * 6 : 0), k6(reg_n9 ? (size_t)nk * 6 : 0);
  std::vector<int> kept(raw_n6 ? (size_t)nk : 0);
  if (raw_n6) {
    APD_HIP(hipMemcpyAsync(all.data(), pc.raw.p, all.size() * 8, hipMemcpyDeviceToHost, stream));
    APD_HIP(hipMemcpyAsync(kept.data(), pc.kept.p, kept.size() * 4, hipMemcpyDeviceToHost, stream));
  }
  if (reg_n9) APD_HIP(hipMemcpyAsync(k6.data(), pc.kcov.p, k6.size() * 8, hipMemcpyDeviceToHost, stream));
  APD_HIP(hipStreamSynchronize(stream));
  for (int64_t j = 0; j < nk && raw_n6; j++) {
    if (kept[j] < 0 || kept[j] >= pc.n) return fail(APDGICP_ERR_INTERNAL, "FAST_VGICP_CUDA: inconsistent kept index");
    memcpy(raw_n6 + 6 * j, &all[6 * (size_t)kept[j]], 6 * sizeof(double));
  }
  for (int64_t j = 0; j < nk && reg_n9; j++) {  // kcov: [6][n_kept]
    const double xx = k6[j], xy = k6[nk + j], xz = k6[2 * nk + j], yy = k6[3 * nk + j], yz = k6[4 * nk + j], zz = k6[5 * nk + j];
    double* o = reg_n9 + 9 * j;
    o[0] = xx, o[1] = xy, o[2] = xz, o[3] = xy, o[4] = yy, o[5] = yz, o[6] = xz, o[7] = yz, o[8] = zz;
  }
  return 0;
}

// VC1 .. VC4: the prepared cloud `which`.  One wait: the kept count and the error flag come back together.
int vc_prepare_cloud(apdgicp_handle* h, int which) {
  Engine& e = h->eng;
  VcState& v = h->vc;
  if (e.clouds.size() < 2 || e.clouds[which].n <= 0) return fail(APDGICP_ERR_NO_INPUT, std::string(cloud_name(which)) + " cloud is not set");
  VcPrepared& pc = v.pc[which];
  if (pc.ready && pc.pts_gen == h->cloud_gen[which] && pc.reg == v.prm.regularization) return 0;
  const int n = e.clouds[which].n;
  if (n < VC_K) return fail(APDGICP_ERR_TOO_FEW_POINTS, "cloud has fewer points than k_correspondences");
  APD_HIP(hipSetDevice(e.device));
  APD_TRY(e.upload_desc());  // (sorts what is not sorted yet)
  h->lin.have = false;
  APD_TRY(v.scal.ensure(32));
  int* d_total = v.scal.as<int>() + 4 + which;
  bool waited = false;
  APD_TRY(vc_enqueue_prepare(e, {VcJob{which, &pc, d_total}}, v.prm.regularization, v.prep_tab[which], v.prep_ids[which], &waited));
  int* hw = e.h_probe.as<int>();
  APD_HIP(hipMemcpyAsync(hw, d_total, sizeof(int), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipMemcpyAsync(hw + 1, e.d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  if (hw[1]) return vc_knn_flag_error(e, hw[1]);
  if (hw[0] < 0 || hw[0] > n) return fail(APDGICP_ERR_INTERNAL, "FAST_VGICP_CUDA: inconsistent kept count");
  pc.n = n, pc.n_kept = hw[0];
  pc.pts_gen = h->cloud_gen[which], pc.reg = v.prm.regularization, pc.id = ++v.preps;
  pc.ready = true;
  return 0;
}

// VC5: the voxel map of the prepared target
int vc_build_map(apdgicp_handle* h) {
  Engine& e = h->eng;
  VcState& v = h->vc;
  APD_TRY(vc_prepare_cloud(h, kTgt));
  const VcPrepared& t = v.pc[kTgt];
  if (v.map_built && v.map_prep_id == t.id && v.map_res == v.prm.resolution) return 0;
  v.map_built = h->lin.have = false;
  int nv = 0;
  if (t.n_kept > 0) {  // (no kept point: an empty map, no sort)
    const int n = t.n_kept;
    VoxSorted s;
    auto point_name = [&](int j) {  // VC4: the message names the point by its index in the caller's cloud (an error path: its own wait)
      int orig = -1;
      if (j >= 0 && j < n && hipMemcpy(&orig, t.kept.as<int>() + j, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) orig = -1;
      return "target point " + std::to_string(orig);
    };
    APD_TRY(handle_sort_voxels(h, t.kpts.as<float4>(), n, v.prm.resolution, v.scal, "FAST_VGICP_CUDA: ", point_name, &s, &nv));
    APD_TRY(v.buf.ensure((size_t)nv, false));
    hipLaunchKernelGGL(k_vg_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, n, h->sort.bsum.as<int>(), t.kpts.as<float4>(), t.kcov.as<double>(), t.ident.as<int>(),
                       v.buf.vkeys.as<unsigned long long>(), v.buf.vcount.as<int>(), v.buf.vmean.as<double>(), v.buf.vcov.as<double>(), nv);
    APD_HIP(hipGetLastError());
  }
  v.n_vox = nv;
  v.map_built = true, v.map_prep_id = t.id, v.map_res = v.prm.resolution;
  v.builds++;
  return 0;
}

// both prepared clouds, the map and the offset table: everything k_vc_linearize reads
int vc_prepare(apdgicp_handle* h) {
  APD_TRY(vc_prepare_cloud(h, kSrc));
  APD_TRY(vc_build_map(h));
  return h->vc.offs.ensure(h->vc.prm, h->eng.stream);
}

int vc_linearize(apdgicp_handle* h, const double* T16, double* H, double* b, double* cost, int* matched) {
  APD_TRY(vc_prepare(h));
  Engine& e = h->eng;
  VcState& v = h->vc;
  FrozenLin& f = h->lin;
  const VcPrepared& s = v.pc[kSrc];
  const int n = s.n_kept, noff = v.offs.count(), nblk = (n + VG_BLK - 1) / VG_BLK;
  APD_TRY(lin_begin(e, f, n, noff, T16));
  const int want = H && b ? 1 : 0;
  if (nblk > 0)
    hipLaunchKernelGGL(k_vc_linearize, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.kpts.as<float4>(), s.kcov.as<double>(), s.ident.as<int>(), n, v.map(), f.T.as<double>(),
                       v.prm.resolution, v.offs.dev.as<int>(), noff, want, f.corr.as<int>(), f.part.as<double>());
  APD_TRY(reduce_and_read(e, f, 0, H, b, cost, matched));  // (no kept source point: no block rows, every sum 0)
  f.have = true;
  v.lin_src_id = s.id, v.lin_build = v.builds;
  return 0;
}

// VC8: the frozen state must still describe what the handle holds
bool vc_frozen_ok(const apdgicp_handle* h) {
  const VcState& v = h->vc;
  const VcPrepared &s = v.pc[kSrc], &t = v.pc[kTgt];
  return h->lin.have && s.ready && s.pts_gen == h->cloud_gen[kSrc] && s.reg == v.prm.regularization && s.id == v.lin_src_id && s.n_kept == h->lin.rows && t.ready &&
         t.pts_gen == h->cloud_gen[kTgt] && t.reg == v.prm.regularization && v.map_built && v.map_prep_id == t.id && v.map_res == v.prm.resolution && v.lin_build == v.builds;
}

int vc_error(apdgicp_handle* h, const double* T16, double* cost) {
  Engine& e = h->eng;
  VcState& v = h->vc;
  const FrozenLin& f = h->lin;
  if (!vc_frozen_ok(h)) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize of the clouds, regularisation and voxel map the handle holds now");
  const VcPrepared& s = v.pc[kSrc];
  const int n = s.n_kept, nblk = (n + VG_BLK - 1) / VG_BLK;
  APD_TRY(err_begin(e, f, T16));
  if (nblk > 0)
    hipLaunchKernelGGL(k_vg_error, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.kpts.as<float4>(), s.kcov.as<double>(), s.ident.as<int>(), n, v.map(), f.T.as<double>(), f.noff,
                       f.corr.as<int>(), f.part.as<double>());
  return reduce_and_read(e, f, 27, nullptr, nullptr, cost, nullptr);
}

int vc_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  APD_TRY(vc_prepare(h));
  return voxel_host_loop(h, guess, out, vc_linearize, vc_error, h->final_H);
}

// ---- NDT (include/apdgicp_hip.h N1 .. N9; kernels: apd_ndt.hpp)
// N1 .. N4: the voxel map of one cloud.  Needs that cloud's points only: no covariances, any size.
int nd_build_map(apdgicp_handle* h, int which) {
  Engine& e = h->eng;
  NdState& v = h->nd;
  if (e.clouds.size() < 2 || e.clouds[which].n <= 0) return fail(APDGICP_ERR_NO_INPUT, std::string(cloud_name(which)) + " cloud is not set");
  NdState::Map& m = v.maps[which];
  if (m.built && m.pts_gen == h->cloud_gen[which] && m.res == v.prm.resolution) return 0;
  APD_HIP(hipSetDevice(e.device));
  APD_TRY(e.upload_desc());  // (sorts what is not sorted yet: a staged cloud's opts are written by its sort)
  Engine::Cloud& c = e.clouds[which];
  m.built = false;
  h->lin.have = false;
  VoxSorted s;
  int nv = 0;
  APD_TRY(handle_sort_voxels(h, which, v.prm.resolution, v.scal, "NDT: ", &s, &nv));
  APD_TRY(m.buf.ensure((size_t)nv, true));
  hipLaunchKernelGGL(k_ndt_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, c.n, h->sort.bsum.as<int>(), c.opts.as<float4>(), m.buf.vkeys.as<unsigned long long>(),
                     m.buf.vcount.as<int>(), m.buf.vmean.as<double>(), m.buf.vraw.as<double>(), m.buf.vcov.as<double>(), nv);
  APD_HIP(hipGetLastError());
  m.nv = nv;
  m.built = true, m.pts_gen = h->cloud_gen[which], m.res = v.prm.resolution;
  m.id = ++v.builds;
  return 0;
}

// both clouds in caller's order on the device and the maps the mode needs (N4): everything k_ndt_linearize reads
int nd_prepare(apdgicp_handle* h) {
  Engine& e = h->eng;
  if (e.clouds.size() < 2 || e.clouds[kSrc].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "source cloud is not set");
  if (e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
  APD_HIP(hipSetDevice(e.device));
  APD_TRY(e.upload_desc());
  APD_TRY(nd_build_map(h, kTgt));
  if (h->nd.prm.distance_mode == APDGICP_NDT_D2D) APD_TRY(nd_build_map(h, kSrc));
  return 0;
}

// linearize (NC:137-160) at T (column-major 4x4)
int nd_linearize(apdgicp_handle* h, const double* T16, double* H, double* b, double* cost, int* matched) {
  APD_TRY(nd_prepare(h));
  Engine& e = h->eng;
  NdState& v = h->nd;
  FrozenLin& f = h->lin;
  const Engine::Cloud& s = e.clouds[kSrc];
  const bool d2d = v.prm.distance_mode == APDGICP_NDT_D2D;
  const NdState::Map &mt = v.maps[kTgt], &ms = v.maps[kSrc];
  const int nrows = d2d ? ms.nv : s.n, noff = n_offsets(v.prm.neighbor_search), nblk = (nrows + VG_BLK - 1) / VG_BLK;
  APD_TRY(lin_begin(e, f, nrows, noff, T16));
  const int want = H && b ? 1 : 0;
  const VgMap smap = d2d ? ms.map() : VgMap{nullptr, nullptr, nullptr, nullptr, 0};
  if (d2d)
    hipLaunchKernelGGL(k_ndt_linearize<true>, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), smap, nrows, mt.map(), f.T.as<double>(), v.prm.resolution,
                       (int)v.prm.neighbor_search, noff, want, f.corr.as<int>(), f.part.as<double>());
  else
    hipLaunchKernelGGL(k_ndt_linearize<false>, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), smap, nrows, mt.map(), f.T.as<double>(), v.prm.resolution,
                       (int)v.prm.neighbor_search, noff, want, f.corr.as<int>(), f.part.as<double>());
  APD_TRY(reduce_and_read(e, f, 0, H, b, cost, matched));
  f.have = true, v.lin_mode = v.prm.distance_mode;
  v.lin_src_gen = h->cloud_gen[kSrc], v.lin_tgt_id = mt.id, v.lin_src_id = d2d ? ms.id : 0;
  return 0;
}

// compute_error (NC:162-177): the voxel indices and R_lin of the last linearize (N7)
int nd_error(apdgicp_handle* h, const double* T16, double* cost) {
  Engine& e = h->eng;
  NdState& v = h->nd;
  const FrozenLin& f = h->lin;
  if (e.clouds.size() < 2) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize");
  const Engine::Cloud& s = e.clouds[kSrc];
  const bool d2d = v.prm.distance_mode == APDGICP_NDT_D2D;
  const NdState::Map &mt = v.maps[kTgt], &ms = v.maps[kSrc];
  // the frozen state must still describe what the handle holds: the same source points, the same maps, the same mode and resolution
  const bool frozen_ok = f.have && s.n > 0 && v.lin_src_gen == h->cloud_gen[kSrc] && v.lin_mode == v.prm.distance_mode && mt.built && mt.id == v.lin_tgt_id &&
                         mt.pts_gen == h->cloud_gen[kTgt] && mt.res == v.prm.resolution && e.clouds[kTgt].n > 0 &&
                         (d2d ? (ms.built && ms.id == v.lin_src_id && ms.pts_gen == h->cloud_gen[kSrc] && ms.res == v.prm.resolution && ms.nv == f.rows)
                              : s.n == f.rows);
  if (!frozen_ok) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize of the clouds and voxel maps the handle holds now");
  const int nrows = f.rows, nblk = (nrows + VG_BLK - 1) / VG_BLK;
  APD_TRY(err_begin(e, f, T16));
  const VgMap smap = d2d ? ms.map() : VgMap{nullptr, nullptr, nullptr, nullptr, 0};
  if (d2d)
    hipLaunchKernelGGL(k_ndt_error<true>, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), smap, nrows, mt.map(), f.T.as<double>(), v.prm.resolution, f.noff,
                       f.corr.as<int>(), f.part.as<double>());
  else
    hipLaunchKernelGGL(k_ndt_error<false>, dim3(nblk), dim3(VG_BLK), 0, e.stream, s.opts.as<float4>(), smap, nrows, mt.map(), f.T.as<double>(), v.prm.resolution, f.noff,
                       f.corr.as<int>(), f.part.as<double>());
  return reduce_and_read(e, f, 27, nullptr, nullptr, cost, nullptr);
}

int nd_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  APD_TRY(nd_prepare(h));
  h->reset_final_H();
  const int rc = voxel_host_loop(h, guess, out, nd_linearize, nd_error, h->final_H);
  h->have_corr = false;  // (the APD kernels' correspondences are not what this mode wrote)
  return rc;
}

// ---- point-to-point ICP (include/apdgicp_hip.h IC1 .. IC10; kernels: apd_icp.hpp)
bool is_identity16(const float* T) {
  for (int q = 0; q < 16; q++)
    if (T[q] != ((q % 5 == 0) ? 1.f : 0.f)) return false;
  return true;
}

// Both clouds sorted, the engine's one-pair search set up with W in place of the sorted source at the identity pose, W0 = T * source
// written, the record started at `final0`.  The handle's own pair is set up again by whoever needs it next.
int ic_begin(apdgicp_handle* h, const float* T16, const float* final0) {
  Engine& e = h->eng;
  IcState& v = h->ic;
  v.have = false;
  h->pair_ready = false;  // (a pair table left by an earlier call may name a W that is replaced below)
  APD_TRY(ensure_pair(h));
  const Engine::Cloud& s = e.clouds[kSrc];
  const int n = s.n, nblk = (n + IC_BLK - 1) / IC_BLK;
  const size_t nch = ((size_t)n + kChunk - 1) / kChunk, ngr = ((size_t)n + kGroupPts - 1) / kGroupPts;
  if ((size_t)n * 16 > v.W.cap || nch * sizeof(Box) > v.cbox.cap || ngr * sizeof(Box) > v.gbox.cap || (size_t)n > v.beaten.cap || (size_t)n * 4 > v.match.cap ||
      (size_t)n * 4 > v.dsq.cap || (size_t)nblk * IC_R2 * 8 > v.part.cap)
    APD_HIP(hipStreamSynchronize(e.stream));
  APD_TRY(v.W.ensure((size_t)n * 16));
  APD_TRY(v.cbox.ensure(nch * sizeof(Box)));
  APD_TRY(v.gbox.ensure(ngr * sizeof(Box)));
  APD_TRY(v.beaten.ensure((size_t)n));
  APD_TRY(v.match.ensure((size_t)n * 4));
  APD_TRY(v.dsq.ensure((size_t)n * 4));
  APD_TRY(v.part.ensure((size_t)nblk * IC_R2 * 8));
  APD_TRY(v.sum1.ensure(IC_R1 * 8));
  APD_TRY(v.rec.ensure(sizeof(IcpRecord)));
  APD_TRY(v.dT.ensure(16 * sizeof(float)));
  APD_TRY(v.h_rec.ensure(sizeof(IcpRecord)));
  PairDesc pd = e.h_pairs[0];
  pd.s.pts = v.W.as<float4>();
  APD_TRY(e.d_pairs.upload(&pd, sizeof(pd), e.stream));
  h->pair_ready = false, h->have_corr = false;
  const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  APD_HIP(hipMemcpyAsync(e.d_T.p, I16, sizeof(I16), hipMemcpyHostToDevice, e.stream));
  hipLaunchKernelGGL(k_set_probe, dim3(1), dim3(1), 0, e.stream, e.d_state.as<PairState>(), e.d_T.as<double>(), (int)ST_NEED_LIN, 0);  // (n_lin = 0: every search is cold)
  IcpRecord r0;
  memset(&r0, 0, sizeof(r0));
  for (int q = 0; q < 16; q++) r0.T_k[q] = (q % 5 == 0) ? 1.f : 0.f;
  memcpy(r0.final_T, final0, sizeof(r0.final_T));
  r0.prev_mse = std::numeric_limits<double>::max();
  APD_HIP(hipMemcpyAsync(v.rec.p, &r0, sizeof(r0), hipMemcpyHostToDevice, e.stream));  // (pageable source: staged before the call returns)
  const bool ident = is_identity16(T16);
  if (!ident) APD_HIP(hipMemcpyAsync(v.dT.p, T16, 16 * sizeof(float), hipMemcpyHostToDevice, e.stream));
  hipLaunchKernelGGL(k_icp_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, s.pts.as<float4>(), n, ident ? nullptr : v.dT.as<float>(),
                     (e.params.flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0, v.W.as<float4>());
  APD_HIP(hipGetLastError());
  v.launches += 2;
  return 0;
}

IcpConsts ic_consts(const apdgicp_params& p, const apdgicp_icp_params& q, int accumulate) {
  IcpConsts c;
  c.thr2 = p.max_correspondence_distance * p.max_correspondence_distance;
  c.trans_eps = p.transformation_epsilon;
  c.rot_thr = q.rotation_epsilon > 0.0 ? q.rotation_epsilon : 1.0 - p.transformation_epsilon;
  c.mse_abs = q.mse_threshold_absolute, c.mse_rel = q.euclidean_fitness_epsilon;
  c.max_iterations = p.max_iterations, c.min_corr = q.min_correspondences, c.max_similar = q.max_similar_transforms, c.accumulate = accumulate;
  return c;
}
IcpConsts ic_consts(const apdgicp_handle* h, int accumulate) { return ic_consts(h->eng.params, h->ic.prm, accumulate); }

// IC2 .. IC7 over the W that is there: the searches, the two reduction passes, the step; the record comes home behind ONE wait
int ic_iteration(apdgicp_handle* h, const IcpConsts& c) {
  Engine& e = h->eng;
  IcState& v = h->ic;
  const Engine::Cloud &s = e.clouds[kSrc];
  const int n = s.n, nblk = (n + IC_BLK - 1) / IC_BLK;
  float4* W = v.W.as<float4>();
  APD_TRY(e.launch_nn(e.whole()));
  APD_TRY(e.launch_linearize(e.whole(), 0));  // (the per-point pass that settles the exact index: Work::nnpt, Work::sqd)
  v.launches += 2;
  const bool recip = v.prm.use_reciprocal_correspondences != 0;
  if (recip) {
    const int nch = (n + kChunk - 1) / kChunk, ngr = (n + kGroupPts - 1) / kGroupPts;
    if (!v.brute) {
      hipLaunchKernelGGL(k_boxes, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, e.stream, W, n, (int)kChunk, v.cbox.as<Box>(), nch);
      hipLaunchKernelGGL(k_boxes, dim3((unsigned)((ngr + 255) / 256)), dim3(256), 0, e.stream, W, n, (int)kGroupPts, v.gbox.as<Box>(), ngr);
      hipLaunchKernelGGL(k_icp_recip<true>, dim3((unsigned)nblk), dim3(IC_BLK), 0, e.stream, W, n, s.perm.as<int>(), v.cbox.as<Box>(), v.gbox.as<Box>(), e.work.nnpt,
                         e.work.sqd, c.thr2, v.beaten.as<unsigned char>());
      v.launches += 3;
    } else {
      hipLaunchKernelGGL(k_icp_recip<false>, dim3((unsigned)nblk), dim3(IC_BLK), 0, e.stream, W, n, s.perm.as<int>(), v.cbox.as<Box>(), v.gbox.as<Box>(), e.work.nnpt,
                         e.work.sqd, c.thr2, v.beaten.as<unsigned char>());
      v.launches += 1;
    }
  }
  hipLaunchKernelGGL(k_icp_pairs, dim3((unsigned)nblk), dim3(IC_BLK), 0, e.stream, W, n, e.work.nnpt, e.work.sqd, recip ? v.beaten.as<unsigned char>() : nullptr, c.thr2,
                     v.match.as<int>(), v.dsq.as<float>(), v.part.as<double>());
  hipLaunchKernelGGL(k_icp_sums, dim3(1), dim3(64), 0, e.stream, v.part.as<double>(), nblk, (int)IC_R1, v.sum1.as<double>());
  hipLaunchKernelGGL(k_icp_cross, dim3((unsigned)nblk), dim3(IC_BLK), 0, e.stream, W, n, e.work.nnpt, v.match.as<int>(), v.sum1.as<double>(), v.part.as<double>());
  hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(64), 0, e.stream, v.part.as<double>(), nblk, v.sum1.as<double>(), v.rec.as<IcpRecord>(), c);
  APD_HIP(hipGetLastError());
  v.launches += 4;
  APD_HIP(hipMemcpyAsync(v.h_rec.p, v.rec.p, sizeof(IcpRecord), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  v.waits += 1;
  return 0;
}

void ic_mark_have(apdgicp_handle* h) {
  IcState& v = h->ic;
  v.have = true, v.have_src_gen = h->cloud_gen[kSrc], v.have_tgt_gen = h->cloud_gen[kTgt], v.n_have = h->eng.clouds[kSrc].n;
}

int ic_estimate(apdgicp_handle* h, const float T[16], float T_out[16], int64_t* n_corr, double* mse, double sums[16]) {
  float I[16];
  identity16(I);
  APD_TRY(ic_begin(h, T, I));
  APD_TRY(ic_iteration(h, ic_consts(h, 0)));
  const IcpRecord& r = *h->ic.h_rec.as<IcpRecord>();
  if (T_out) memcpy(T_out, r.T_k, sizeof(r.T_k));
  if (n_corr) *n_corr = r.n_corr;
  if (mse) *mse = r.mse;
  if (sums) memcpy(sums, r.sums, sizeof(r.sums));
  ic_mark_have(h);
  return 0;
}

int ic_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  Engine& e = h->eng;
  IcState& v = h->ic;
  float g[16];
  if (guess) memcpy(g, guess, sizeof(g));
  else identity16(g);
  v.tr_T.clear(), v.tr_n.clear(), v.tr_mse.clear(), v.tr_sim.clear();
  v.launches = v.waits = 0;
  v.state = APDGICP_ICP_NOT_CONVERGED;
  APD_TRY(ic_begin(h, g, g));
  const IcpConsts c = ic_consts(h, 1);
  const int n = e.clouds[kSrc].n, xf = (e.params.flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0;
  const IcpRecord& r = *v.h_rec.as<IcpRecord>();
  for (;;) {
    APD_TRY(ic_iteration(h, c));
    v.tr_T.insert(v.tr_T.end(), r.T_k, r.T_k + 16);
    v.tr_n.push_back(r.n_corr), v.tr_mse.push_back(r.mse), v.tr_sim.push_back(r.similar);
    if (r.estimated) {  // IC1: W = T_k * W, T_k read from the device record (after the last iteration too: W ends as PCL's output cloud)
      hipLaunchKernelGGL(k_icp_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, v.W.as<float4>(), n, v.rec.as<IcpRecord>(), xf);
      APD_HIP(hipGetLastError());
      v.launches += 1;
    }
    if (r.stop) break;
  }
  APD_HIP(hipStreamSynchronize(e.stream));
  v.state = r.state;
  memcpy(out->T, r.final_T, sizeof(out->T));
  out->final_cost = r.mse;
  out->converged = r.converged;
  out->iterations = r.iterations;
  out->n_linearize = r.iterations;
  out->n_compute_error = 0;
  out->lm_failed = 0;
  out->n_matched = (int)std::min<long long>(r.n_corr, 2147483647ll);
  h->trace_from_host_loop = true;  // (apdgicp_get_trace: this align left no optimiser trace)
  h->tr_lambda.clear(), h->tr_rho.clear(), h->tr_y0.clear(), h->tr_yi.clear(), h->tr_dnorm.clear(), h->tr_poses.clear();
  ic_mark_have(h);
  return 0;
}

// ---- FastGICPMultiPoints (include/apdgicp_hip.h MP1 .. MP11; kernels: apd_gicp_mp.hpp over apd_search.hpp)
int check_gicp_mp_params(const apdgicp_gicp_mp_params* p) {
  if (!p) return 0;
  if (!std::isfinite(p->neighbor_search_radius) || !(p->neighbor_search_radius > 0.0))
    return fail(APDGICP_ERR_INVALID_ARG, "FastGICPMultiPoints: neighbor_search_radius must be finite and positive");
  return 0;
}

// MP1: the regularisations whose result does not depend on the scale of the scatter matrix
int mp_check_regularization(const apdgicp_handle* h) {
  const int r = h->eng.params.regularization;
  if (r != APDGICP_REG_PLANE && r != APDGICP_REG_NORMALIZED_MIN_EIG)
    return fail(APDGICP_ERR_UNSUPPORTED, "FastGICPMultiPoints: only PLANE and NORMALIZED_MIN_EIG are offered (MIN_EIG and FROBENIUS act on the undivided scatter matrix there, NONE aborts)");
  return 0;
}

// both clouds sorted, both covariances there, the target's inverse permutation
int mp_prepare(apdgicp_handle* h) {
  Engine& e = h->eng;
  MpState& v = h->mp;
  APD_TRY(mp_check_regularization(h));
  if (e.clouds.size() < 2 || e.clouds[kSrc].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "source cloud is not set");
  if (e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
  for (int which : {kSrc, kTgt})
    if (e.clouds[which].n < e.params.k_correspondences)
      return fail(APDGICP_ERR_TOO_FEW_POINTS, std::string("FastGICPMultiPoints: the ") + cloud_name(which) + " cloud has fewer points than k_correspondences");
  APD_TRY(ensure_pair(h));
  APD_HIP(hipSetDevice(e.device));
  const Engine::Cloud& t = e.clouds[kTgt];
  if (!v.inv_t.p || v.inv_tgt_gen != h->cloud_gen[kTgt] || v.inv_n != t.n || (size_t)t.n * 4 > v.inv_t.cap) {
    v.inv_n = 0;
    APD_TRY(v.inv_t.ensure((size_t)t.n * 4));
    hipLaunchKernelGGL(k_vg_inverse_perm, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, e.stream, t.perm.as<int>(), t.n, v.inv_t.as<int>());
    APD_HIP(hipGetLastError());
    v.inv_tgt_gen = h->cloud_gen[kTgt], v.inv_n = t.n;
    v.launches += 1;
  }
  return 0;
}

// linearize (MP2 .. MP5) at T (column-major 4x4): two waits, one behind the total that sizes the rows, one behind the sums
int mp_linearize(apdgicp_handle* h, const double* T16, double* H, double* b, double* cost, int* matched) {
  APD_TRY(mp_prepare(h));
  Engine& e = h->eng;
  MpState& v = h->mp;
  roctx_range rr("apdgicp:gicp_mp_linearize");
  const Engine::Cloud &s = e.clouds[kSrc], &t = e.clouds[kTgt];
  const int n = s.n, nqb = (n + SQ_BLK - 1) / SQ_BLK, nsb = (n + SCAN_BLK - 1) / SCAN_BLK, npb = (n + MP_BLK - 1) / MP_BLK;
  const int xf = (e.params.flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0;
  const double radius = v.prm.neighbor_search_radius;
  const float r2 = (float)(radius * radius);  // Q4
  v.have = false;
  APD_TRY(v.q.ensure((size_t)n * sizeof(float4)));
  APD_TRY(v.cnt.ensure((size_t)n * sizeof(int)));
  APD_TRY(v.pos.ensure((size_t)n * sizeof(int)));
  APD_TRY(v.bsum.ensure(((size_t)nsb + 1) * sizeof(int)));
  APD_TRY(v.visit.ensure((size_t)nqb * sizeof(int)));
  APD_TRY(v.fused.ensure((size_t)n * MP_FUSED * sizeof(double)));
  APD_TRY(v.part.ensure((size_t)npb * MP_R * sizeof(double)));
  APD_TRY(v.out.ensure(64 * sizeof(double)));
  APD_TRY(v.T.ensure(12 * sizeof(double)));
  APD_TRY(v.tot.ensure(sizeof(long long)));
  double T12[12];
  colmajor_to_rows12(T16, T12);
  APD_HIP(hipMemcpyAsync(v.T.p, T12, sizeof(T12), hipMemcpyHostToDevice, e.stream));
  const SearchTarget tg{t.pts.as<float4>(), t.perm.as<int>(), t.cbox.as<Box>(), t.gbox.as<Box>(), t.n, 0};
  auto mark = [&](int k) -> int {  // (profiling only: an event behind what has been enqueued so far)
    if (!v.profiling) return 0;
    if (!v.ev[k]) APD_HIP(hipEventCreate(&v.ev[k]));
    APD_HIP(hipEventRecord(v.ev[k], e.stream));
    return 0;
  };
  APD_TRY(mark(0));
  hipLaunchKernelGGL(k_mp_transform, dim3((unsigned)npb), dim3(MP_BLK), 0, e.stream, s.pts.as<float4>(), n, v.T.as<double>(), xf, v.q.as<float4>());
  APD_TRY(mark(1));
  hipLaunchKernelGGL(k_radius_count, dim3((unsigned)nqb), dim3(SQ_BLK), 0, e.stream, tg, v.q.as<float4>(), s.perm.as<int>(), n, r2, v.cnt.as<int>(), v.visit.as<int>());
  hipLaunchKernelGGL(k_mp_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, v.q.as<float4>(), s.perm.as<int>(), n, v.cnt.as<int>());
  hipLaunchKernelGGL(k_mp_total, dim3(1), dim3(MP_BLK), 0, e.stream, v.cnt.as<int>(), n, v.tot.as<long long>());
  APD_TRY(mark(2));
  hipLaunchKernelGGL(k_radius_scan, dim3((unsigned)nsb), dim3(SCAN_BLK), 0, e.stream, v.cnt.as<int>(), n, v.pos.as<int>(), v.bsum.as<int>());
  hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, e.stream, v.bsum.as<int>(), nsb, v.bsum.as<int>() + nsb);
  APD_HIP(hipGetLastError());
  APD_TRY(mark(3));
  APD_HIP(hipMemcpyAsync(e.h_probe.p, v.tot.p, sizeof(long long), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  v.launches += 6, v.waits += 1;
  const long long total = *e.h_probe.as<long long>();
  if (total < 0 || total > 0x7fffffffll) return fail(APDGICP_ERR_UNSUPPORTED, "FastGICPMultiPoints: more than 2^31 - 1 hits in all (" + std::to_string(total) + ")");
  if (total > 0) APD_TRY(v.keys.ensure((size_t)total * sizeof(unsigned long long)));
  APD_TRY(mark(4));
  if (total > 0) {
    hipLaunchKernelGGL(k_radius_fill, dim3((unsigned)nqb), dim3(SQ_BLK), 0, e.stream, tg, v.q.as<float4>(), s.perm.as<int>(), n, r2, v.cnt.as<int>(), v.pos.as<int>(),
                       v.bsum.as<int>(), v.keys.as<unsigned long long>());
    APD_TRY(mark(5));
    hipLaunchKernelGGL(k_radius_sort_rows, dim3((unsigned)n), dim3(SQ_SORT_BLK), 0, e.stream, v.cnt.as<int>(), v.pos.as<int>(), v.bsum.as<int>(),
                       v.keys.as<unsigned long long>());
    v.launches += 2;
  } else {
    APD_TRY(mark(5));
  }
  APD_TRY(mark(6));
  const MpCloud S{s.pts.as<float4>(), s.cov.as<double>(), s.perm.as<int>(), n, 0}, Tg{t.opts.as<float4>(), t.cov.as<double>(), v.inv_t.as<int>(), t.n, 0};
  hipLaunchKernelGGL(k_mp_point, dim3((unsigned)npb), dim3(MP_BLK), 0, e.stream, S, Tg, v.keys.as<unsigned long long>(), v.cnt.as<int>(), v.pos.as<int>(), v.bsum.as<int>(),
                     v.T.as<double>(), radius, v.fused.as<double>(), v.part.as<double>());
  hipLaunchKernelGGL(k_icp_sums, dim3(1), dim3(64), 0, e.stream, v.part.as<double>(), npb, (int)MP_R, v.out.as<double>());
  APD_HIP(hipGetLastError());
  APD_TRY(mark(7));
  APD_HIP(hipMemcpyAsync(e.h_probe.p, v.out.p, MP_R * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  v.launches += 2, v.waits += 1;
  if (v.profiling) {
    const int from[6] = {0, 1, 2, 4, 5, 6}, to[6] = {1, 2, 3, 5, 6, 7};
    for (int k = 0; k < 6; k++) {
      float ms = 0.f;
      APD_HIP(hipEventElapsedTime(&ms, v.ev[from[k]], v.ev[to[k]]));
      v.phase_ms[k] = (double)ms;
    }
  }
  const double* o = e.h_probe.as<double>();
  int at = 0;
  for (int a = 0; a < 6; a++)
    for (int c = a; c < 6; c++, at++) h->final_H[a + 6 * c] = h->final_H[c + 6 * a] = o[at];  // MP9: the last H
  if (H && b) {
    memcpy(H, h->final_H, 36 * sizeof(double));
    memcpy(b, o + 21, 6 * sizeof(double));
  }
  if (cost) *cost = o[27];
  if (matched) *matched = (int)std::min(o[28], 2147483647.0);
  v.have = true, v.have_src_gen = h->cloud_gen[kSrc], v.have_tgt_gen = h->cloud_gen[kTgt], v.n_have = n, v.total = total;
  return 0;
}

// MP6 / MP7: plain Gauss-Newton on the host over mp_linearize
int mp_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  Engine& e = h->eng;
  MpState& v = h->mp;
  const apdgicp_params& p = e.params;
  v.launches = v.waits = 0;
  APD_TRY(mp_prepare(h));
  float g[16];
  if (guess) memcpy(g, guess, sizeof(g));
  else identity16(g);
  Rigid x;  // MP6: the guess's blocks, widened
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) x.m[4 * i + j] = (double)g[i + 4 * j];
  v.tr_pose.clear(), v.tr_cost.clear(), v.tr_delta.clear(), v.tr_n.clear();
  v.state = APDGICP_GICP_MP_NOT_CONVERGED;
  bool converged = false;
  int iterations = 0, n_lin = 0, matched = 0;
  double cost = 0.0;
  for (int it = 0; it < p.max_iterations; it++) {  // MPI:92
    iterations = it;
    double T16[16], H[36], gr[6], ng[6], d[6] = {0, 0, 0, 0, 0, 0};
    rigid_to_colmajor(x, T16);
    APD_TRY(mp_linearize(h, T16, H, gr, &cost, &matched));
    n_lin++;
    v.tr_pose.insert(v.tr_pose.end(), T16, T16 + 16), v.tr_cost.push_back(cost), v.tr_n.push_back(matched);
    if (matched < 2) {  // MP7: H has rank <= 3 per row
      v.state = APDGICP_GICP_MP_TOO_FEW_ROWS;
      v.tr_delta.insert(v.tr_delta.end(), d, d + 6);
      break;
    }
    for (int q = 0; q < 6; q++) ng[q] = -gr[q];
    solve6_spd(H, 0.0, ng, d);  // H d = g (MPI:99)
    v.tr_delta.insert(v.tr_delta.end(), d, d + 6);
    bool finite = true;
    for (int q = 0; q < 6; q++) finite = finite && std::isfinite(d[q]);
    if (!finite) {
      v.state = APDGICP_GICP_MP_SINGULAR;
      break;
    }
    const double nr[6] = {-d[0], -d[1], -d[2], 0.0, 0.0, 0.0};
    const Rigid E = make_delta(nr);  // MPI:101-102: R <- exp(-d_r) R, t <- t - d_t (the translation is not rotated)
    Rigid y = x;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) y.m[4 * i + j] = (E.m[4 * i] * x.m[j] + E.m[4 * i + 1] * x.m[4 + j]) + E.m[4 * i + 2] * x.m[8 + j];
      y.m[4 * i + 3] = x.m[4 * i + 3] - d[3 + i];
    }
    x = y;
    if (is_converged(make_delta(d), p.rotation_epsilon, p.transformation_epsilon)) {  // MPI:104, 118-127
      converged = true;
      v.state = APDGICP_GICP_MP_CONVERGED;
      break;
    }
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) out->T[i + 4 * j] = (float)x.m[4 * i + j];
  out->T[3] = out->T[7] = out->T[11] = 0.f;
  out->T[15] = 1.f;
  out->final_cost = cost;
  out->converged = converged;
  out->iterations = iterations;
  out->n_linearize = n_lin;
  out->n_compute_error = 0;
  out->lm_failed = 0;
  out->n_matched = matched;
  h->trace_from_host_loop = true;  // (apdgicp_get_trace: this align left no optimiser trace)
  h->tr_lambda.clear(), h->tr_rho.clear(), h->tr_y0.clear(), h->tr_yi.clear(), h->tr_dnorm.clear(), h->tr_poses.clear();
  return 0;
}

// the align of the mode that is on (APD has two loops of its own: apdgicp_align, apdgicp_align_host_loop)
int mode_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  switch (h->mode) {
    case Mode::ICP: return ic_align(h, guess, out);
    case Mode::GICP_MP: return mp_align(h, guess, out);
    case Mode::NDT: return nd_align(h, guess, out);
    case Mode::VGICP: return vg_align(h, guess, out);
    case Mode::VGICP_CUDA: return vc_align(h, guess, out);
    case Mode::APD: break;
  }
  return fail(APDGICP_ERR_INTERNAL, "no mode is on");
}

int check_icp_params(const apdgicp_icp_params* p) {
  if (!p) return 0;
  if (p->min_correspondences < 1) return fail(APDGICP_ERR_INVALID_ARG, "ICP: min_correspondences must be at least 1");
  if (p->max_similar_transforms < 0) return fail(APDGICP_ERR_INVALID_ARG, "ICP: max_similar_transforms must not be negative");
  if (std::isnan(p->euclidean_fitness_epsilon) || std::isnan(p->rotation_epsilon) || std::isnan(p->mse_threshold_absolute))
    return fail(APDGICP_ERR_INVALID_ARG, "ICP: a threshold is not a number");
  return 0;
}

const char* const kIcNoLinearize = "point-to-point ICP has no linearisation: apdgicp_icp_estimate is this mode's probe";

// ---- the voxel modes on a batch handle: what voxelized GICP (V8 .. V12) and NDT (N10 .. N15) share
constexpr int kVgbChunk = 4;  // ticks enqueued per look at the done counter (docs/experiments.md, "VGICP batch: chunk length")

int device_loop_ensure_words(apdgicp_batch* b, size_t ints) {
  DeviceLoop& l = b->loop;
  if (ints * sizeof(int) <= l.h_words.cap) return 0;
  APD_HIP(hipStreamSynchronize(b->eng.stream));
  APD_TRY(l.h_words.ensure(std::max<size_t>(ints * 2, 1024) * sizeof(int)));
  memset(l.h_words.p, 0, l.h_words.cap);
  return 0;
}

// V8 / N10: the maps of the listed slots (sorted) that are not current: enqueued one after the other with no wait in between, then ONE copy of
// every slot's {first bad point, voxel count} and one wait for all of them.  The mode says which slots are current(t), whether a slot's own
// buffers grow(t), sizes them and enqueues the build of slot t (launch(t): enqueue_voxel_sort, then its voxel kernel) and marks it
// built(t, nv); prefix: "voxelized GICP: " / "NDT: ".  errflag (voxelized GICP): the covariance kernels' flag, read with the same wait.
template <class Current, class Grows, class Launch, class Built>
int batch_build_maps(apdgicp_batch* b, const std::vector<int>& slots, const char* prefix, double resolution, const DevBuf& scal, Current&& current, Grows&& grows,
                     Launch&& launch, Built&& built, int* errflag = nullptr, const std::function<int(int, int)>* caller_index = nullptr) {
  Engine& e = b->eng;
  std::vector<int> todo;
  int nmax = 0;
  for (int t : slots)
    if (!current(t) && std::find(todo.begin(), todo.end(), t) == todo.end()) todo.push_back(t), nmax = std::max(nmax, e.clouds[t].n);
  if (todo.empty()) return 0;
  const int lo = *std::min_element(todo.begin(), todo.end()), hi = *std::max_element(todo.begin(), todo.end());
  APD_TRY(device_loop_ensure_words(b, 4 + 4 * (size_t)(hi - lo + 1)));
  bool any_grows = false;
  APD_TRY(b->sort.ensure(nmax, &any_grows));
  for (int t : todo) any_grows |= grows(t);
  if (any_grows) APD_HIP(hipStreamSynchronize(e.stream));  // (buffers below may be replaced; never on a reused handle with clouds of the same sizes)
  APD_TRY(b->sort.ensure(nmax));
  // (a slot with an offending point has key 0 there: its voxels are wrong and never used -- the align fails below before any pair runs)
  for (int t : todo) APD_TRY(launch(t));
  int* hw = b->loop.h_words.as<int>() + 4;
  APD_HIP(hipMemcpyAsync(hw, scal.as<int>() + 4 * (size_t)lo, (size_t)(hi - lo + 1) * 16, hipMemcpyDeviceToHost, e.stream));
  if (errflag) APD_HIP(hipMemcpyAsync(b->loop.h_words.as<int>() + 2, e.d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  if (errflag) *errflag = b->loop.h_words.as<int>()[2];
  int rc = 0;
  for (int t : todo) {
    const int* w = hw + 4 * (size_t)(t - lo);
    if (w[0] != kVgBadNone) {
      // (caller_index: the mode built the map over a compacted cloud and names the point by its index in the caller's)
      if (rc == 0) rc = voxel_key_range_error(std::string(prefix) + "point " + std::to_string(caller_index ? (*caller_index)(t, w[0]) : w[0]) + " of cloud slot " + std::to_string(t), resolution);
    } else if (w[1] < 1 || w[1] > e.clouds[t].n) {
      if (rc == 0) rc = fail(APDGICP_ERR_INTERNAL, std::string(prefix) + "inconsistent voxel count");
    } else {
      built(t, w[1]);
    }
  }
  return rc;
}

// room for `bytes` device bytes per slot of the engine; the words of what is built survive a growth
int batch_ensure_slot_words(Engine& e, DevBuf& words, int& slots, size_t bytes) {
  const int want = (int)e.clouds.size();
  if (want <= slots) return 0;
  const int cap = std::max(64, 2 * want);
  DevBuf grown;
  APD_TRY(grown.ensure((size_t)cap * bytes));
  APD_HIP(hipStreamSynchronize(e.stream));
  if (slots) APD_HIP(hipMemcpy(grown.p, words.p, (size_t)slots * bytes, hipMemcpyDeviceToDevice));
  words = std::move(grown);
  slots = cap;
  return 0;
}

// room for every slot of the engine in a mode's table and in the list of what its maps were made from (ids: the mode's `slots`)
template <class Id>
int ensure_slots(Engine& e, VoxSlots& s, std::vector<Id>& ids) {
  if (ids.size() < e.clouds.size()) ids.resize(e.clouds.size());
  if (s.slots.size() < e.clouds.size()) s.slots.resize(e.clouds.size());
  return batch_ensure_slot_words(e, s.scal, s.scal_slots, 16);
}

void mark_built(VoxSlots& s, int t, int nv) { s.slots[t].nv = nv, s.builds++; }  // slot t's build has come home (what it was made from: stamped by the mode)

// the head of a getter of one slot in mode m; the caller goes on to upload_desc (sorts what is not sorted yet: a staged cloud's opts are written by its sort)
int batch_slot_enter(apdgicp_batch* b, Mode m, int32_t cloud) {
  Engine& e = b->eng;
  if (b->mode != m) return mode_is_off(m, true);
  if (cloud < 0 || cloud >= (int)e.clouds.size() || e.clouds[cloud].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "cloud not set");
  APD_HIP(hipSetDevice(e.device));
  APD_TRY(e.pool_leave());
  return e.finish_align();
}

// V12 / N15: what the tick loop needs besides the pairs -- the done counter, the pinned words, the two events
int device_loop_prepare(apdgicp_batch* b) {
  DeviceLoop& v = b->loop;
  APD_TRY(v.done.ensure(16));
  APD_TRY(device_loop_ensure_words(b, 4));
  for (hipEvent_t& ev : v.ev)
    if (!ev) APD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return 0;
}

// V10 / V12 / N13 / N15: the optimiser loop of every pair of the engine's list (setup_pairs done, device_loop_prepare done) on the device.
// launch_tick() enqueues the two launches of one tick on the engine's stream.  Ticks go out in chunks, one chunk ahead of the pinned word the
// host looks at; returns with the device records complete and the deferred error flag read.
// launch_init() enqueues what builds every pair's state and zeroes the done counter; bound: the ticks after which every pair has finished (0:
// no tick runs, the records are those of the initial states -- the voxel modes only).
template <class Init, class Tick>
int device_loop_run(apdgicp_batch* b, long long bound, Init&& launch_init, Tick&& launch_tick) {
  Engine& e = b->eng;
  DeviceLoop& v = b->loop;
  const int np = e.npairs;
  PairState* st = e.d_state.as<PairState>();
  ResultRec* recs = e.d_results.as<ResultRec>();
  launch_init();
  const int chunk = std::max(1, v.chunk);
  long long ticks = 0;
  int nchunks = 0, waits = 0;
  auto enqueue_chunk = [&]() -> int {
    const int todo = (int)std::min<long long>(chunk, bound - ticks);
    for (int q = 0; q < todo; q++) launch_tick();
    APD_HIP(hipGetLastError());
    ticks += todo;
    // the done counter as of this chunk, mirrored into the pinned word of the chunk's parity
    APD_HIP(hipMemcpyAsync(v.h_words.as<int>() + (nchunks & 1), v.done.p, sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipEventRecord(v.ev[nchunks & 1], e.stream));
    nchunks++;
    return 0;
  };
  if (bound == 0) {
    hipLaunchKernelGGL(k_vgb_records, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, e.stream, st, np, recs);
    APD_HIP(hipGetLastError());
  } else {
    APD_TRY(enqueue_chunk());
    for (int waited = 0;; waited++) {
      if (ticks < bound) APD_TRY(enqueue_chunk());  // (one chunk ahead while the host waits for the one before)
      APD_HIP(hipEventSynchronize(v.ev[waited & 1]));
      waits++;
      if (v.h_words.as<int>()[waited & 1] >= np || waited + 1 >= nchunks) break;
    }
  }
  // the covariance kernels' error flag (deferred by setup_pairs) with the final wait
  APD_HIP(hipMemcpyAsync(v.h_words.as<int>() + 2, e.d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  for (Engine::Cloud& c : e.clouds) c.stage_pending = false, c.stage_wait = nullptr, c.stage_seq_word = nullptr;  // (every sort has run)
  e.n_stage_pending = 0;
  v.last_ticks = (int)ticks;
  v.last_chunks = nchunks, v.last_waits = waits + 1;
  e.last_ticks = (int)ticks;
  if (v.h_words.as<int>()[2]) {
    const int flag = v.h_words.as<int>()[2];
    APD_HIP(hipMemsetAsync(e.d_errflag.p, 0, sizeof(int), e.stream));
    return fail(APDGICP_ERR_INTERNAL, Engine::errflag_text(flag));
  }
  e.poses_of_align = true;
  return 0;
}

// the voxel modes: V10's state machine from the guesses, its tick bound
template <class Tick>
int device_loop_run(apdgicp_batch* b, Tick&& launch_tick) {
  Engine& e = b->eng;
  const apdgicp_params& p = e.params;
  const long long bound = p.max_iterations <= 0 ? 0 : (p.optimizer == APDGICP_OPT_GN ? (long long)p.max_iterations : (long long)p.max_iterations * (1 + (long long)std::max(0, p.lm_max_iterations)));
  return device_loop_run(
      b, bound,
      [&]() {
        hipLaunchKernelGGL(k_vgb_init, dim3((unsigned)((e.npairs + 63) / 64)), dim3(64), 0, e.stream, e.d_state.as<PairState>(), e.d_guess.as<Rigid>(), e.npairs,
                           p.max_iterations, b->loop.done.as<int>());
      },
      launch_tick);
}

struct VoxTick {  // what the two launches of a voxel mode's tick read besides the mode's own: sizes, strides and pointers of this align
  int np, nblk_max;
  size_t corr_stride;
  Consts cst;
  PairState* st;
  ResultRec* recs;
  int *corr, *done;
  double* part;
};

// V10 / V12 / N13 / N15 / VC14 / VC16: the tail of a voxel mode's align, its pair table uploaded (apdgicp_batch::run) -- the frozen indices
// (pairs x rows_max x noff ints, min_corr_bytes at least) and the block rows sized, then the loop of every pair on the device, a tick being
// launch_points(t) then launch_step(t).  (rows_max is 0 only where FAST_VGICP_CUDA kept no source point anywhere: one block per pair, which
// returns.)
template <class Points, class Step>
int voxel_batch_run(apdgicp_batch* b, int rows_max, int noff, size_t min_corr_bytes, Points&& launch_points, Step&& launch_step) {
  Engine& e = b->eng;
  VoxRun& r = b->run;
  const int np = e.npairs, nblk_max = std::max(1, (rows_max + VG_BLK - 1) / VG_BLK);
  r.noff = noff, r.corr_stride = (size_t)rows_max * (size_t)noff;  // (computed in size_t)
  APD_TRY(ensure_corr_part(e, r.corr, r.part, std::max(min_corr_bytes, (size_t)np * r.corr_stride * 4), (size_t)np * nblk_max * VG_RED * 8));
  APD_TRY(device_loop_prepare(b));
  const VoxTick t{np, nblk_max, r.corr_stride, e.consts(), e.d_state.as<PairState>(), e.d_results.as<ResultRec>(), r.corr.as<int>(), b->loop.done.as<int>(), r.part.as<double>()};
  return device_loop_run(b, [&]() {
    launch_points(t);
    launch_step(t);
  });
}

// ---- voxelized GICP on a batch handle (include/apdgicp_hip.h V8 .. V12; kernels: apd_vgicp_batch.hpp)
bool vgb_map_current(const apdgicp_batch* b, int slot) {
  const VgbState& v = b->vg;
  const Engine::Cloud& c = b->eng.clouds[slot];
  const VgbState::Slot& sl = v.slots[slot];
  return sl.map_built && c.cov_valid && sl.map_pts_gen == c.pts_gen && sl.map_cov_gen == c.cov_gen && sl.map_res == v.prm.resolution && sl.map_mode == v.prm.voxel_mode;
}

// the inverse permutation of a sorted slot, once per setting of its points
int vgb_ensure_inv(apdgicp_batch* b, int slot) {
  Engine& e = b->eng;
  Engine::Cloud& c = e.clouds[slot];
  VgbState::Slot& sl = b->vg.slots[slot];
  if (sl.inv.p && sl.inv_pts_gen == c.pts_gen && (size_t)c.n * 4 <= sl.inv.cap) return 0;
  sl.inv_pts_gen = 0;
  if ((size_t)c.n * 4 > sl.inv.cap) APD_HIP(hipStreamSynchronize(e.stream));
  APD_TRY(sl.inv.ensure((size_t)c.n * 4));
  hipLaunchKernelGGL(k_vg_inverse_perm, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, e.stream, c.perm.as<int>(), c.n, sl.inv.as<int>());
  APD_HIP(hipGetLastError());
  sl.inv_pts_gen = c.pts_gen;
  return 0;
}

// V8: the maps of the listed slots (sorted, covariances there) that are not current
int vgb_build_maps(apdgicp_batch* b, const std::vector<int>& targets) {
  Engine& e = b->eng;
  VgbState& v = b->vg;
  APD_TRY(ensure_slots(e, v.vox, v.slots));
  int flag = 0;
  int rc = batch_build_maps(
      b, targets, "voxelized GICP: ", v.prm.resolution, v.vox.scal, [&](int t) { return vgb_map_current(b, t); },
      [&](int t) { return (size_t)e.clouds[t].n * 48 > v.vox.slots[t].buf.vcov.cap || (size_t)e.clouds[t].n * 4 > v.slots[t].inv.cap; },
      [&](int t) -> int {
        Engine::Cloud& c = e.clouds[t];
        VgbState::Slot& sl = v.slots[t];
        VoxMapBufs& buf = v.vox.slots[t].buf;
        const int n = c.n;
        sl.map_built = false;
        APD_TRY(buf.ensure((size_t)n, false));
        APD_TRY(vgb_ensure_inv(b, t));
        VoxSorted s;
        APD_TRY(enqueue_voxel_sort(e.stream, b->sort, c.opts.as<float4>(), n, v.prm.resolution, v.vox.words(t), &s));
        hipLaunchKernelGGL(k_vg_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, n, b->sort.bsum.as<int>(), c.opts.as<float4>(), c.cov.as<double>(), sl.inv.as<int>(),
                           buf.vkeys.as<unsigned long long>(), buf.vcount.as<int>(), buf.vmean.as<double>(), buf.vcov.as<double>(), n);
        APD_HIP(hipGetLastError());
        return 0;
      },
      [&](int t, int nv) {
        VgbState::Slot& sl = v.slots[t];
        const Engine::Cloud& c = e.clouds[t];
        mark_built(v.vox, t, nv);
        sl.map_built = true, sl.map_pts_gen = c.pts_gen, sl.map_cov_gen = c.cov_gen, sl.map_res = v.prm.resolution, sl.map_mode = v.prm.voxel_mode;
      },
      &flag);
  if (flag) {  // a point that is not finite trips the covariance kernels too: the message about the point is the useful one
    APD_HIP(hipMemsetAsync(e.d_errflag.p, 0, sizeof(int), e.stream));
    if (rc == 0) rc = fail(APDGICP_ERR_INTERNAL, Engine::errflag_text(flag));
  }
  return rc;
}

// one slot's map for the getters: sorted, covariances computed, built
int vgb_slot_map(apdgicp_batch* b, int32_t cloud) {
  Engine& e = b->eng;
  APD_TRY(batch_slot_enter(b, Mode::VGICP, cloud));
  APD_TRY(e.compute_covariances({cloud}));
  APD_TRY(e.upload_desc());
  return vgb_build_maps(b, {cloud});
}

// V10 / V12: the optimiser loop of every pair on the device; returns with the device records complete
int vgb_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs) {
  Engine& e = b->eng;
  VgbState& v = b->vg;
  APD_TRY(e.finish_align());  // (an uncollected deferred align from before the mode was switched on)
  APD_TRY(e.setup_pairs(pairs, n_pairs, true));  // clouds sorted, covariances there, d_state / d_results / d_guess
  e.results_on_host = false;
  const int np = e.npairs, noff = n_offsets(v.prm.neighbor_search);
  std::vector<int> targets;
  for (int i = 0; i < np; i++) targets.push_back(e.h_pairs[i].tgt);
  APD_TRY(vgb_build_maps(b, targets));
  for (int i = 0; i < np; i++) APD_TRY(vgb_ensure_inv(b, e.h_pairs[i].src));
  std::vector<VgbPair> tab(np);
  for (int i = 0; i < np; i++) {
    const int s = e.h_pairs[i].src, t = e.h_pairs[i].tgt;
    tab[i] = VgbPair{e.clouds[s].opts.as<float4>(), e.clouds[s].cov.as<double>(), v.slots[s].inv.as<int>(), e.clouds[s].n, 0, v.vox.map(t)};
  }
  APD_TRY(b->run.pairs.upload(tab.data(), tab.size() * sizeof(VgbPair), e.stream));
  return voxel_batch_run(
      b, e.nmax_src, noff, 0,
      [&](const VoxTick& t) {
        hipLaunchKernelGGL(k_vgb_points, dim3((unsigned)t.nblk_max, (unsigned)t.np), dim3(VG_BLK), 0, e.stream, b->run.pairs.as<VgbPair>(), t.st, v.prm.resolution,
                           (int)v.prm.neighbor_search, noff, t.corr, t.corr_stride, t.part, t.nblk_max);
      },
      [&](const VoxTick& t) {
        hipLaunchKernelGGL(k_vgb_step, dim3((unsigned)t.np), dim3(64), 0, e.stream, b->run.pairs.as<VgbPair>(), t.st, t.cst, t.part, t.nblk_max, t.recs, t.done);
      });
}

// ---- NDT on a batch handle (include/apdgicp_hip.h N10 .. N15; kernels: apd_ndt_batch.hpp)
bool ndb_map_current(const apdgicp_batch* b, int slot) {
  const NdbState::Slot& sl = b->nd.slots[slot];
  return sl.built && sl.pts_gen == b->eng.clouds[slot].pts_gen && sl.res == b->nd.prm.resolution;
}

// N10: the maps of the listed slots (sorted) that are not current.  No covariances (so no error flag to read), no inverse permutation.
int ndb_build_maps(apdgicp_batch* b, const std::vector<int>& slots) {
  Engine& e = b->eng;
  NdbState& v = b->nd;
  APD_TRY(ensure_slots(e, v.vox, v.slots));
  return batch_build_maps(
      b, slots, "NDT: ", v.prm.resolution, v.vox.scal, [&](int t) { return ndb_map_current(b, t); },
      [&](int t) { return (size_t)e.clouds[t].n * 48 > v.vox.slots[t].buf.vcov.cap; },
      [&](int t) -> int {
        Engine::Cloud& c = e.clouds[t];
        VoxMapBufs& buf = v.vox.slots[t].buf;
        const int n = c.n;
        v.slots[t].built = false;
        APD_TRY(buf.ensure((size_t)n, true));
        VoxSorted s;
        APD_TRY(enqueue_voxel_sort(e.stream, b->sort, c.opts.as<float4>(), n, v.prm.resolution, v.vox.words(t), &s));
        hipLaunchKernelGGL(k_ndt_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, n, b->sort.bsum.as<int>(), c.opts.as<float4>(), buf.vkeys.as<unsigned long long>(),
                           buf.vcount.as<int>(), buf.vmean.as<double>(), buf.vraw.as<double>(), buf.vcov.as<double>(), n);
        APD_HIP(hipGetLastError());
        return 0;
      },
      [&](int t, int nv) {
        NdbState::Slot& sl = v.slots[t];
        mark_built(v.vox, t, nv);
        sl.built = true, sl.pts_gen = e.clouds[t].pts_gen, sl.res = v.prm.resolution;
      });
}

// one slot's map for the getters: sorted, built
int ndb_slot_map(apdgicp_batch* b, int32_t cloud) {
  APD_TRY(batch_slot_enter(b, Mode::NDT, cloud));
  APD_TRY(b->eng.upload_desc());
  return ndb_build_maps(b, {cloud});
}

// N13 / N15: the optimiser loop of every pair on the device; returns with the device records complete
int ndb_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs) {
  Engine& e = b->eng;
  NdbState& v = b->nd;
  APD_TRY(e.finish_align());  // (an uncollected deferred align from before the mode was switched on)
  APD_TRY(e.setup_pairs(pairs, n_pairs, true, /*pipeline_cov=*/false, /*need_cov=*/false));  // N11: clouds sorted, d_state / d_results / d_guess
  e.results_on_host = false;
  const int np = e.npairs, noff = n_offsets(v.prm.neighbor_search);
  const bool d2d = v.prm.distance_mode == APDGICP_NDT_D2D;
  std::vector<int> slots;
  for (int i = 0; i < np; i++) {
    slots.push_back(e.h_pairs[i].tgt);
    if (d2d) slots.push_back(e.h_pairs[i].src);
  }
  APD_TRY(ndb_build_maps(b, slots));
  std::vector<NdbPair> tab(np);
  for (int i = 0; i < np; i++) {
    const int s = e.h_pairs[i].src, t = e.h_pairs[i].tgt;
    tab[i] = NdbPair{e.clouds[s].opts.as<float4>(), e.clouds[s].n, 0, d2d ? v.vox.map(s) : VgbMap{nullptr, nullptr, nullptr, nullptr, nullptr}, v.vox.map(t)};
  }
  APD_TRY(b->run.pairs.upload(tab.data(), tab.size() * sizeof(NdbPair), e.stream));
  // (a pair's rows are at most its source's points: the grid and the strides are sized by the points, the blocks beyond a pair's rows return)
  return voxel_batch_run(
      b, e.nmax_src, noff, 0,
      [&](const VoxTick& t) {
        const dim3 grid((unsigned)t.nblk_max, (unsigned)t.np);
        if (d2d)
          hipLaunchKernelGGL(k_ndb_points<true>, grid, dim3(VG_BLK), 0, e.stream, b->run.pairs.as<NdbPair>(), t.st, v.prm.resolution, (int)v.prm.neighbor_search, noff, t.corr,
                             t.corr_stride, t.part, t.nblk_max);
        else
          hipLaunchKernelGGL(k_ndb_points<false>, grid, dim3(VG_BLK), 0, e.stream, b->run.pairs.as<NdbPair>(), t.st, v.prm.resolution, (int)v.prm.neighbor_search, noff, t.corr,
                             t.corr_stride, t.part, t.nblk_max);
      },
      [&](const VoxTick& t) {
        hipLaunchKernelGGL(k_ndb_step, dim3((unsigned)t.np), dim3(64), 0, e.stream, b->run.pairs.as<NdbPair>(), t.st, t.cst, t.part, t.nblk_max, d2d ? 1 : 0, t.recs, t.done);
      });
}

// ---- FAST_VGICP_CUDA on a batch handle (include/apdgicp_hip.h VC11 .. VC16; kernels: apd_vgicp_cuda_batch.hpp)
bool vcb_prepared(const apdgicp_batch* b, int slot) {
  const VcPrepared& pc = b->vc.slots[slot].pc;
  return pc.ready && pc.pts_gen == b->eng.clouds[slot].pts_gen && pc.reg == b->vc.prm.regularization;
}

bool vcb_map_current(const apdgicp_batch* b, int slot) {
  const VcbState::Slot& sl = b->vc.slots[slot];
  return vcb_prepared(b, slot) && sl.map_built && sl.map_prep_id == sl.pc.id && sl.map_res == b->vc.prm.resolution;
}

// VC11: the prepared clouds of the listed slots (sorted) that are not current.  The launches of all of them go out with no wait in between;
// ONE copy brings every slot's kept count back, one the k-NN error flag, and one wait covers both.
int vcb_prepare_slots(apdgicp_batch* b, const std::vector<int>& slots) {
  Engine& e = b->eng;
  VcbState& v = b->vc;
  APD_TRY(ensure_slots(e, v.vox, v.slots));
  APD_TRY(batch_ensure_slot_words(e, v.nk, v.nk_slots, 4));  // (the kept counts, one int per slot)
  std::vector<int> todo;
  for (int t : slots) {
    if (e.clouds[t].n < VC_K) return fail(APDGICP_ERR_TOO_FEW_POINTS, "FAST_VGICP_CUDA: cloud slot " + std::to_string(t) + " has fewer than " + std::to_string(VC_K) + " points");
    if (!vcb_prepared(b, t) && std::find(todo.begin(), todo.end(), t) == todo.end()) todo.push_back(t);
  }
  if (todo.empty()) return 0;
  std::sort(todo.begin(), todo.end());
  const int lo = todo.front(), hi = todo.back();
  APD_TRY(device_loop_ensure_words(b, 4 + (size_t)(hi - lo + 1)));
  std::vector<VcJob> jobs;
  for (int t : todo) {
    v.slots[t].map_built = false;
    jobs.push_back(VcJob{t, &v.slots[t].pc, v.nk.as<int>() + t});
  }
  bool waited = false;
  const int rc = vc_enqueue_prepare(e, jobs, v.prm.regularization, v.prep_tab, v.prep_ids, &waited);
  if (waited) v.prep_waits++;
  APD_TRY(rc);
  int* hw = b->loop.h_words.as<int>();
  APD_HIP(hipMemcpyAsync(hw + 4, v.nk.as<int>() + lo, (size_t)(hi - lo + 1) * 4, hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipMemcpyAsync(hw + 2, e.d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  v.prep_waits++;
  if (hw[2]) return vc_knn_flag_error(e, hw[2]);
  for (int t : todo) {
    const int nk = hw[4 + (t - lo)];
    if (nk < 0 || nk > e.clouds[t].n) return fail(APDGICP_ERR_INTERNAL, "FAST_VGICP_CUDA: inconsistent kept count");
  }
  for (int t : todo) {
    VcPrepared& pc = v.slots[t].pc;
    pc.n = e.clouds[t].n, pc.n_kept = hw[4 + (t - lo)];
    pc.pts_gen = e.clouds[t].pts_gen, pc.reg = v.prm.regularization, pc.id = ++v.preps;
    pc.ready = true;
  }
  return 0;
}

// VC12: the maps of the listed slots (prepared) that are not current, over their kept points
int vcb_build_maps(apdgicp_batch* b, const std::vector<int>& targets) {
  Engine& e = b->eng;
  VcbState& v = b->vc;
  std::vector<int> full;
  for (int t : targets) {
    VcbState::Slot& sl = v.slots[t];
    if (vcb_map_current(b, t)) continue;
    if (sl.pc.n_kept > 0) {
      full.push_back(t);
      continue;
    }
    // no kept point: an empty map, no sort (the shared builder calls a voxel count of 0 inconsistent) -- the device word the tick reads is 0
    APD_HIP(hipMemsetAsync(v.vox.words(t), 0, 16, e.stream));
    mark_built(v.vox, t, 0);
    sl.map_built = true, sl.map_prep_id = sl.pc.id, sl.map_res = v.prm.resolution;
  }
  if (full.empty()) return 0;
  v.map_waits++;
  const std::function<int(int, int)> caller_index = [&](int t, int j) -> int {  // kept point j of slot t in the caller's cloud (an error path: its own wait)
    int orig = -1;
    if (j >= 0 && j < v.slots[t].pc.n_kept && hipMemcpy(&orig, v.slots[t].pc.kept.as<int>() + j, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) orig = -1;
    return orig;
  };
  return batch_build_maps(
      b, full, "FAST_VGICP_CUDA: ", v.prm.resolution, v.vox.scal, [&](int) { return false; },
      [&](int t) { return (size_t)v.slots[t].pc.n_kept * 48 > v.vox.slots[t].buf.vcov.cap; },
      [&](int t) -> int {
        VcbState::Slot& sl = v.slots[t];
        VoxMapBufs& buf = v.vox.slots[t].buf;
        const VcPrepared& pc = sl.pc;
        const int n = pc.n_kept;
        sl.map_built = false;
        APD_TRY(buf.ensure((size_t)n, false));
        VoxSorted s;
        APD_TRY(enqueue_voxel_sort(e.stream, b->sort, pc.kpts.as<float4>(), n, v.prm.resolution, v.vox.words(t), &s));
        hipLaunchKernelGGL(k_vg_voxels, dim3(s.nhb), dim3(MAP_BLK), 0, e.stream, s.keys, s.idx, n, b->sort.bsum.as<int>(), pc.kpts.as<float4>(), pc.kcov.as<double>(), pc.ident.as<int>(),
                           buf.vkeys.as<unsigned long long>(), buf.vcount.as<int>(), buf.vmean.as<double>(), buf.vcov.as<double>(), n);
        APD_HIP(hipGetLastError());
        return 0;
      },
      [&](int t, int nv) {
        VcbState::Slot& sl = v.slots[t];
        mark_built(v.vox, t, nv);
        sl.map_built = true, sl.map_prep_id = sl.pc.id, sl.map_res = v.prm.resolution;
      },
      nullptr, &caller_index);
}

// one slot for the getters: sorted, prepared, and with want_map its map built
int vcb_slot(apdgicp_batch* b, int32_t cloud, bool want_map) {
  APD_TRY(batch_slot_enter(b, Mode::VGICP_CUDA, cloud));
  APD_TRY(b->eng.upload_desc());
  APD_TRY(vcb_prepare_slots(b, {cloud}));
  return want_map ? vcb_build_maps(b, {cloud}) : 0;
}

// VC14 / VC16: the optimiser loop of every pair on the device; returns with the device records complete
int vcb_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs) {
  Engine& e = b->eng;
  VcbState& v = b->vc;
  v.have = false;
  APD_TRY(e.finish_align());  // (an uncollected deferred align from before the mode was switched on)
  APD_TRY(e.setup_pairs(pairs, n_pairs, true, /*pipeline_cov=*/false, /*need_cov=*/false));  // VC11: clouds sorted, d_state / d_results / d_guess; no covariances
  e.results_on_host = false;
  const int np = e.npairs;
  std::vector<int> named, targets;
  for (int i = 0; i < np; i++) named.push_back(e.h_pairs[i].src), named.push_back(e.h_pairs[i].tgt), targets.push_back(e.h_pairs[i].tgt);
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  // apdgicp_batch_set_profiling: the phases of this align by the host clock.  One more wait in front (the sorts of the clouds set since the
  // last align are not this mode's preparation); every other boundary is behind a wait the align makes anyway.
  if (e.profile_nn) APD_HIP(hipStreamSynchronize(e.stream));
  clock::time_point t0 = clock::now();
  APD_TRY(vcb_prepare_slots(b, named));
  v.phase_ms[0] = ms_since(t0), t0 = clock::now();
  APD_TRY(vcb_build_maps(b, targets));
  v.phase_ms[1] = ms_since(t0), t0 = clock::now();
  APD_TRY(v.offs.ensure(v.prm, e.stream));
  const int noff = v.offs.count();
  std::vector<VgbPair> tab(np);
  std::vector<int> nks(np);
  int nk_max = 0;
  for (int i = 0; i < np; i++) {
    const VcPrepared& s = v.slots[e.h_pairs[i].src].pc;
    tab[i] = VgbPair{s.kpts.as<float4>(), s.kcov.as<double>(), s.ident.as<int>(), s.n_kept, 0, v.vox.map(e.h_pairs[i].tgt)};
    nks[i] = s.n_kept;
    nk_max = std::max(nk_max, s.n_kept);
  }
  APD_TRY(b->run.pairs.upload(tab.data(), tab.size() * sizeof(VgbPair), e.stream));
  APD_TRY(voxel_batch_run(
      b, nk_max, noff, 16,
      [&](const VoxTick& t) {
        hipLaunchKernelGGL(k_vcb_points, dim3((unsigned)t.nblk_max, (unsigned)t.np), dim3(VG_BLK), 0, e.stream, b->run.pairs.as<VgbPair>(), t.st, v.prm.resolution,
                           v.offs.dev.as<int>(), noff, t.corr, t.corr_stride, t.part, t.nblk_max);
      },
      [&](const VoxTick& t) {
        hipLaunchKernelGGL(k_vgb_step, dim3((unsigned)t.np), dim3(64), 0, e.stream, b->run.pairs.as<VgbPair>(), t.st, t.cst, t.part, t.nblk_max, t.recs, t.done);
      }));
  v.phase_ms[2] = ms_since(t0);
  v.have = true, v.have_epoch = e.pts_epoch, v.have_nk = nks;
  return 0;
}

// ---- point-to-point ICP on a batch handle (include/apdgicp_hip.h IC11 .. IC16; kernels: apd_icp_batch.hpp)
constexpr int kIcbTraceCap = 1024;  // a pair's trace keeps its first this many iterations (the count goes on)

// IC13 / IC15: the loop of every pair on the device; returns with the device records complete
int icb_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs) {
  Engine& e = b->eng;
  IcbState& v = b->ic;
  v.have = false;
  if (n_pairs > 65535) return fail(APDGICP_ERR_INVALID_ARG, "point-to-point ICP: at most 65535 pairs per align (the pair is a grid dimension)");
  APD_TRY(e.finish_align());  // (an uncollected deferred align from before the mode was switched on)
  APD_TRY(e.setup_pairs(pairs, n_pairs, true, /*pipeline_cov=*/false, /*need_cov=*/false));  // clouds sorted, no covariances, the search buffers
  e.results_on_host = false;
  const int np = e.npairs, nstride = e.work.nstride, nblk_max = (e.nmax_src + IC_BLK - 1) / IC_BLK;
  const size_t nch_max = ((size_t)e.nmax_src + kChunk - 1) / kChunk, ngr_max = ((size_t)e.nmax_src + kGroupPts - 1) / kGroupPts;
  const long long bound = std::max(1, e.params.max_iterations);  // (max_iterations <= 1 still runs one iteration, as the single handle does)
  const int trace_cap = (int)std::min<long long>(bound, kIcbTraceCap);
  v.src.resize(np), v.tgt.resize(np), v.n_src.resize(np), v.w_off.resize(np);
  size_t total = 0;
  for (int i = 0; i < np; i++) {
    v.src[i] = e.h_pairs[i].src, v.tgt[i] = e.h_pairs[i].tgt, v.n_src[i] = e.clouds[v.src[i]].n;
    v.w_off[i] = total;
    total += (size_t)v.n_src[i];
  }
  const bool recip = v.prm.use_reciprocal_correspondences != 0;
  struct Want {
    DevBuf* buf;
    size_t bytes;
  };
  const Want wants[] = {{&v.W, total * 16},
                        {&v.cbox, recip ? (size_t)np * nch_max * sizeof(Box) : 0},
                        {&v.gbox, recip ? (size_t)np * ngr_max * sizeof(Box) : 0},
                        {&v.beaten, recip ? (size_t)np * nstride : 0},
                        {&v.match, (size_t)np * nstride * 4},
                        {&v.dsq, (size_t)np * nstride * 4},
                        {&v.part, (size_t)np * nblk_max * IC_R2 * 8},
                        {&v.sum1, (size_t)np * IC_R1 * 8},
                        {&v.rec, (size_t)np * sizeof(IcpRecord)},
                        {&v.aux, (size_t)np * sizeof(IcbAux)},
                        {&v.trace, (size_t)np * trace_cap * sizeof(IcbTrace)},
                        {&v.guess, (size_t)np * 16 * sizeof(float)}};
  bool grows = false;
  for (const Want& w : wants) grows |= w.bytes > w.buf->cap;
  if (grows) APD_HIP(hipStreamSynchronize(e.stream));  // (getters of the last align may still read the old buffers)
  for (const Want& w : wants) APD_TRY(w.buf->ensure(w.bytes));
  v.nstride = nstride, v.trace_cap = trace_cap;
  std::vector<IcbPair> tab(np);
  std::vector<PairDesc> nn(np);
  for (int i = 0; i < np; i++) {
    const Engine::Cloud& s = e.clouds[v.src[i]];
    float4* W = v.W.as<float4>() + v.w_off[i];
    tab[i] = IcbPair{s.pts.as<float4>(), s.perm.as<int>(), W, recip ? v.cbox.as<Box>() + (size_t)i * nch_max : nullptr, recip ? v.gbox.as<Box>() + (size_t)i * ngr_max : nullptr,
                     s.n, 0};
    nn[i] = e.h_pairs[i];
    nn[i].s.pts = W;  // IC12: the search sees W itself at the identity pose
  }
  APD_TRY(v.pairs.upload(tab.data(), tab.size() * sizeof(IcbPair), e.stream));
  APD_TRY(v.nn_pairs.upload(nn.data(), nn.size() * sizeof(PairDesc), e.stream));
  APD_HIP(hipMemcpyAsync(v.guess.p, e.h_guesses.data(), (size_t)np * 16 * sizeof(float), hipMemcpyHostToDevice, e.stream));  // (pageable source: staged before the call returns)
  APD_TRY(device_loop_prepare(b));
  const IcpConsts c = ic_consts(e.params, v.prm, 1);
  const int xf = (e.params.flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0;
  // the engine's search with this mode's inputs, for the length of this call: W as the source, the distances kept, no keeping, no timing
  struct SearchScope {
    Engine& e;
    float* sqd;
    bool profile;
    int active;
    ~SearchScope() { e.pairs_override = nullptr, e.work.sqd = sqd, e.profile_nn = profile, e.cur_active = active; }
  } scope{e, e.work.sqd, e.profile_nn, e.cur_active};
  e.pairs_override = v.nn_pairs.as<PairDesc>();
  e.work.sqd = e.b_sqd.as<float>();
  e.profile_nn = false, e.cur_active = 0;
  const IcbTab t{v.pairs.as<IcbPair>(), e.d_state.as<PairState>(), v.rec.as<IcpRecord>(), v.aux.as<IcbAux>(), v.trace.as<IcbTrace>(), e.work.nnpt, e.work.sqd,
                 v.match.as<int>(), v.dsq.as<float>(), v.beaten.as<unsigned char>(), v.part.as<double>(), v.sum1.as<double>(), nstride, nblk_max, trace_cap, 0};
  ResultRec* recs = e.d_results.as<ResultRec>();
  int* done = b->loop.done.as<int>();
  const dim3 grid_pts((unsigned)nblk_max, (unsigned)np), grid_w((unsigned)((e.nmax_src + 255) / 256), (unsigned)np);
  int tick = 0, rc_tick = 0;
  const int per_tick = 2 + (recip ? (v.brute ? 1 : 3) : 0) + 5;
  const int rc = device_loop_run(
      b, bound,
      [&]() {
        hipLaunchKernelGGL(k_icb_init, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, e.stream, t, v.guess.as<float>(), np, done);
        hipLaunchKernelGGL(k_icb_winit, grid_w, dim3(256), 0, e.stream, t.pairs, v.guess.as<float>(), xf);
      },
      [&]() {
        if (rc_tick == 0) rc_tick = e.launch_nn(e.whole());
        if (rc_tick == 0) rc_tick = e.launch_linearize(e.whole(), 0);  // (the per-point pass that settles the exact index: Work::nnpt, Work::sqd)
        if (recip && !v.brute) {
          hipLaunchKernelGGL(k_icb_boxes, dim3((unsigned)((nch_max + 255) / 256), (unsigned)np), dim3(256), 0, e.stream, t, 0);
          hipLaunchKernelGGL(k_icb_boxes, dim3((unsigned)((ngr_max + 255) / 256), (unsigned)np), dim3(256), 0, e.stream, t, 1);
          hipLaunchKernelGGL(k_icb_recip<true>, grid_pts, dim3(IC_BLK), 0, e.stream, t, c.thr2);
        } else if (recip) {
          hipLaunchKernelGGL(k_icb_recip<false>, grid_pts, dim3(IC_BLK), 0, e.stream, t, c.thr2);
        }
        hipLaunchKernelGGL(k_icb_pairs, grid_pts, dim3(IC_BLK), 0, e.stream, t, recip ? 1 : 0, c.thr2);
        hipLaunchKernelGGL(k_icb_sums, dim3((unsigned)np), dim3(64), 0, e.stream, t);
        hipLaunchKernelGGL(k_icb_cross, grid_pts, dim3(IC_BLK), 0, e.stream, t);
        hipLaunchKernelGGL(k_icb_step, dim3((unsigned)np), dim3(64), 0, e.stream, t, c, tick, recs, done);
        hipLaunchKernelGGL(k_icb_transform, grid_w, dim3(256), 0, e.stream, t, tick, xf);  // IC1: once per iteration, the last included
        tick++;
      });
  APD_TRY(rc);
  APD_TRY(rc_tick);
  v.ticks = b->loop.last_ticks, v.waits = b->loop.last_waits;
  v.launches = 2 + (int64_t)v.ticks * per_tick;
  v.have = true, v.have_epoch = e.pts_epoch;
  return 0;
}

// the last align in this mode must still describe the slots as they are
int icb_check_have(apdgicp_batch* b, int64_t pair) {
  const IcbState& v = b->ic;
  if (b->mode != Mode::ICP) return mode_is_off(Mode::ICP, true);
  if (!v.have || v.have_epoch != b->eng.pts_epoch) return fail(APDGICP_ERR_NO_INPUT, "no align in this mode of the clouds the handle holds now");
  if (pair < 0 || pair >= (int64_t)v.src.size()) return fail(APDGICP_ERR_INVALID_ARG, "pair is not one of the last align");
  return 0;
}

// what the single and the batch setters refuse (null: nothing to check -- the mode is being switched off)
int check_vgicp_params(const apdgicp_vgicp_params* p) {
  if (!p) return 0;
  if (!(p->resolution > 0.0) || !std::isfinite(p->resolution)) return fail(APDGICP_ERR_INVALID_ARG, "voxelized GICP: the resolution must be finite and positive");
  if (p->neighbor_search < APDGICP_VGICP_DIRECT1 || p->neighbor_search > APDGICP_VGICP_DIRECT27) return fail(APDGICP_ERR_INVALID_ARG, "voxelized GICP: unknown neighbour search method");
  if (p->voxel_mode == APDGICP_VGICP_MULTIPLICATIVE) return fail(APDGICP_ERR_UNSUPPORTED, "voxelized GICP: MULTIPLICATIVE accumulation is not offered");
  if (p->voxel_mode != APDGICP_VGICP_ADDITIVE && p->voxel_mode != APDGICP_VGICP_ADDITIVE_WEIGHTED) return fail(APDGICP_ERR_INVALID_ARG, "voxelized GICP: unknown accumulation mode");
  return 0;
}

int check_ndt_params(const apdgicp_ndt_params* p) {
  if (!p) return 0;
  if (!(p->resolution > 0.0) || !std::isfinite(p->resolution)) return fail(APDGICP_ERR_INVALID_ARG, "NDT: the resolution must be finite and positive");
  if (p->distance_mode != APDGICP_NDT_P2D && p->distance_mode != APDGICP_NDT_D2D) return fail(APDGICP_ERR_INVALID_ARG, "NDT: unknown distance mode");
  if (p->neighbor_search == APDGICP_NDT_DIRECT_RADIUS) return fail(APDGICP_ERR_UNSUPPORTED, "NDT: DIRECT_RADIUS neighbour search is not offered");
  if (p->neighbor_search < APDGICP_VGICP_DIRECT1 || p->neighbor_search > APDGICP_VGICP_DIRECT27) return fail(APDGICP_ERR_INVALID_ARG, "NDT: unknown neighbour search method");
  return 0;
}

// the pooled / deferred aligns of the APD path finish as what they were enqueued as; the chunk length of the device loop is read once
int batch_enter_device_loop_mode(apdgicp_batch* b) {
  if (b->eng.stream) {
    APD_TRY(b->eng.pool_leave());
    APD_TRY(b->eng.finish_align());
  }
  if (!b->loop.chunk) b->loop.chunk = std::max(1, std::min(1024, env_int("APDGICP_VGB_CHUNK", kVgbChunk)));
  return 0;
}

// The one writer of apdgicp_handle::mode, with every effect of leaving one mode and entering another ("Mode transitions").  A setter
// that changes the parameters of the mode that is already on does not come through here.
void set_mode(apdgicp_handle* h, Mode to) {
  const Mode from = h->mode;
  if (from == to) return;
  h->have_corr = false;  // (the APD kernels' correspondences are those of their own last linearize, and none is left)
  if (from == Mode::ICP || to == Mode::ICP) h->pair_ready = false;  // (the pair of the other side was set up with / without covariances)
  h->lin.have = false;  // (the one frozen state is the mode's that made it)
  if (to == Mode::VGICP_CUDA || to == Mode::NDT || to == Mode::GICP_MP) h->reset_final_H();
  if (from == Mode::GICP_MP || to == Mode::GICP_MP) {  // (what the mode's getters read is one visit's)
    MpState& v = h->mp;
    v.have = false, v.state = APDGICP_GICP_MP_NOT_CONVERGED, v.launches = v.waits = 0;
    v.tr_pose.clear(), v.tr_cost.clear(), v.tr_delta.clear(), v.tr_n.clear();
  }
  h->mode = to;  // (apdgicp_set_icp forgets the last estimate with every enabling call, entering or not)
}

// ... and of apdgicp_batch::mode.  Fails, with the mode unchanged, when the APD path's aligns in flight cannot be finished.
int set_mode(apdgicp_batch* b, Mode to) {
  const Mode from = b->mode;
  if (from == to) return 0;
  if (from == Mode::APD) APD_TRY(batch_enter_device_loop_mode(b));
  if (from == Mode::ICP) b->eng.poses_of_align = false;  // IC16: the engine's pair state holds that mode's identity poses, not an align's
  b->mode = to;  // (what the ICP and FAST_VGICP_CUDA getters may read goes with every enabling call of their setters, entering or not)
  return 0;
}

}  // namespace

extern "C" {

int apdgicp_abi_version(void) { return APDGICP_ABI_VERSION; }
// What this library was compiled with: the compiler flags build.py passed ("unknown" for a hand build), then " | variant:" and every
// experiment define that CHANGES RESULTS OR KERNELS -- detected here by the preprocessor, so no build script can leave one out.  A
// library that lists a variant is an ablation / A-B build (some are wrong by design): the Python loader and the C++ adapter's self-check
// refuse it unless APDGICP_ALLOW_VARIANT_LIB=1.
#ifndef APD_BUILD_FLAGS
#define APD_BUILD_FLAGS "unknown"
#endif
#define APD_STR2(x) #x
#define APD_STR(x) APD_STR2(x)
const char* apdgicp_build_flags(void) {
  return APD_BUILD_FLAGS " | variant:"
#ifdef APD_ABL_KNN_SKIP_C
      " APD_ABL_KNN_SKIP_C"
#endif
#ifdef APD_ABL_LM_NO_ERROR
      " APD_ABL_LM_NO_ERROR"
#endif
#ifdef APD_ABL_LIN_DOUBLE_ATAN
      " APD_ABL_LIN_DOUBLE_ATAN"
#endif
#ifdef APD_ABL_LIN_DOUBLE_SINCOS
      " APD_ABL_LIN_DOUBLE_SINCOS"
#endif
#ifdef APD_ABL_LIN_NO_ATAN
      " APD_ABL_LIN_NO_ATAN"
#endif
#ifdef APD_ABL_LIN_NO_SINCOS
      " APD_ABL_LIN_NO_SINCOS"
#endif
#ifdef APD_ABL_SEARCH_KEEP_AFTER
      " APD_ABL_SEARCH_KEEP_AFTER=" APD_STR(APD_ABL_SEARCH_KEEP_AFTER)
#endif
#ifdef APD_OCML_ATAN2F
      " APD_OCML_ATAN2F"
#endif
#ifdef APD_BLOCK_TIMELINE
      " APD_BLOCK_TIMELINE"
#endif
#ifdef APD_AB_NO_ASM_NOP
      " APD_AB_NO_ASM_NOP"
#endif
#ifdef APD_SINCOS_NO_TABLE
      " APD_SINCOS_NO_TABLE"
#endif
      ;
}
#ifndef APD_SOURCE_STAMP
#define APD_SOURCE_STAMP "unstamped"
#endif
// (build.py passes "apd-source-stamp:<16 hex digits>": the marker is what build.library_stamp() looks for in the file)
const char* apdgicp_source_stamp(void) {
  static const char stamp[] = APD_SOURCE_STAMP;
  const char* colon = strchr(stamp, ':');
  return colon ? colon + 1 : stamp;
}
const char* apdgicp_last_error(void) { return g_last_error.c_str(); }

int apdgicp_device_count(int* count) {
  if (!count) return fail(APDGICP_ERR_INVALID_ARG, "count is null");
  *count = 0;
  APD_HIP(hipGetDeviceCount(count));
  return 0;
}

void apdgicp_default_params(apdgicp_params* p) {
  if (!p) return;
  p->k_correspondences = 20;                 // A:21
  p->max_iterations = 64;                    // L:13
  p->lm_max_iterations = 10;                 // L:19
  p->optimizer = APDGICP_OPT_LM;             // L:17
  p->regularization = APDGICP_REG_PLANE;     // A:25
  p->flags = 0;
  p->max_correspondence_distance = (double)FLT_MAX;  // A:23
  p->transformation_epsilon = 5e-4;          // L:15
  p->rotation_epsilon = 2e-3;                // L:14
  p->lm_init_lambda_factor = 1e-9;           // L:20
  p->distance_variance = 0.86;               // H:109
  p->azimuth_variance_deg = 0.5;             // H:107
  p->elevation_variance_deg = 1.0;           // H:108
}

// ------------------------------------------------------------------------------------ single
int apdgicp_create(const apdgicp_params* p, int device, void* stream, apdgicp_handle** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_params dflt;
    apdgicp_default_params(&dflt);
    apdgicp_handle* h = new apdgicp_handle;
    const int rc = h->eng.init(p ? p : &dflt, device, stream);
    if (rc < 0) {
      delete h;
      return rc;
    }
    h->eng.clouds.resize(2);
    const char* recip_mode = getenv("APDGICP_ICP_RECIP_MODE");
    h->ic.brute = recip_mode && std::string(recip_mode) == "brute";
    *out = h;
    return 0;
  });
}

int apdgicp_destroy(apdgicp_handle* h) {
  delete h;
  return 0;
}

int apdgicp_set_params(apdgicp_handle* h, const apdgicp_params* p) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  return h->eng.set_params(p);
}

int apdgicp_get_params(const apdgicp_handle* h, apdgicp_params* p) {
  if (!h || !p) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *p = h->eng.params;
  return 0;
}

static int set_cloud_common(apdgicp_handle* h, int slot, const float* xyz, int64_t n, int64_t stride, int on_device, uint64_t token) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    Engine& e = h->eng;
    if (token != 0 && e.clouds[slot].n > 0 && e.clouds[slot].token == token) return 0;  // A:91-93 / A:102-104
    APD_TRY(e.set_cloud(slot, xyz, n, stride, on_device, token));
    h->pair_ready = false;
    h->have_corr = false;
    h->cloud_gen[slot] = ++h->cloud_epoch;
    return 0;
  });
}

int apdgicp_set_source(apdgicp_handle* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device, uint64_t token) {
  return set_cloud_common(h, kSrc, xyz, n, stride_bytes, on_device, token);
}
int apdgicp_set_target(apdgicp_handle* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device, uint64_t token) {
  return set_cloud_common(h, kTgt, xyz, n, stride_bytes, on_device, token);
}

int apdgicp_clear_source(apdgicp_handle* h) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  h->eng.clear_cloud(kSrc);
  h->pair_ready = h->have_corr = false;
  h->cloud_gen[kSrc] = ++h->cloud_epoch;
  return 0;
}
int apdgicp_clear_target(apdgicp_handle* h) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  h->eng.clear_cloud(kTgt);
  h->pair_ready = h->have_corr = false;
  h->cloud_gen[kTgt] = ++h->cloud_epoch;
  return 0;
}
int apdgicp_swap_source_and_target(apdgicp_handle* h) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  std::swap(h->eng.clouds[kSrc], h->eng.clouds[kTgt]);  // input_.swap(target_), covs swap, A:68-75
  h->eng.clouds_written();
  h->pair_ready = h->have_corr = false;
  std::swap(h->cloud_gen[kSrc], h->cloud_gen[kTgt]);
  std::swap(h->nd.maps[kSrc], h->nd.maps[kTgt]);  // NC:90-93: the NDT maps go with their clouds (tied to them by identity either way)
  std::swap(h->vc.pc[kSrc], h->vc.pc[kTgt]);  // VC:97-107: the prepared clouds go with their clouds; the map is then another target's and is rebuilt
  if (h->mode != Mode::VGICP) h->lin.have = false;  // (voxelized GICP tracks its frozen state by identity alone: a second swap makes it current again, V6)
  return 0;
}

int apdgicp_compute_covariances(apdgicp_handle* h, int which) {
  return guarded([&]() -> int {
    if (!h || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    return h->eng.compute_covariances({which});
  });
}

int apdgicp_get_covariances(apdgicp_handle* h, int which, double* out, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !out || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    Engine& e = h->eng;
    APD_TRY(e.compute_covariances({which}));
    Engine::Cloud& c = e.clouds[which];
    if (n != c.n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the cloud size");
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 16 * sizeof(double)));
    hipLaunchKernelGGL(k_unpack_cov, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, c.cov.as<double>(), c.perm.as<int>(), (int)n,
                       e.d_stage.as<double>());
    APD_HIP(hipMemcpyAsync(out, e.d_stage.p, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_set_covariances(apdgicp_handle* h, int which, const double* in, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !in || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    Engine& e = h->eng;
    Engine::Cloud& c = e.clouds[which];
    if (c.n <= 0) return fail(APDGICP_ERR_NO_INPUT, "cloud not set");
    if (n != c.n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the cloud size");
    APD_TRY(e.upload_desc());  // allocates c.cov
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 16 * sizeof(double)));
    APD_HIP(hipMemcpyAsync(e.d_stage.p, in, (size_t)n * 16 * sizeof(double), hipMemcpyHostToDevice, e.stream));
    hipLaunchKernelGGL(k_pack_cov, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, e.d_stage.as<double>(), c.perm.as<int>(), (int)n,
                       c.cov.as<double>());
    APD_HIP(hipStreamSynchronize(e.stream));
    c.cov_valid = true;
    c.cov_gen = ++e.cov_epoch;
    return 0;
  });
}

int apdgicp_linearize(apdgicp_handle* h, const double T[16], double H[36], double b[6], double* cost) {
  return guarded([&]() -> int {
    if (!h || !T) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    switch (h->mode) {
      case Mode::ICP: return fail(APDGICP_ERR_UNSUPPORTED, kIcNoLinearize);
      case Mode::GICP_MP: return mp_linearize(h, T, H, b, cost, nullptr);
      case Mode::NDT: return nd_linearize(h, T, H, b, cost, nullptr);
      case Mode::VGICP: return vg_linearize(h, T, H, b, cost, nullptr);
      case Mode::VGICP_CUDA: return vc_linearize(h, T, H, b, cost, nullptr);
      case Mode::APD: break;
    }
    APD_TRY(ensure_pair(h));
    APD_TRY(h->eng.probe_linearize(T, H, b, cost, nullptr));
    h->have_corr = true;
    return 0;
  });
}

int apdgicp_compute_error(apdgicp_handle* h, const double T[16], double* cost) {
  return guarded([&]() -> int {
    if (!h || !T || !cost) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    switch (h->mode) {
      case Mode::ICP: return fail(APDGICP_ERR_UNSUPPORTED, kIcNoLinearize);
      case Mode::GICP_MP: return fail(APDGICP_ERR_UNSUPPORTED, "FastGICPMultiPoints has no compute_error: its loop is plain Gauss-Newton (MP7)");
      case Mode::NDT: return nd_error(h, T, cost);
      case Mode::VGICP: return vg_error(h, T, cost);
      case Mode::VGICP_CUDA: return vc_error(h, T, cost);
      case Mode::APD: break;
    }
    if (!h->pair_ready || !h->have_corr) return fail(APDGICP_ERR_NO_INPUT, "compute_error needs a previous linearize");
    return h->eng.probe_error(T, cost);
  });
}

int apdgicp_get_correspondences(apdgicp_handle* h, int32_t* corr, float* sq, int64_t n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    switch (h->mode) {
      case Mode::ICP: return fail(APDGICP_ERR_UNSUPPORTED, "point-to-point ICP keeps its own correspondences: apdgicp_icp_get_correspondences");
      case Mode::GICP_MP: return fail(APDGICP_ERR_UNSUPPORTED, "FastGICPMultiPoints has a row of correspondences per point: apdgicp_gicp_mp_get_rows");
      case Mode::NDT: return fail(APDGICP_ERR_UNSUPPORTED, "NDT has no point correspondences: apdgicp_ndt_get_correspondences");
      case Mode::VGICP: return fail(APDGICP_ERR_UNSUPPORTED, "voxelized GICP has no point correspondences: apdgicp_vgicp_get_correspondences");
      case Mode::VGICP_CUDA: return fail(APDGICP_ERR_UNSUPPORTED, "FAST_VGICP_CUDA has no point correspondences: apdgicp_vgicp_cuda_get_correspondences");
      case Mode::APD: break;
    }
    Engine& e = h->eng;
    if (!h->pair_ready || !h->have_corr) return fail(APDGICP_ERR_NO_INPUT, "no correspondences yet");
    if (n != e.clouds[kSrc].n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 8));
    int* d_c = e.d_stage.as<int>();
    float* d_s = (float*)(d_c + n);
    hipLaunchKernelGGL(k_export_corr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, e.work.corr, e.work.sqd, e.clouds[kSrc].perm.as<int>(),
                       e.clouds[kTgt].perm.as<int>(), (int)n, d_c, d_s);
    if (corr) APD_HIP(hipMemcpyAsync(corr, d_c, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    if (sq) APD_HIP(hipMemcpyAsync(sq, d_s, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_get_mahalanobis(apdgicp_handle* h, double* out, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::APD) return fail(APDGICP_ERR_UNSUPPORTED, std::string(kModeText[(int)h->mode].name) + " keeps no per-point Mahalanobis matrices");
    Engine& e = h->eng;
    if (!h->pair_ready || !h->have_corr) return fail(APDGICP_ERR_NO_INPUT, "no correspondences yet");
    if (n != e.clouds[kSrc].n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
    const size_t ns = e.work.nstride;
    std::vector<double> m6(6 * ns);
    std::vector<int> corr(n), perm(n);
    APD_HIP(hipMemcpyAsync(m6.data(), e.work.maha, 6 * ns * sizeof(double), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipMemcpyAsync(corr.data(), e.work.corr, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipMemcpyAsync(perm.data(), e.clouds[kSrc].perm.p, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    for (int64_t i = 0; i < n; i++) {  // i = position on the Z-curve, perm[i] = the caller's index
      double* o = out + 16 * perm[i];
      memset(o, 0, 16 * sizeof(double));
      if (corr[i] < 0) continue;
      const double xx = m6[i], xy = m6[ns + i], xz = m6[2 * ns + i], yy = m6[3 * ns + i], yz = m6[4 * ns + i], zz = m6[5 * ns + i];
      o[0] = xx, o[1] = xy, o[2] = xz, o[4] = xy, o[5] = yy, o[6] = yz, o[8] = xz, o[9] = yz, o[10] = zz;  // (3,3) = 0, A:192
    }
    return 0;
  });
}

int apdgicp_align(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  return guarded([&]() -> int {
    if (!h || !out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::APD) return mode_align(h, guess, out);
    float g[16];
    if (guess) memcpy(g, guess, sizeof(g));
    else identity16(g);
    Engine& e = h->eng;
    struct Fuse {  // the covariance launch of freshly set clouds goes out with the first tick's search (k_knn_and_search)
      Engine& e;
      explicit Fuse(Engine& e_) : e(e_) { e.fuse_first_search = true; }
      ~Fuse() {
        e.fuse_first_search = false;
        (void)e.flush_pending_knn();  // (only after an error on the way: nothing stays pending)
      }
    } fuse(e);
    APD_TRY(ensure_pair(h, g));
    APD_TRY(e.upload_guesses(g, 1));  // no-op when ensure_pair has just uploaded it
    APD_TRY(e.run_align());
    h->trace_from_host_loop = false;
    if (const ResultRec* r = e.host_results()) {  // came home with the last poll
      memcpy(out, r, sizeof(apdgicp_result));
    } else {
      APD_HIP(hipMemcpyAsync(out, e.d_results.p, sizeof(apdgicp_result), hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
    }
    h->have_corr = out->n_linearize > 0;
    return 0;
  });
}

// The reference's own control flow (L:55-173) on the host, calling the device through the same two
// virtuals the reference uses (linearize, compute_error).  Used to separate "kernel parity" from
// "state-machine parity" in the tests.
int apdgicp_align_host_loop(apdgicp_handle* h, const float guess[16], apdgicp_result* out) {
  return guarded([&]() -> int {
    if (!h || !out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::APD) return mode_align(h, guess, out);
    APD_TRY(ensure_pair(h));
    Engine& e = h->eng;
    return host_loop(
        h, guess, out, [&](const double* T, double* H, double* b, double* y0, int* m) { return e.probe_linearize(T, H, b, y0, m); },
        [&](const double* T, double* yi) { return e.probe_error(T, yi); }, false);
  });
}

// ------------------------------------------------------------------------------------ voxelized GICP
void apdgicp_vgicp_default_params(apdgicp_vgicp_params* p) {
  if (!p) return;
  p->resolution = 1.0;                          // V:22
  p->neighbor_search = APDGICP_VGICP_DIRECT1;   // V:23
  p->voxel_mode = APDGICP_VGICP_ADDITIVE;       // V:24
}

int apdgicp_set_vgicp(apdgicp_handle* h, const apdgicp_vgicp_params* p) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  VgState& v = h->vg;
  if (!p) {  // back to the APD-GICP / plain GICP kernels (a no-op while another mode is on)
    if (h->mode == Mode::VGICP) set_mode(h, Mode::APD);
    return 0;
  }
  APD_TRY(check_vgicp_params(p));
  if (p->resolution != v.prm.resolution || p->voxel_mode != v.prm.voxel_mode || p->neighbor_search != v.prm.neighbor_search) h->lin.have = false;
  v.prm = *p;
  set_mode(h, Mode::VGICP);
  return 0;
}

int apdgicp_get_vgicp(const apdgicp_handle* h, apdgicp_vgicp_params* p, int* enabled) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (p) *p = h->vg.prm;
  if (enabled) *enabled = h->mode == Mode::VGICP ? 1 : 0;
  return 0;
}

int apdgicp_vgicp_voxel_count(apdgicp_handle* h, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!h || !n_voxels) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::VGICP) return mode_is_off(Mode::VGICP, false);
    APD_TRY(vg_build_map(h));
    *n_voxels = h->vg.n_vox;
    return 0;
  });
}

int apdgicp_vgicp_get_voxels(apdgicp_handle* h, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    if (h->mode != Mode::VGICP) return mode_is_off(Mode::VGICP, false);
    APD_TRY(vg_build_map(h));
    return read_voxels(h->eng.stream, h->vg.buf, h->vg.n_vox, capacity, coords_n3, counts, means_n3, nullptr, covs_n9);
  });
}

int apdgicp_vgicp_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_source) {
  return guarded([&]() -> int {
    if (!h || !voxel_index) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::VGICP) return mode_is_off(Mode::VGICP, false);
    if (!h->lin.have || h->vg.lin_src_gen != h->cloud_gen[kSrc]) return fail(APDGICP_ERR_NO_INPUT, "no correspondences yet");
    return read_frozen_corr(h->eng, h->lin, voxel_index, n_source, "n_source does not match the source size");
  });
}

int apdgicp_vgicp_build_count(apdgicp_handle* h, int64_t* n_builds) {
  if (!h || !n_builds) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n_builds = h->vg.builds;
  return 0;
}

// ------------------------------------------------------------------------------------ FAST_VGICP_CUDA
void apdgicp_vgicp_cuda_default_params(apdgicp_vgicp_cuda_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->resolution = 1.0;                                 // VCI:24
  p->neighbor_search = APDGICP_VGICP_DIRECT1;          // VC:28
  p->search_radius = 1.5;                              // (pygicp's default for DIRECT_RADIUS)
  p->regularization = APDGICP_REG_PLANE;               // VCI:26
  p->nn_method = APDGICP_NN_CPU_PARALLEL_KDTREE;       // VCI:27
}

int apdgicp_set_vgicp_cuda(apdgicp_handle* h, const apdgicp_vgicp_cuda_params* p) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  VcState& v = h->vc;
  if (!p) {  // back to what apdgicp_params says (a no-op while another mode is on)
    if (h->mode == Mode::VGICP_CUDA) set_mode(h, Mode::APD);
    return 0;
  }
  APD_TRY(check_vgicp_cuda_params(p));
  const bool same_offsets = p->neighbor_search == v.prm.neighbor_search && (p->neighbor_search != APDGICP_VGICP_CUDA_DIRECT_RADIUS || p->search_radius == v.prm.search_radius);
  if (p->resolution != v.prm.resolution || p->regularization != v.prm.regularization || !same_offsets) h->lin.have = false;
  if (!same_offsets) v.offs.clear();
  v.prm = *p;
  set_mode(h, Mode::VGICP_CUDA);
  return 0;
}

int apdgicp_get_vgicp_cuda(const apdgicp_handle* h, apdgicp_vgicp_cuda_params* p, int* enabled) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (p) *p = h->vc.prm;
  if (enabled) *enabled = h->mode == Mode::VGICP_CUDA ? 1 : 0;
  return 0;
}

int apdgicp_vgicp_cuda_offsets(const apdgicp_vgicp_cuda_params* p, int32_t* out_n3, int64_t* n) {
  return guarded([&]() -> int {
    if (!p || !n) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(check_vgicp_cuda_params(p));
    std::vector<int32_t> offs;
    vc_offsets(*p, offs);
    *n = (int64_t)(offs.size() / 3);
    if (out_n3) memcpy(out_n3, offs.data(), offs.size() * sizeof(int32_t));
    return 0;
  });
}

int apdgicp_vgicp_cuda_kept(apdgicp_handle* h, int which, int64_t* n_kept, int32_t* kept_index, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h || !n_kept || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (h->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, false);
    APD_TRY(vc_prepare_cloud(h, which));
    return read_kept(h->eng.stream, h->vc.pc[which], n_kept, kept_index, capacity);
  });
}

int apdgicp_vgicp_cuda_get_covariances(apdgicp_handle* h, int which, double* raw_n6, double* reg_n9, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (h->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, false);
    APD_TRY(vc_prepare_cloud(h, which));
    return read_prepared_covariances(h->eng.stream, h->vc.pc[which], raw_n6, reg_n9, capacity);
  });
}

int apdgicp_vgicp_cuda_voxel_count(apdgicp_handle* h, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!h || !n_voxels) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, false);
    APD_TRY(vc_build_map(h));
    *n_voxels = h->vc.n_vox;
    return 0;
  });
}

int apdgicp_vgicp_cuda_get_voxels(apdgicp_handle* h, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    if (h->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, false);
    APD_TRY(vc_build_map(h));
    if (h->vc.n_vox == 0) return 0;
    return read_voxels(h->eng.stream, h->vc.buf, h->vc.n_vox, capacity, coords_n3, counts, means_n3, nullptr, covs_n9);
  });
}

int apdgicp_vgicp_cuda_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_kept_source) {
  return guarded([&]() -> int {
    if (!h || !voxel_index) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, false);
    if (!vc_frozen_ok(h)) return fail(APDGICP_ERR_NO_INPUT, "no correspondences yet");
    return read_frozen_corr(h->eng, h->lin, voxel_index, n_kept_source, "n_kept_source does not match the kept source size");
  });
}

int apdgicp_vgicp_cuda_build_count(apdgicp_handle* h, int64_t* n_builds) {
  if (!h || !n_builds) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n_builds = h->vc.builds;
  return 0;
}

// ------------------------------------------------------------------------------------ NDT
void apdgicp_ndt_default_params(apdgicp_ndt_params* p) {
  if (!p) return;
  p->resolution = 1.0;                          // NC:15
  p->distance_mode = APDGICP_NDT_D2D;           // NC:16
  p->neighbor_search = APDGICP_VGICP_DIRECT7;   // NC:17
}

int apdgicp_set_ndt(apdgicp_handle* h, const apdgicp_ndt_params* p) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  NdState& v = h->nd;
  if (!p) {  // back to what apdgicp_params says (a no-op while another mode is on)
    if (h->mode == Mode::NDT) set_mode(h, Mode::APD);
    return 0;
  }
  APD_TRY(check_ndt_params(p));
  if (p->resolution != v.prm.resolution || p->distance_mode != v.prm.distance_mode || p->neighbor_search != v.prm.neighbor_search) h->lin.have = false;
  v.prm = *p;
  set_mode(h, Mode::NDT);
  return 0;
}

// ------------------------------------------------------------------------------------ point-to-point ICP
void apdgicp_icp_default_params(apdgicp_icp_params* p) {
  if (!p) return;
  p->enable = 1;
  p->use_reciprocal_correspondences = 0;   // pcl::IterativeClosestPoint: use_reciprocal_correspondence_(false)
  p->min_correspondences = 3;              // pcl::Registration: min_number_correspondences_(3)
  p->max_similar_transforms = 0;           // DefaultConvergenceCriteria: max_iterations_similar_transforms_(0)
  p->euclidean_fitness_epsilon = -std::numeric_limits<double>::max();  // pcl::Registration: euclidean_fitness_epsilon_
  p->rotation_epsilon = 0.0;               // pcl::Registration: transformation_rotation_epsilon_(0.0)
  p->mse_threshold_absolute = 1e-12;       // DefaultConvergenceCriteria: mse_threshold_absolute_(1e-12)
}

int apdgicp_set_icp(apdgicp_handle* h, const apdgicp_icp_params* p) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  IcState& v = h->ic;
  APD_TRY(check_icp_params(p));
  if (p) v.prm = *p;
  if (!p || !p->enable) {  // (a no-op while another mode is on)
    if (h->mode == Mode::ICP) set_mode(h, Mode::APD);
    return 0;
  }
  set_mode(h, Mode::ICP);
  v.have = false, v.state = APDGICP_ICP_NOT_CONVERGED;  // (of every enabling call: what the last estimate or align left is not this setting's)
  return 0;
}

int apdgicp_get_icp(const apdgicp_handle* h, apdgicp_icp_params* p, int* enabled) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (p) {
    *p = h->ic.prm;
    p->enable = h->mode == Mode::ICP ? 1 : 0;
  }
  if (enabled) *enabled = h->mode == Mode::ICP ? 1 : 0;
  return 0;
}

int apdgicp_icp_estimate(apdgicp_handle* h, const float T[16], float T_out[16], int64_t* n_corr, double* mse, double sums[16]) {
  return guarded([&]() -> int {
    if (!h || !T) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::ICP) return mode_is_off(Mode::ICP, false);
    return ic_estimate(h, T, T_out, n_corr, mse, sums);
  });
}

// the last estimate / align must still describe the clouds the handle holds
static int ic_check_have(apdgicp_handle* h, int64_t n) {
  const IcState& v = h->ic;
  if (h->mode != Mode::ICP) return mode_is_off(Mode::ICP, false);
  if (!v.have || v.have_src_gen != h->cloud_gen[kSrc] || v.have_tgt_gen != h->cloud_gen[kTgt] || h->eng.clouds[kSrc].n != v.n_have)
    return fail(APDGICP_ERR_NO_INPUT, "no estimate or align of the clouds the handle holds now");
  if (n != v.n_have) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
  return 0;
}

int apdgicp_icp_get_correspondences(apdgicp_handle* h, int32_t* match, float* sq_dist, int64_t n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    APD_TRY(ic_check_have(h, n));
    Engine& e = h->eng;
    IcState& v = h->ic;
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 8));
    int* d_c = e.d_stage.as<int>();
    float* d_s = (float*)(d_c + n);
    hipLaunchKernelGGL(k_icp_export, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, v.match.as<int>(), v.dsq.as<float>(), e.clouds[kSrc].perm.as<int>(),
                       e.clouds[kTgt].perm.as<int>(), (int)n, d_c, d_s);
    APD_HIP(hipGetLastError());
    if (match) APD_HIP(hipMemcpyAsync(match, d_c, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    if (sq_dist) APD_HIP(hipMemcpyAsync(sq_dist, d_s, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_icp_get_working_cloud(apdgicp_handle* h, float* xyz, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !xyz) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(ic_check_have(h, n));
    Engine& e = h->eng;
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 12));
    hipLaunchKernelGGL(k_icp_export_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, h->ic.W.as<float4>(), e.clouds[kSrc].perm.as<int>(), (int)n,
                       e.d_stage.as<float>());
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(xyz, e.d_stage.p, (size_t)n * 12, hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_icp_get_trace(apdgicp_handle* h, int64_t capacity, float* T_k16, int64_t* n_corr, double* mse, int32_t* similar, int64_t* n_iterations) {
  return guarded([&]() -> int {
    if (!h || !n_iterations || capacity < 0) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    const IcState& v = h->ic;
    *n_iterations = (int64_t)v.tr_n.size();
    const int64_t m = std::min<int64_t>(*n_iterations, capacity);
    if (m && T_k16) memcpy(T_k16, v.tr_T.data(), m * 16 * sizeof(float));
    if (m && n_corr) memcpy(n_corr, v.tr_n.data(), m * sizeof(int64_t));
    if (m && mse) memcpy(mse, v.tr_mse.data(), m * sizeof(double));
    if (m && similar) memcpy(similar, v.tr_sim.data(), m * sizeof(int32_t));
    return 0;
  });
}

int apdgicp_icp_convergence_state(apdgicp_handle* h, int32_t* state) {
  if (!h || !state) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *state = h->ic.state;
  return 0;
}

int apdgicp_icp_debug_counts(apdgicp_handle* h, int64_t* launches, int64_t* waits) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (launches) *launches = h->ic.launches;
  if (waits) *waits = h->ic.waits;
  return 0;
}

// ------------------------------------------------------------------------------------ FastGICPMultiPoints
void apdgicp_gicp_mp_default_params(apdgicp_gicp_mp_params* p) {
  if (!p) return;
  p->enable = 1;
  p->reserved = 0;
  p->neighbor_search_radius = 0.5;  // MPI:35
}

int apdgicp_set_gicp_mp(apdgicp_handle* h, const apdgicp_gicp_mp_params* p) {
  APD_TRY(check_gicp_mp_params(p));  // (before the handle: what can be said about the parameters alone)
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  MpState& v = h->mp;
  if (!p || !p->enable) {  // (a no-op while another mode is on)
    if (p) v.prm = *p;
    if (h->mode == Mode::GICP_MP) set_mode(h, Mode::APD);
    return 0;
  }
  APD_TRY(mp_check_regularization(h));  // MP1: refused with nothing changed
  if (p->neighbor_search_radius != v.prm.neighbor_search_radius) v.have = false;
  v.prm = *p;
  set_mode(h, Mode::GICP_MP);
  return 0;
}

int apdgicp_get_gicp_mp(const apdgicp_handle* h, apdgicp_gicp_mp_params* p, int* enabled) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (p) {
    *p = h->mp.prm;
    p->enable = h->mode == Mode::GICP_MP ? 1 : 0;
  }
  if (enabled) *enabled = h->mode == Mode::GICP_MP ? 1 : 0;
  return 0;
}

// the last linearize must still describe the clouds the handle holds
static int mp_check_have(apdgicp_handle* h, int64_t n) {
  const MpState& v = h->mp;
  if (h->mode != Mode::GICP_MP) return mode_is_off(Mode::GICP_MP, false);
  if (!v.have || v.have_src_gen != h->cloud_gen[kSrc] || v.have_tgt_gen != h->cloud_gen[kTgt] || h->eng.clouds[kSrc].n != v.n_have)
    return fail(APDGICP_ERR_NO_INPUT, "no linearize of the clouds the handle holds now");
  if (n != v.n_have) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
  return 0;
}

int apdgicp_gicp_mp_get_rows(apdgicp_handle* h, int64_t* row_start, int64_t n, int64_t* total) {
  return guarded([&]() -> int {
    if (!h || !row_start || !total) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(mp_check_have(h, n));
    Engine& e = h->eng;
    std::vector<int> cnt((size_t)n);
    APD_HIP(hipSetDevice(e.device));
    APD_HIP(hipMemcpyAsync(cnt.data(), h->mp.cnt.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    int64_t sum = 0;
    for (int64_t i = 0; i < n; i++) row_start[i] = sum, sum += cnt[(size_t)i];
    row_start[n] = sum;
    if (sum != h->mp.total) return fail(APDGICP_ERR_INTERNAL, "FastGICPMultiPoints: inconsistent row lengths");
    *total = sum;
    return 0;
  });
}

int apdgicp_gicp_mp_get_row_entries(apdgicp_handle* h, int32_t* index, float* sq_dist) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    APD_TRY(mp_check_have(h, h->mp.n_have));
    const MpState& v = h->mp;
    if (v.total == 0) return 0;
    if (!index || !sq_dist) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = h->eng;
    APD_HIP(hipSetDevice(e.device));
    std::vector<unsigned long long> keys((size_t)v.total);  // (the rows lie one behind the other in the caller's source order)
    APD_HIP(hipMemcpyAsync(keys.data(), v.keys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    for (size_t i = 0; i < keys.size(); i++) {
      const uint32_t bits = (uint32_t)(keys[i] >> 32);
      index[i] = (int32_t)(uint32_t)keys[i];
      memcpy(&sq_dist[i], &bits, 4);
    }
    return 0;
  });
}

int apdgicp_gicp_mp_get_fused(apdgicp_handle* h, double* sum_w, double* mean_B, double* cov_B, int64_t n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    APD_TRY(mp_check_have(h, n));
    Engine& e = h->eng;
    APD_HIP(hipSetDevice(e.device));
    std::vector<double> f((size_t)n * MP_FUSED);
    APD_HIP(hipMemcpyAsync(f.data(), h->mp.fused.p, f.size() * sizeof(double), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    for (int64_t i = 0; i < n; i++) {
      const double* r = &f[(size_t)i * MP_FUSED];
      if (sum_w) sum_w[i] = r[0];
      if (mean_B) memcpy(mean_B + 3 * i, r + 1, 3 * sizeof(double));
      if (cov_B) memcpy(cov_B + 6 * i, r + 4, 6 * sizeof(double));
    }
    return 0;
  });
}

int apdgicp_gicp_mp_get_trace(apdgicp_handle* h, int64_t capacity, double* pose16, double* cost, int64_t* n_matched, double* delta6, int64_t* n_iterations) {
  return guarded([&]() -> int {
    if (!h || !n_iterations || capacity < 0) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (h->mode != Mode::GICP_MP) return mode_is_off(Mode::GICP_MP, false);
    const MpState& v = h->mp;
    *n_iterations = (int64_t)v.tr_n.size();
    const int64_t m = std::min<int64_t>(*n_iterations, capacity);
    if (m && pose16) memcpy(pose16, v.tr_pose.data(), m * 16 * sizeof(double));
    if (m && cost) memcpy(cost, v.tr_cost.data(), m * sizeof(double));
    if (m && n_matched) memcpy(n_matched, v.tr_n.data(), m * sizeof(int64_t));
    if (m && delta6) memcpy(delta6, v.tr_delta.data(), m * 6 * sizeof(double));
    return 0;
  });
}

int apdgicp_gicp_mp_state(apdgicp_handle* h, int32_t* state) {
  if (!h || !state) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  if (h->mode != Mode::GICP_MP) return mode_is_off(Mode::GICP_MP, false);
  *state = h->mp.state;
  return 0;
}

int apdgicp_gicp_mp_debug_counts(apdgicp_handle* h, int64_t* launches, int64_t* waits) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (h->mode != Mode::GICP_MP) return mode_is_off(Mode::GICP_MP, false);
  if (launches) *launches = h->mp.launches;
  if (waits) *waits = h->mp.waits;
  return 0;
}

int apdgicp_gicp_mp_set_profiling(apdgicp_handle* h, int enable) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  h->mp.profiling = enable != 0;
  return 0;
}

int apdgicp_gicp_mp_last_phases(apdgicp_handle* h, double ms[6]) {
  if (!h || !ms) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  if (h->mode != Mode::GICP_MP) return mode_is_off(Mode::GICP_MP, false);
  if (!h->mp.profiling || !h->mp.have) return fail(APDGICP_ERR_NO_INPUT, "no profiled linearize (apdgicp_gicp_mp_set_profiling)");
  memcpy(ms, h->mp.phase_ms, sizeof(h->mp.phase_ms));
  return 0;
}

int apdgicp_get_ndt(const apdgicp_handle* h, apdgicp_ndt_params* p, int* enabled) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  if (p) *p = h->nd.prm;
  if (enabled) *enabled = h->mode == Mode::NDT ? 1 : 0;
  return 0;
}

int apdgicp_ndt_voxel_count(apdgicp_handle* h, int which, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!h || !n_voxels || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (h->mode != Mode::NDT) return mode_is_off(Mode::NDT, false);
    APD_TRY(nd_build_map(h, which));
    *n_voxels = h->nd.maps[which].nv;
    return 0;
  });
}

int apdgicp_ndt_get_voxels(apdgicp_handle* h, int which, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* raw_covs_n6, double* covs_n9) {
  return guarded([&]() -> int {
    if (!h || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (h->mode != Mode::NDT) return mode_is_off(Mode::NDT, false);
    APD_TRY(nd_build_map(h, which));
    const NdState::Map& m = h->nd.maps[which];
    return read_voxels(h->eng.stream, m.buf, m.nv, capacity, coords_n3, counts, means_n3, raw_covs_n6, covs_n9);
  });
}

int apdgicp_ndt_get_correspondences(apdgicp_handle* h, int32_t* voxel_index, int64_t n_rows) {
  return guarded([&]() -> int {
    if (!h || !voxel_index) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (h->mode != Mode::NDT) return mode_is_off(Mode::NDT, false);
    if (!h->lin.have || h->nd.lin_src_gen != h->cloud_gen[kSrc]) return fail(APDGICP_ERR_NO_INPUT, "no correspondences yet");
    return read_frozen_corr(h->eng, h->lin, voxel_index, n_rows, "n_rows does not match the rows of the last linearize");
  });
}

int apdgicp_ndt_build_count(apdgicp_handle* h, int64_t* n_builds) {
  if (!h || !n_builds) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n_builds = h->nd.builds;
  return 0;
}

int apdgicp_batch_set_vgicp(apdgicp_batch* b, const apdgicp_vgicp_params* p) {
  return guarded([&]() -> int {
    // (the parameters first: what is wrong with them does not depend on the handle)
    APD_TRY(check_vgicp_params(p));
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (!p) return b->mode == Mode::VGICP ? set_mode(b, Mode::APD) : 0;  // (a no-op while another mode is on)
    APD_TRY(set_mode(b, Mode::VGICP));
    b->vg.prm = *p;
    return 0;
  });
}

int apdgicp_batch_get_vgicp(const apdgicp_batch* b, apdgicp_vgicp_params* p, int* enabled) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (p) *p = b->vg.prm;
  if (enabled) *enabled = b->mode == Mode::VGICP ? 1 : 0;
  return 0;
}

int apdgicp_batch_vgicp_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!b || !n_voxels) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(vgb_slot_map(b, cloud));
    *n_voxels = b->vg.vox.slots[cloud].nv;
    return 0;
  });
}

int apdgicp_batch_vgicp_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    APD_TRY(vgb_slot_map(b, cloud));
    const VoxSlots::Slot& sl = b->vg.vox.slots[cloud];
    return read_voxels(b->eng.stream, sl.buf, sl.nv, capacity, coords_n3, counts, means_n3, nullptr, covs_n9);
  });
}

int apdgicp_batch_vgicp_build_count(apdgicp_batch* b, int64_t* n_builds) {
  if (!b || !n_builds) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n_builds = b->vg.vox.builds;
  return 0;
}

int apdgicp_batch_set_ndt(apdgicp_batch* b, const apdgicp_ndt_params* p) {
  return guarded([&]() -> int {
    // (the parameters first: what is wrong with them does not depend on the handle)
    APD_TRY(check_ndt_params(p));
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (!p) return b->mode == Mode::NDT ? set_mode(b, Mode::APD) : 0;  // (a no-op while another mode is on)
    APD_TRY(set_mode(b, Mode::NDT));
    b->nd.prm = *p;
    return 0;
  });
}

int apdgicp_batch_get_ndt(const apdgicp_batch* b, apdgicp_ndt_params* p, int* enabled) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (p) *p = b->nd.prm;
  if (enabled) *enabled = b->mode == Mode::NDT ? 1 : 0;
  return 0;
}

int apdgicp_batch_ndt_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!b || !n_voxels) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(ndb_slot_map(b, cloud));
    *n_voxels = b->nd.vox.slots[cloud].nv;
    return 0;
  });
}

int apdgicp_batch_ndt_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* raw_covs_n6,
                                 double* covs_n9) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    APD_TRY(ndb_slot_map(b, cloud));
    const VoxSlots::Slot& sl = b->nd.vox.slots[cloud];
    return read_voxels(b->eng.stream, sl.buf, sl.nv, capacity, coords_n3, counts, means_n3, raw_covs_n6, covs_n9);
  });
}

int apdgicp_batch_ndt_build_count(apdgicp_batch* b, int64_t* n_builds) {
  if (!b || !n_builds) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n_builds = b->nd.vox.builds;
  return 0;
}

// ------------------------------------------------------------------------------------ FAST_VGICP_CUDA on batch handles
int apdgicp_batch_set_vgicp_cuda(apdgicp_batch* b, const apdgicp_vgicp_cuda_params* p) {
  return guarded([&]() -> int {
    // (the parameters first: what is wrong with them does not depend on the handle)
    APD_TRY(check_vgicp_cuda_params(p));
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (!p) return b->mode == Mode::VGICP_CUDA ? set_mode(b, Mode::APD) : 0;  // (a no-op while another mode is on)
    APD_TRY(set_mode(b, Mode::VGICP_CUDA));
    b->vc.have = false;
    b->vc.prm = *p;
    return 0;
  });
}

int apdgicp_batch_get_vgicp_cuda(const apdgicp_batch* b, apdgicp_vgicp_cuda_params* p, int* enabled) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (p) *p = b->vc.prm;
  if (enabled) *enabled = b->mode == Mode::VGICP_CUDA ? 1 : 0;
  return 0;
}

int apdgicp_batch_vgicp_cuda_kept(apdgicp_batch* b, int32_t cloud, int64_t* n_kept, int32_t* kept_index, int64_t capacity) {
  return guarded([&]() -> int {
    if (!b || !n_kept) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(vcb_slot(b, cloud, false));
    return read_kept(b->eng.stream, b->vc.slots[cloud].pc, n_kept, kept_index, capacity);
  });
}

int apdgicp_batch_vgicp_cuda_get_covariances(apdgicp_batch* b, int32_t cloud, double* raw_n6, double* reg_n9, int64_t capacity) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    APD_TRY(vcb_slot(b, cloud, false));
    return read_prepared_covariances(b->eng.stream, b->vc.slots[cloud].pc, raw_n6, reg_n9, capacity);
  });
}

int apdgicp_batch_vgicp_cuda_voxel_count(apdgicp_batch* b, int32_t cloud, int64_t* n_voxels) {
  return guarded([&]() -> int {
    if (!b || !n_voxels) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(vcb_slot(b, cloud, true));
    *n_voxels = b->vc.vox.slots[cloud].nv;
    return 0;
  });
}

int apdgicp_batch_vgicp_cuda_get_voxels(apdgicp_batch* b, int32_t cloud, int64_t capacity, int32_t* coords_n3, int32_t* counts, double* means_n3, double* covs_n9) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    APD_TRY(vcb_slot(b, cloud, true));
    const VoxSlots::Slot& sl = b->vc.vox.slots[cloud];
    if (sl.nv == 0) return 0;
    return read_voxels(b->eng.stream, sl.buf, sl.nv, capacity, coords_n3, counts, means_n3, nullptr, covs_n9);
  });
}

int apdgicp_batch_vgicp_cuda_get_correspondences(apdgicp_batch* b, int64_t pair, int32_t* voxel_index, int64_t n_kept_source) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    const VcbState& v = b->vc;
    if (b->mode != Mode::VGICP_CUDA) return mode_is_off(Mode::VGICP_CUDA, true);
    if (!v.have || v.have_epoch != b->eng.pts_epoch) return fail(APDGICP_ERR_NO_INPUT, "no align in this mode since the cloud slots and the mode were last set");
    if (pair < 0 || pair >= (int64_t)v.have_nk.size()) return fail(APDGICP_ERR_INVALID_ARG, "pair is not one of the last align");
    if (!voxel_index) return v.have_nk[pair];  // (the size query)
    if (n_kept_source != v.have_nk[pair]) return fail(APDGICP_ERR_INVALID_ARG, "n_kept_source does not match the pair's kept source size");
    if (n_kept_source == 0) return 0;
    APD_HIP(hipMemcpyAsync(voxel_index, b->run.corr.as<int>() + (size_t)pair * b->run.corr_stride, (size_t)n_kept_source * b->run.noff * 4, hipMemcpyDeviceToHost, b->eng.stream));
    APD_HIP(hipStreamSynchronize(b->eng.stream));
    return 0;
  });
}

int apdgicp_batch_vgicp_cuda_build_count(apdgicp_batch* b, int64_t* n_prepared, int64_t* n_maps) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (n_prepared) *n_prepared = b->vc.preps;
  if (n_maps) *n_maps = b->vc.vox.builds;
  return 0;
}

int apdgicp_batch_vgicp_cuda_last_phases(apdgicp_batch* b, double ms[3]) {
  if (!b || !ms) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  memcpy(ms, b->vc.phase_ms, sizeof(b->vc.phase_ms));
  return 0;
}

int apdgicp_batch_vgicp_cuda_debug_counts(apdgicp_batch* b, int64_t* prepare_waits, int64_t* map_waits, int64_t* ticks) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (prepare_waits) *prepare_waits = b->vc.prep_waits;
  if (map_waits) *map_waits = b->vc.map_waits;
  if (ticks) *ticks = b->loop.last_ticks;
  return 0;
}

int apdgicp_set_trace(apdgicp_handle* h, int enable) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  h->eng.trace_on = enable != 0;
  return 0;
}

int apdgicp_get_trace(apdgicp_handle* h, int64_t trial_capacity, double* lambdas, double* rhos, double* y0s, double* yis, int64_t* n_trials,
                      int64_t pose_capacity, double* poses16, int64_t* n_poses) {
  return guarded([&]() -> int {
    if (!h || !n_trials || !n_poses) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (trial_capacity < 0 || pose_capacity < 0 || (trial_capacity > 0 && (!lambdas || !rhos)) || (pose_capacity > 0 && !poses16))
      return fail(APDGICP_ERR_INVALID_ARG, "bad capacity / buffer");
    Engine& e = h->eng;
    if (!e.trace_on) return fail(APDGICP_ERR_NO_INPUT, "tracing is off (apdgicp_set_trace)");
    if (h->trace_from_host_loop) {
      *n_trials = (int64_t)h->tr_lambda.size(), *n_poses = (int64_t)h->tr_poses.size() / 16;
      const int64_t nt = std::min<int64_t>(*n_trials, trial_capacity), np = std::min<int64_t>(*n_poses, pose_capacity);
      if (nt) memcpy(lambdas, h->tr_lambda.data(), nt * sizeof(double)), memcpy(rhos, h->tr_rho.data(), nt * sizeof(double));
      if (nt && y0s) memcpy(y0s, h->tr_y0.data(), nt * sizeof(double));
      if (nt && yis) memcpy(yis, h->tr_yi.data(), nt * sizeof(double));
      if (np) memcpy(poses16, h->tr_poses.data(), np * 16 * sizeof(double));
      return 0;
    }
    if (!e.d_trace.p) return fail(APDGICP_ERR_NO_INPUT, "no align has run since tracing was enabled");
    std::vector<double> buf(e.trace_bytes() / sizeof(double));
    APD_HIP(hipMemcpyAsync(buf.data(), e.d_trace.p, e.trace_bytes(), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    int hdr[4];
    memcpy(hdr, buf.data(), sizeof(hdr));
    *n_trials = hdr[0], *n_poses = hdr[1];
    const int64_t nt = std::min<int64_t>(std::min(hdr[0], hdr[2]), trial_capacity), np = std::min<int64_t>(std::min(hdr[1], hdr[3]), pose_capacity);
    if (nt) memcpy(lambdas, &buf[2], nt * sizeof(double)), memcpy(rhos, &buf[2 + hdr[2]], nt * sizeof(double));
    if (nt && y0s) memcpy(y0s, &buf[2 + 2 * (size_t)hdr[2]], nt * sizeof(double));
    if (nt && yis) memcpy(yis, &buf[2 + 3 * (size_t)hdr[2]], nt * sizeof(double));
    for (int64_t q = 0; q < np; q++) {
      Rigid r;
      memcpy(r.m, &buf[2 + 4 * (size_t)hdr[2] + 12 * (size_t)q], sizeof(r.m));
      rigid_to_colmajor(r, poses16 + 16 * q);
    }
    return 0;
  });
}

int apdgicp_get_trace_step_norms(apdgicp_handle* h, int64_t capacity, double* norms, int64_t* n_trials) {
  return guarded([&]() -> int {
    if (!h || !n_trials || capacity < 0 || (capacity > 0 && !norms)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    Engine& e = h->eng;
    if (!e.trace_on) return fail(APDGICP_ERR_NO_INPUT, "tracing is off (apdgicp_set_trace)");
    if (h->trace_from_host_loop) {
      *n_trials = (int64_t)h->tr_dnorm.size();
      const int64_t nt = std::min<int64_t>(*n_trials, capacity);
      if (nt) memcpy(norms, h->tr_dnorm.data(), nt * sizeof(double));
      return 0;
    }
    if (!e.d_trace.p) return fail(APDGICP_ERR_NO_INPUT, "no align has run since tracing was enabled");
    std::vector<double> buf(e.trace_bytes() / sizeof(double));
    APD_HIP(hipMemcpyAsync(buf.data(), e.d_trace.p, e.trace_bytes(), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    int hdr[4];
    memcpy(hdr, buf.data(), sizeof(hdr));
    *n_trials = hdr[0];
    const int64_t nt = std::min<int64_t>(std::min(hdr[0], hdr[2]), capacity);
    if (nt) memcpy(norms, &buf[2 + 4 * (size_t)hdr[2] + 12 * (size_t)hdr[3]], nt * sizeof(double));
    return 0;
  });
}

int apdgicp_debug_atan2f(int device, const float* y, const float* x, float* out, int64_t n) {
  return guarded([&]() -> int {
    if (!y || !x || !out || n < 0) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(device));
    DevBuf buf;
    APD_TRY(buf.ensure((size_t)n * 12));
    float* dy = buf.as<float>();
    APD_HIP(hipMemcpy(dy, y, (size_t)n * 4, hipMemcpyHostToDevice));
    APD_HIP(hipMemcpy(dy + n, x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_atan2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dy, dy + n, dy + 2 * n, (long long)n);
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpy(out, dy + 2 * n, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
  });
}

int apdgicp_debug_live_buffers(int64_t* device_buffers, int64_t* pinned_buffers) {
  if (device_buffers) *device_buffers = DevBuf::live.load();
  if (pinned_buffers) *pinned_buffers = PinnedBuf::live.load();
  return 0;
}

int apdgicp_get_final_hessian(apdgicp_handle* h, double H[36]) {
  return guarded([&]() -> int {
    if (!h || !H) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = h->eng;
    switch (h->mode) {
      case Mode::ICP: return fail(APDGICP_ERR_UNSUPPORTED, "point-to-point ICP has no Hessian");
      case Mode::NDT:  // NDT and FAST_VGICP_CUDA keep the Hessian of their last align on the host (identity until then)
      case Mode::VGICP_CUDA:
      case Mode::GICP_MP:  // (of its last linearize: MP9)
        memcpy(H, h->final_H, 36 * sizeof(double));
        return 0;
      case Mode::VGICP:
      case Mode::APD: break;  // (on the device, in the pair state)
    }
    if (!h->pair_ready) {  // L:23: identity until the first accepted step
      for (int q = 0; q < 36; q++) H[q] = (q % 7 == 0) ? 1.0 : 0.0;
      return 0;
    }
    APD_HIP(hipMemcpyAsync(H, (char*)e.d_state.p + offsetof(PairState, final_H), 36 * sizeof(double), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_transform_source(apdgicp_handle* h, const float T[16], float* out_xyz, int64_t n, int64_t out_stride_bytes) {
  return guarded([&]() -> int {
    if (!h || !T || !out_xyz) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = h->eng;
    Engine::Cloud& c = e.clouds[kSrc];
    if (c.n <= 0) return fail(APDGICP_ERR_NO_INPUT, "source cloud is not set");
    if (n != c.n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
    if (out_stride_bytes < 12 || (out_stride_bytes & 3)) return fail(APDGICP_ERR_INVALID_ARG, "bad output stride");
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 12 + 64));
    float* dT = (float*)((char*)e.d_stage.p + (size_t)n * 12);
    APD_HIP(hipMemcpyAsync(dT, T, 16 * sizeof(float), hipMemcpyHostToDevice, e.stream));
    hipLaunchKernelGGL(k_transform_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, c.opts.as<float4>(), (int)n, dT, e.d_stage.as<float>(),
                       3ll);
    if (out_stride_bytes == 12) {
      APD_HIP(hipMemcpyAsync(out_xyz, e.d_stage.p, (size_t)n * 12, hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
    } else {
      std::vector<float> tmp((size_t)n * 3);
      APD_HIP(hipMemcpyAsync(tmp.data(), e.d_stage.p, (size_t)n * 12, hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
      for (int64_t i = 0; i < n; i++) memcpy((char*)out_xyz + i * out_stride_bytes, &tmp[3 * i], 12);
    }
    return 0;
  });
}

// nearest-neighbour statistics of the T-transformed source: sum and count of the squared distances inside the range
static int nn_range_stats(apdgicp_handle* h, const float T[16], double max_range2, int strict, double* sum, double* cnt) {
  APD_TRY(ensure_pair(h));
  Engine& e = h->eng;
  roctx_range rr("apdgicp:fitness");
  double T16[16];
  for (int q = 0; q < 16; q++) T16[q] = (double)T[q];
  APD_HIP(hipMemcpyAsync(e.d_T.p, T16, sizeof(T16), hipMemcpyHostToDevice, e.stream));
  hipLaunchKernelGGL(k_set_probe, dim3(1), dim3(1), 0, e.stream, e.d_state.as<PairState>(), e.d_T.as<double>(), (int)ST_NEED_LIN, 0);
  APD_TRY(e.launch_nn(e.whole()));
  APD_HIP(hipMemsetAsync(e.d_probe.p, 0, 2 * sizeof(double), e.stream));
  hipLaunchKernelGGL(k_fitness, dim3((unsigned)e.work.nblk_max, 1), dim3(LIN_BLK), 0, e.stream, e.d_desc.as<CloudDesc>(), e.d_pairs.as<PairDesc>(), e.work,
                     max_range2, e.d_probe.as<double>(), strict);
  APD_HIP(hipMemcpyAsync(e.h_probe.p, e.d_probe.p, 2 * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  h->have_corr = false;  // the nn partials were overwritten at another pose
  *sum = e.h_probe.as<double>()[0], *cnt = e.h_probe.as<double>()[1];
  return 0;
}

int apdgicp_fitness_score(apdgicp_handle* h, const float T[16], double max_range, double* score, int64_t* n_inliers) {
  return guarded([&]() -> int {
    if (!h || !T || !score) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    double sum = 0, cnt = 0;
    APD_TRY(nn_range_stats(h, T, max_range, 0, &sum, &cnt));
    *score = cnt > 0 ? sum / cnt : std::numeric_limits<double>::max();  // pcl returns max() when nothing is in range
    if (n_inliers) *n_inliers = (int64_t)cnt;
    return 0;
  });
}

int apdgicp_inlier_fraction(apdgicp_handle* h, const float T[16], double max_correspondence_dist, double* fraction, int64_t* n_inliers) {
  return guarded([&]() -> int {
    if (!h || !T || !fraction) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    double sum = 0, cnt = 0;
    APD_TRY(nn_range_stats(h, T, max_correspondence_dist * max_correspondence_dist, 1, &sum, &cnt));
    *fraction = (double)((float)(int)cnt / (float)h->eng.clouds[kSrc].n);  // static_cast<float>(num_inliers) / aligned->size()
    if (n_inliers) *n_inliers = (int64_t)cnt;
    return 0;
  });
}

int apdgicp_nearest_neighbours(apdgicp_handle* h, const float T[16], int32_t* index, float* sq_dist, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !T || !index || !sq_dist) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(ensure_pair(h));
    Engine& e = h->eng;
    if (n != e.clouds[kSrc].n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the source size");
    double T16[16], cost = 0.0;
    for (int q = 0; q < 16; q++) T16[q] = (double)T[q];
    APD_TRY(e.probe_linearize(T16, nullptr, nullptr, &cost, nullptr));  // search (ungated, cold) + the per-point pass that settles the exact index
    h->have_corr = true;
    APD_TRY(e.d_stage.ensure((size_t)n * 8));
    int* d_i = e.d_stage.as<int>();
    float* d_s = (float*)(d_i + n);
    hipLaunchKernelGGL(k_export_nn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, e.work.nnpt, e.work.sqd, e.clouds[kSrc].perm.as<int>(),
                       e.clouds[kTgt].perm.as<int>(), (int)n, d_i, d_s);
    APD_HIP(hipMemcpyAsync(index, d_i, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipMemcpyAsync(sq_dist, d_s, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_nearest_neighbours_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, int32_t* index, float* sq_dist) {
  return guarded([&]() -> int {
    if (!h || !queries_xyz || !index || !sq_dist || n <= 0) return fail(APDGICP_ERR_INVALID_ARG, "null argument or no queries");
    Engine& e = h->eng;
    constexpr int kQry = 2;  // a scratch cloud slot behind source and target
    if (e.clouds.size() < 2 || e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
    APD_TRY(e.set_cloud(kQry, queries_xyz, n, stride_bytes, 0, 0));
    apdgicp_pair p;
    p.source_cloud = kQry, p.target_cloud = kTgt;
    identity16(p.guess);
    h->pair_ready = false, h->have_corr = false;  // the handle's own pair is set up again by whoever needs it next
    APD_TRY(e.setup_pairs(&p, 1, true, false, /*need_cov=*/false));
    // the ungated cold search + the per-point pass that settles the exact index (the queries' covariances are whatever the buffer holds:
    // the pass computes a cost nobody reads)
    const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double cost = 0.0;
    APD_TRY(e.probe_linearize(I16, nullptr, nullptr, &cost, nullptr));
    APD_TRY(e.d_stage.ensure((size_t)n * 8));
    int* d_i = e.d_stage.as<int>();
    float* d_s = (float*)(d_i + n);
    hipLaunchKernelGGL(k_export_nn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, e.work.nnpt, e.work.sqd, e.clouds[kQry].perm.as<int>(),
                       e.clouds[kTgt].perm.as<int>(), (int)n, d_i, d_s);
    APD_HIP(hipMemcpyAsync(index, d_i, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipMemcpyAsync(sq_dist, d_s, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

// ---- exact k-nearest and radius queries of the target (apd_search.hpp; Q1 .. Q9 of the header)
// Q3: everything that can be said about the queries without a handle, in the order the header lists it
static int search_check_queries(const float* queries_xyz, int64_t n, int64_t stride_bytes) {
  if (!queries_xyz || n <= 0) return fail(APDGICP_ERR_INVALID_ARG, "null argument or no queries");
  if (n > (1 << 30)) return fail(APDGICP_ERR_INVALID_ARG, "too many queries");
  if (stride_bytes < 12 || (stride_bytes & 3)) return fail(APDGICP_ERR_INVALID_ARG, "stride_bytes must be a multiple of 4 and >= 12");
  for (int64_t i = 0; i < n; i++) {
    const float* p = (const float*)((const char*)queries_xyz + i * stride_bytes);
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
      return fail(APDGICP_ERR_INVALID_ARG, "query " + std::to_string(i) + " has a non-finite coordinate");
  }
  return 0;
}

// the queries into the scratch slot, sorted; Q7: the handle's own pair is set up again by whoever needs it next
static int search_set_queries(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, SearchTarget* T, int* nblk) {
  constexpr int kQry = 2;  // the scratch cloud slot of apdgicp_nearest_neighbours_of
  Engine& e = h->eng;
  e.sq.rows_valid = false;
  e.sq.groups_visited = e.sq.groups_total = 0;
  APD_TRY(e.set_cloud(kQry, queries_xyz, n, stride_bytes, 0, 0));
  h->pair_ready = false, h->have_corr = false;
  APD_TRY(e.pool_leave());   // (everything below runs on e.stream)
  APD_TRY(e.upload_desc());  // sorts what is not sorted yet: the queries, and a target nobody has searched so far
  const Engine::Cloud& t = e.clouds[kTgt];
  *T = SearchTarget{t.pts.as<float4>(), t.perm.as<int>(), t.cbox.as<Box>(), t.gbox.as<Box>(), t.n, 0};
  *nblk = (int)((n + SQ_BLK - 1) / SQ_BLK);
  APD_TRY(e.sq.visit.ensure((size_t)*nblk * sizeof(int)));
  return 0;
}

// groups the waves of the call's first searching launch looked at (apdgicp_search_group_stats): read behind the wait of the call
static int search_add_group_stats(Engine& e, int nblk, int target_n) {
  std::vector<int> v((size_t)nblk);
  APD_HIP(hipMemcpy(v.data(), e.sq.visit.p, v.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int x : v) e.sq.groups_visited += x;
  e.sq.groups_total += (int64_t)v.size() * ((target_n + kGroupPts - 1) / kGroupPts);
  return 0;
}

// k_knn_queries into sq.keys ([n][k]) and sq.cnt ([n]), enqueued
static int search_launch_knn(Engine& e, const SearchTarget& T, int64_t n, int nblk, int k, bool bounded, float r2) {
  constexpr int kQry = 2;
  APD_TRY(e.sq.keys.ensure((size_t)n * k * sizeof(unsigned long long)));
  APD_TRY(e.sq.cnt.ensure((size_t)n * sizeof(int)));
  const Engine::Cloud& q = e.clouds[kQry];
  hipLaunchKernelGGL(k_knn_queries, dim3((unsigned)nblk), dim3(SQ_BLK), 0, e.stream, T, q.pts.as<float4>(), q.perm.as<int>(), (int)n, k, bounded ? 1 : 0, r2,
                     e.sq.keys.as<unsigned long long>(), e.sq.cnt.as<int>(), e.sq.visit.as<int>());
  APD_HIP(hipGetLastError());
  return 0;
}

int apdgicp_knn_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, int32_t k, int32_t* index, float* sq_dist, int32_t* n_found) {
  return guarded([&]() -> int {
    if (k < 1) return fail(APDGICP_ERR_INVALID_ARG, "k must be at least 1");
    if (k > SQ_KMAX) return fail(APDGICP_ERR_UNSUPPORTED, "k above 64 is not offered");
    APD_TRY(search_check_queries(queries_xyz, n, stride_bytes));
    if (!h || !index || !sq_dist) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = h->eng;
    if (e.clouds.size() < 2 || e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
    roctx_range rr("apdgicp:knn_of");
    SearchTarget T;
    int nblk = 0;
    APD_TRY(search_set_queries(h, queries_xyz, n, stride_bytes, &T, &nblk));
    APD_TRY(search_launch_knn(e, T, n, nblk, k, false, 0.f));
    std::vector<unsigned long long> keys((size_t)n * k);
    APD_HIP(hipMemcpyAsync(keys.data(), e.sq.keys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(search_add_group_stats(e, nblk, T.n));
    for (size_t i = 0; i < keys.size(); i++) {
      const unsigned long long key = keys[i];
      const uint32_t bits = key == ~0ull ? 0x7f800000u : (uint32_t)(key >> 32);
      index[i] = key == ~0ull ? -1 : (int32_t)(uint32_t)key;
      memcpy(&sq_dist[i], &bits, 4);
    }
    if (n_found) *n_found = std::min<int32_t>(k, T.n);
    return 0;
  });
}

int apdgicp_radius_search_of(apdgicp_handle* h, const float* queries_xyz, int64_t n, int64_t stride_bytes, double radius, int32_t max_nn, int64_t* row_start,
                             int64_t* total) {
  return guarded([&]() -> int {
    if (!std::isfinite(radius) || radius < 0.0) return fail(APDGICP_ERR_INVALID_ARG, "radius must be finite and not negative");
    if (max_nn < 0) return fail(APDGICP_ERR_INVALID_ARG, "max_nn must not be negative");
    APD_TRY(search_check_queries(queries_xyz, n, stride_bytes));
    if (!h || !row_start || !total) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = h->eng;
    if (e.clouds.size() < 2 || e.clouds[kTgt].n <= 0) return fail(APDGICP_ERR_NO_INPUT, "target cloud is not set");
    roctx_range rr("apdgicp:radius_search_of");
    const float r2 = (float)(radius * radius);  // Q4
    SearchTarget T;
    int nblk = 0;
    APD_TRY(search_set_queries(h, queries_xyz, n, stride_bytes, &T, &nblk));
    Engine::SearchState& s = e.sq;
    s.src_start.assign((size_t)n + 1, 0);
    s.len.assign((size_t)n, 0);
    const Engine::Cloud& q = e.clouds[2];
    if (max_nn > 0 && max_nn <= SQ_KMAX && max_nn < T.n) {
      // Q9: the k-nearest kernel with r2 as its bound; row i is the head of the table's row i
      APD_TRY(search_launch_knn(e, T, n, nblk, max_nn, true, r2));
      APD_HIP(hipMemcpyAsync(s.len.data(), s.cnt.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
      APD_TRY(search_add_group_stats(e, nblk, T.n));
      for (int64_t i = 0; i < n; i++) s.src_start[i] = i * max_nn;
      s.span = n * max_nn;
    } else {
      // every hit: count, scan, (one wait: the total sizes the rows), fill, sort each row
      const int nsb = (int)((n + SCAN_BLK - 1) / SCAN_BLK);
      APD_TRY(s.cnt.ensure((size_t)n * sizeof(int)));
      APD_TRY(s.pos.ensure((size_t)n * sizeof(int)));
      APD_TRY(s.bsum.ensure(((size_t)nsb + 1) * sizeof(int)));
      hipLaunchKernelGGL(k_radius_count, dim3((unsigned)nblk), dim3(SQ_BLK), 0, e.stream, T, q.pts.as<float4>(), q.perm.as<int>(), (int)n, r2, s.cnt.as<int>(),
                         s.visit.as<int>());
      hipLaunchKernelGGL(k_radius_scan, dim3((unsigned)nsb), dim3(SCAN_BLK), 0, e.stream, s.cnt.as<int>(), (int)n, s.pos.as<int>(), s.bsum.as<int>());
      hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, e.stream, s.bsum.as<int>(), nsb, s.bsum.as<int>() + nsb);
      APD_HIP(hipGetLastError());
      APD_HIP(hipMemcpyAsync(s.len.data(), s.cnt.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
      // (the device's scan is in int32: the host's own sum decides whether it can be trusted)
      int64_t all = 0;
      for (int64_t i = 0; i < n; i++) s.src_start[i] = all, all += s.len[i];
      if (all > 0x7fffffffll) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^31 - 1 hits in all (" + std::to_string(all) + ")");
      s.span = all;
      if (all > 0) {
        APD_TRY(s.keys.ensure((size_t)all * sizeof(unsigned long long)));
        hipLaunchKernelGGL(k_radius_fill, dim3((unsigned)nblk), dim3(SQ_BLK), 0, e.stream, T, q.pts.as<float4>(), q.perm.as<int>(), (int)n, r2, s.cnt.as<int>(),
                           s.pos.as<int>(), s.bsum.as<int>(), s.keys.as<unsigned long long>());
        hipLaunchKernelGGL(k_radius_sort_rows, dim3((unsigned)n), dim3(SQ_SORT_BLK), 0, e.stream, s.cnt.as<int>(), s.pos.as<int>(), s.bsum.as<int>(),
                           s.keys.as<unsigned long long>());
        APD_HIP(hipGetLastError());
        APD_HIP(hipStreamSynchronize(e.stream));
      }
      APD_TRY(search_add_group_stats(e, nblk, T.n));
      if (max_nn > 0 && max_nn < T.n)  // Q5: the max_nn smallest of a longer row
        for (int64_t i = 0; i < n; i++) s.len[i] = std::min<int>(s.len[i], max_nn);
    }
    int64_t sum = 0;
    for (int64_t i = 0; i < n; i++) row_start[i] = sum, sum += s.len[i];
    row_start[n] = sum;
    if (sum > 0x7fffffffll) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^31 - 1 hits in all (" + std::to_string(sum) + ")");
    *total = s.total = sum;
    s.tgt_gen = h->cloud_gen[kTgt];
    s.rows_valid = true;
    return 0;
  });
}

int apdgicp_radius_search_rows(apdgicp_handle* h, int32_t* index, float* sq_dist) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
    Engine& e = h->eng;
    Engine::SearchState& s = e.sq;
    if (!s.rows_valid) return fail(APDGICP_ERR_NO_INPUT, "no radius search whose rows are kept (apdgicp_radius_search_of)");
    if (s.tgt_gen != h->cloud_gen[kTgt]) return fail(APDGICP_ERR_NO_INPUT, "the target has been set since the radius search");
    if (s.total == 0) return 0;
    if (!index || !sq_dist) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(e.device));
    std::vector<unsigned long long> keys((size_t)s.span);
    APD_HIP(hipMemcpyAsync(keys.data(), s.keys.p, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    int64_t o = 0;
    for (size_t i = 0; i < s.len.size(); i++)
      for (int r = 0; r < s.len[i]; r++, o++) {
        const unsigned long long key = keys[(size_t)s.src_start[i] + r];
        const uint32_t bits = (uint32_t)(key >> 32);
        index[o] = (int32_t)(uint32_t)key;
        memcpy(&sq_dist[o], &bits, 4);
      }
    return 0;
  });
}

int apdgicp_search_group_stats(apdgicp_handle* h, int64_t* groups_visited, int64_t* groups_total) {
  if (!h || !groups_visited || !groups_total) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *groups_visited = h->eng.sq.groups_visited, *groups_total = h->eng.sq.groups_total;
  return 0;
}

int apdgicp_get_points(apdgicp_handle* h, int which, float* out_xyz, int64_t n) {
  return guarded([&]() -> int {
    if (!h || !out_xyz || (which != kSrc && which != kTgt)) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    Engine& e = h->eng;
    Engine::Cloud& c = e.clouds[which];
    if (c.n <= 0) return fail(APDGICP_ERR_NO_INPUT, "cloud not set");
    if (n != c.n) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the cloud size");
    APD_HIP(hipSetDevice(e.device));
    if (c.staged) {  // a scan-sized host cloud still waiting in its pinned buffer for the sort: the float4 copy is right there
      const float4* p = c.stage.as<const float4>();
      for (int64_t i = 0; i < n; i++) out_xyz[3 * i] = p[i].x, out_xyz[3 * i + 1] = p[i].y, out_xyz[3 * i + 2] = p[i].z;
      return 0;
    }
    APD_TRY(e.upload_desc());  // (sorts what is not sorted yet: a staged cloud's opts are written by its sort)
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 12));
    hipLaunchKernelGGL(k_unpack_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, c.opts.as<float4>(), (int)n, e.d_stage.as<float>());
    APD_HIP(hipMemcpyAsync(out_xyz, e.d_stage.p, (size_t)n * 12, hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_wait_producer(apdgicp_handle* h, void* producer_stream) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  return h->eng.wait_producer(producer_stream);
}

int apdgicp_get_stream(apdgicp_handle* h, void** stream) {
  if (!h || !stream) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *stream = (void*)h->eng.stream;
  return 0;
}

int apdgicp_batch_get_stream(apdgicp_batch* b, void** stream) {
  if (!b || !stream) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *stream = (void*)b->eng.stream;
  return 0;
}

int apdgicp_batch_wait_producer(apdgicp_batch* b, void* producer_stream) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  return b->eng.wait_producer(producer_stream);
}

int apdgicp_synchronize(apdgicp_handle* h) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "handle is null");
  APD_HIP(hipStreamSynchronize(h->eng.stream));
  return 0;
}

// ------------------------------------------------------------------------------------ batch
int apdgicp_batch_create(const apdgicp_params* p, int device, void* stream, apdgicp_batch** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_params dflt;
    apdgicp_default_params(&dflt);
    apdgicp_batch* b = new apdgicp_batch;
    const int rc = b->eng.init(p ? p : &dflt, device, stream);
    if (rc < 0) {
      delete b;
      return rc;
    }
    b->eng.profile_nn = env_int("APDGICP_PROFILE_NN", 0) != 0;
    b->eng.keep_maha = false;  // no batch entry point reads the Mahalanobis matrices back
    const char* recip_mode = getenv("APDGICP_ICP_RECIP_MODE");
    b->ic.brute = recip_mode && std::string(recip_mode) == "brute";
    *out = b;
    return 0;
  });
}

int apdgicp_batch_destroy(apdgicp_batch* b) {
  delete b;
  return 0;
}

int apdgicp_batch_set_params(apdgicp_batch* b, const apdgicp_params* p) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  return b->eng.set_params(p);
}

int apdgicp_batch_clear(apdgicp_batch* b) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  APD_TRY(b->eng.pool_leave());
  APD_HIP(hipStreamSynchronize(b->eng.stream));
  b->eng.clouds.clear();  // (frees every slot's buffers)
  b->eng.clouds_written();
  b->release_voxel_modes();  // (V8 / N10: every slot's map and inverse permutation go with the clouds)
  return 0;
}

int apdgicp_batch_add_cloud(apdgicp_batch* b, const float* xyz, int64_t n, int64_t stride_bytes, int on_device) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    const int slot = (int)b->eng.clouds.size();
    const int rc = b->eng.set_cloud(slot, xyz, n, stride_bytes, on_device, 0);
    if (rc < 0) {
      if ((int)b->eng.clouds.size() > slot) b->eng.clouds.resize(slot);
      return rc;
    }
    return slot;
  });
}

int apdgicp_batch_set_cloud(apdgicp_batch* b, int32_t index, const float* xyz, int64_t n, int64_t stride_bytes, int on_device) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (index < 0 || index >= (1 << 24)) return fail(APDGICP_ERR_INVALID_ARG, "cloud index out of range");
    APD_TRY(b->eng.set_cloud(index, xyz, n, stride_bytes, on_device, 0));
    return index;
  });
}

int apdgicp_batch_set_clouds(apdgicp_batch* b, int32_t first_index, int32_t count, const float* const* xyz, const int64_t* n, int64_t stride_bytes,
                             int on_device) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (on_device) return b->eng.set_clouds_device(first_index, count, xyz, n, stride_bytes);
    return b->eng.set_clouds_host(first_index, count, xyz, n, stride_bytes);
  });
}

int apdgicp_batch_compute_covariances(apdgicp_batch* b) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    std::vector<int> ids;
    for (int i = 0; i < (int)b->eng.clouds.size(); i++)
      if (b->eng.clouds[i].n > 0) ids.push_back(i);
    return b->eng.compute_covariances(ids);
  });
}

int apdgicp_batch_align_async(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, void** d_results) {
  return guarded([&]() -> int {
    if (!b || !pairs) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (b->mode != Mode::APD) {  // the device-loop modes: complete on return (V12 / N15 / IC15 / VC16)
      switch (b->mode) {
        case Mode::VGICP: APD_TRY(vgb_align(b, pairs, n_pairs)); break;
        case Mode::NDT: APD_TRY(ndb_align(b, pairs, n_pairs)); break;
        case Mode::ICP: APD_TRY(icb_align(b, pairs, n_pairs)); break;
        case Mode::VGICP_CUDA: APD_TRY(vcb_align(b, pairs, n_pairs)); break;
        case Mode::GICP_MP:  // (single handles only: no setter of a batch handle names it)
        case Mode::APD: break;
      }
      if (d_results) *d_results = b->eng.d_results.p;
      return 0;
    }
    if (b->eng.pool_eligible()) {  // Levenberg-Marquardt: through the pair pool (complete on return, like every LM run)
      uint64_t ticket = 0;
      APD_TRY(b->eng.pool_enqueue(pairs, n_pairs, &ticket));
      return b->eng.pool_collect(ticket, d_results, nullptr);
    }
    APD_TRY(b->eng.setup_pairs(pairs, n_pairs, true, /*pipeline_cov=*/true));
    APD_TRY(b->eng.run_align());
    if (d_results) *d_results = b->eng.d_results.p;
    return 0;
  });
}

int apdgicp_batch_align_enqueue(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, uint64_t* ticket) {
  return guarded([&]() -> int {
    if (!b || !pairs || !ticket) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (b->mode != Mode::APD) return no_pipeline(b->mode);
    Engine& e = b->eng;
    if (e.pool_eligible()) return e.pool_enqueue(pairs, n_pairs, ticket);
    APD_TRY(e.ensure_alt_slot());
    e.swap_slots();  // the slot of the batch before the last one becomes current (run_align waits for it if nobody collected it)
    e.align_seq++;
    b->slot_pairs[e.align_seq & 1] = n_pairs;
    APD_TRY(e.setup_pairs(pairs, n_pairs, true, /*pipeline_cov=*/true));
    APD_TRY(e.run_align(/*defer_poll=*/true));
    *ticket = e.align_seq;
    return 0;
  });
}

int apdgicp_batch_pump(apdgicp_batch* b) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (b->mode != Mode::APD) return no_pipeline(b->mode);
    return b->eng.pool.on ? b->eng.pool_pump(false) : 0;
  });
}

int apdgicp_batch_is_pooled(apdgicp_batch* b) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (b->mode != Mode::APD) return 0;
  return b->eng.pool_eligible() ? Engine::pool_lanes_cfg() : 0;
}

int apdgicp_batch_align_collect(apdgicp_batch* b, uint64_t ticket, void** d_results, apdgicp_result* host_results) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    if (b->mode != Mode::APD) return no_pipeline(b->mode);
    Engine& e = b->eng;
    if (e.pool_find(ticket)) return e.pool_collect(ticket, d_results, host_results);
    const bool previous = ticket + 1 == e.align_seq;
    if (ticket == 0 || (ticket != e.align_seq && !previous)) return fail(APDGICP_ERR_INVALID_ARG, "ticket is not one of the last two enqueued batches");
    if (previous) e.swap_slots();
    int rc = e.finish_align();
    const int64_t n = b->slot_pairs[ticket & 1];
    if (rc == 0) {
      if (d_results) *d_results = e.d_results.p;
      if (host_results) {
        if (const ResultRec* r = e.host_results()) {
          memcpy(host_results, r, n * sizeof(apdgicp_result));
        } else {
          const hipError_t he = hipMemcpy(host_results, e.d_results.p, n * sizeof(apdgicp_result), hipMemcpyDeviceToHost);
          if (he != hipSuccess) rc = fail(APDGICP_ERR_HIP, hipGetErrorString(he));
        }
      }
    }
    if (previous) e.swap_slots();
    return rc;
  });
}

int apdgicp_batch_align(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, apdgicp_result* results) {
  return guarded([&]() -> int {
    if (!results) return fail(APDGICP_ERR_INVALID_ARG, "results is null");
    if (b && pairs && b->mode == Mode::APD && b->eng.pool_eligible()) {
      uint64_t ticket = 0;
      APD_TRY(b->eng.pool_enqueue(pairs, n_pairs, &ticket));
      return b->eng.pool_collect(ticket, nullptr, results);
    }
    APD_TRY(apdgicp_batch_align_async(b, pairs, n_pairs, nullptr));
    Engine& e = b->eng;
    if (const ResultRec* r = e.host_results()) {
      memcpy(results, r, n_pairs * sizeof(apdgicp_result));
      return 0;
    }
    APD_HIP(hipMemcpyAsync(results, e.d_results.p, n_pairs * sizeof(apdgicp_result), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_batch_fitness(apdgicp_batch* b, const apdgicp_pair* pairs, int64_t n_pairs, const float* T, double max_range, double* scores,
                          int64_t* inliers) {
  return guarded([&]() -> int {
    if (!b || !pairs || !scores) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    Engine& e = b->eng;
    const bool same = e.npairs == n_pairs && (int64_t)e.h_pairs.size() == n_pairs && e.pairs_current;  // (no cloud slot written since: Engine::pairs_current)
    bool same_pairs = same;
    for (int64_t i = 0; same_pairs && i < n_pairs; i++)
      same_pairs = e.h_pairs[i].src == pairs[i].source_cloud && e.h_pairs[i].tgt == pairs[i].target_cloud;
    std::vector<float> pool_T;
    if (!T && e.pool.on && e.pool.last_lane >= 0) {  // the last align ran in the pair pool: its poses are in the batch's records
      const Engine::PoolJob& j = e.pool.jobs[e.pool.last_lane];
      bool match = j.state != Engine::PoolJob::FREE && !j.clouds_replaced && (int64_t)j.pair_ids.size() == n_pairs;  // (no cloud replaced since)
      for (int64_t i = 0; match && i < n_pairs; i++) match = j.pair_ids[i].first == pairs[i].source_cloud && j.pair_ids[i].second == pairs[i].target_cloud;
      if (match) {
        APD_TRY(e.pool_collect(j.ticket, nullptr, nullptr));
        pool_T.resize((size_t)n_pairs * 16);
        for (int64_t i = 0; i < n_pairs; i++) memcpy(&pool_T[(size_t)i * 16], j.recs[i].T, 16 * sizeof(float));
        T = pool_T.data();
        same_pairs = false;
      }
    }
    if (!T && b->mode == Mode::ICP && same_pairs && e.poses_of_align) {  // IC16: the poses of an ICP align are its records' (the pair state holds the identity)
      std::vector<ResultRec> recs((size_t)n_pairs);
      APD_HIP(hipMemcpyAsync(recs.data(), e.d_results.p, recs.size() * sizeof(ResultRec), hipMemcpyDeviceToHost, e.stream));
      APD_HIP(hipStreamSynchronize(e.stream));
      pool_T.resize((size_t)n_pairs * 16);
      for (int64_t i = 0; i < n_pairs; i++) memcpy(&pool_T[(size_t)i * 16], recs[i].T, 16 * sizeof(float));
      T = pool_T.data();
    }
    // (the state's poses are the align's only until somebody else writes them: an explicit-pose call on the same list does)
    if (!T && !(same_pairs && e.poses_of_align)) return fail(APDGICP_ERR_NO_INPUT, "T == NULL needs a previous align of the same pair list");
    if (!same_pairs) APD_TRY(e.setup_pairs(pairs, n_pairs, true));
    else APD_TRY(e.pool_leave());  // (a pooled batch of ANOTHER list may have come since: the launches below are not the pool's)
    if (T) e.poses_of_align = !pool_T.empty();  // (the pool's records ARE the last align's poses; the caller's are not)
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n_pairs * (16 * sizeof(float) + 2 * sizeof(double))));
    double* d_out = e.d_stage.as<double>();
    float* d_T = (float*)(d_out + 2 * n_pairs);
    if (T) APD_HIP(hipMemcpyAsync(d_T, T, (size_t)n_pairs * 16 * sizeof(float), hipMemcpyHostToDevice, e.stream));
    APD_HIP(hipMemsetAsync(d_out, 0, (size_t)n_pairs * 2 * sizeof(double), e.stream));
    hipLaunchKernelGGL(k_set_poses, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), 0, e.stream, e.d_state.as<PairState>(), T ? d_T : (const float*)nullptr,
                       (int)n_pairs);
    APD_TRY(e.launch_nn(e.whole()));
    hipLaunchKernelGGL(k_fitness, dim3((unsigned)e.work.nblk_max, (unsigned)n_pairs), dim3(LIN_BLK), 0, e.stream, e.d_desc.as<CloudDesc>(),
                       e.d_pairs.as<PairDesc>(), e.work, max_range, d_out, 0);
    std::vector<double> h((size_t)n_pairs * 2);
    APD_HIP(hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    for (int64_t i = 0; i < n_pairs; i++) {
      scores[i] = h[2 * i + 1] > 0 ? h[2 * i] / h[2 * i + 1] : std::numeric_limits<double>::max();
      if (inliers) inliers[i] = (int64_t)h[2 * i + 1];
    }
    return 0;
  });
}

int apdgicp_batch_synchronize(apdgicp_batch* b) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  return guarded([&]() -> int {
    if (b->eng.pool.on) APD_TRY(b->eng.pool_drain());  // (pooled LM batches: every batch in flight runs to its end)
    if (b->eng.cstream != b->eng.stream) APD_HIP(hipStreamSynchronize(b->eng.cstream));
    APD_HIP(hipStreamSynchronize(b->eng.stream));
    return 0;
  });
}

int apdgicp_batch_copy_results(apdgicp_batch* b, void* dst, int64_t n_pairs, int dst_on_device) {
  if (!b || !dst) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  Engine& e = b->eng;
  if (e.pool.on && e.pool.last_lane >= 0) {  // the last align ran in the pair pool
    Engine::PoolJob& j = e.pool.jobs[e.pool.last_lane];
    if (n_pairs <= 0 || n_pairs > j.np) return fail(APDGICP_ERR_INVALID_ARG, "n_pairs exceeds the last batch");
    void* d = nullptr;
    APD_TRY(e.pool_collect(j.ticket, &d, nullptr));
    APD_HIP(hipMemcpyAsync(dst, d, n_pairs * sizeof(apdgicp_result), dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  }
  if (n_pairs <= 0 || n_pairs > e.npairs) return fail(APDGICP_ERR_INVALID_ARG, "n_pairs exceeds the last batch");
  APD_HIP(hipSetDevice(e.device));
  APD_HIP(hipMemcpyAsync(dst, e.d_results.p, n_pairs * sizeof(apdgicp_result), dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  return 0;
}

int apdgicp_batch_set_pair_groups(apdgicp_batch* b, int max_groups) {
  if (!b || max_groups < 1) return fail(APDGICP_ERR_INVALID_ARG, "batch is null or max_groups < 1");
  b->eng.max_groups = max_groups;
  return 0;
}

int apdgicp_batch_set_profiling(apdgicp_batch* b, int enable) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  b->eng.profile_nn = enable != 0;
  return 0;
}

int apdgicp_batch_last_nn_time(apdgicp_batch* b, double* total_ms, int64_t* launches) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (total_ms) *total_ms = b->eng.last_nn_ms;
  if (launches) *launches = b->eng.last_nn_launches;
  return 0;
}

int apdgicp_batch_set_icp(apdgicp_batch* b, const apdgicp_icp_params* p) {
  return guarded([&]() -> int {
    // (the parameters first: what is wrong with them does not depend on the handle)
    APD_TRY(check_icp_params(p));
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    IcbState& v = b->ic;
    if (p) v.prm = *p;
    if (!p || !p->enable) return b->mode == Mode::ICP ? set_mode(b, Mode::APD) : 0;  // (a no-op while another mode is on)
    APD_TRY(set_mode(b, Mode::ICP));
    v.have = false;
    return 0;
  });
}

int apdgicp_batch_get_icp(const apdgicp_batch* b, apdgicp_icp_params* p, int* enabled) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (p) {
    *p = b->ic.prm;
    p->enable = b->mode == Mode::ICP ? 1 : 0;
  }
  if (enabled) *enabled = b->mode == Mode::ICP ? 1 : 0;
  return 0;
}

int apdgicp_batch_icp_states(apdgicp_batch* b, int32_t* states, int64_t n_pairs) {
  return guarded([&]() -> int {
    if (!b || !states) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(icb_check_have(b, 0));
    IcbState& v = b->ic;
    if (n_pairs != (int64_t)v.src.size()) return fail(APDGICP_ERR_INVALID_ARG, "n_pairs does not match the last align");
    std::vector<IcpRecord> recs((size_t)n_pairs);
    APD_HIP(hipMemcpyAsync(recs.data(), v.rec.p, recs.size() * sizeof(IcpRecord), hipMemcpyDeviceToHost, b->eng.stream));
    APD_HIP(hipStreamSynchronize(b->eng.stream));
    for (int64_t i = 0; i < n_pairs; i++) states[i] = recs[i].state;
    return 0;
  });
}

int apdgicp_batch_icp_get_correspondences(apdgicp_batch* b, int64_t pair, int32_t* match, float* sq_dist, int64_t n) {
  return guarded([&]() -> int {
    if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
    APD_TRY(icb_check_have(b, pair));
    Engine& e = b->eng;
    IcbState& v = b->ic;
    if (n != v.n_src[pair]) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the pair's source size");
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 8));
    int* d_c = e.d_stage.as<int>();
    float* d_s = (float*)(d_c + n);
    const size_t o = (size_t)pair * v.nstride;
    hipLaunchKernelGGL(k_icp_export, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, v.match.as<int>() + o, v.dsq.as<float>() + o,
                       e.clouds[v.src[pair]].perm.as<int>(), e.clouds[v.tgt[pair]].perm.as<int>(), (int)n, d_c, d_s);
    APD_HIP(hipGetLastError());
    if (match) APD_HIP(hipMemcpyAsync(match, d_c, n * sizeof(int), hipMemcpyDeviceToHost, e.stream));
    if (sq_dist) APD_HIP(hipMemcpyAsync(sq_dist, d_s, n * sizeof(float), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_batch_icp_get_working_cloud(apdgicp_batch* b, int64_t pair, float* xyz, int64_t n) {
  return guarded([&]() -> int {
    if (!b || !xyz) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(icb_check_have(b, pair));
    Engine& e = b->eng;
    IcbState& v = b->ic;
    if (n != v.n_src[pair]) return fail(APDGICP_ERR_INVALID_ARG, "n does not match the pair's source size");
    APD_HIP(hipStreamSynchronize(e.stream));
    APD_TRY(e.d_stage.ensure((size_t)n * 12));
    hipLaunchKernelGGL(k_icp_export_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, v.W.as<float4>() + v.w_off[pair], e.clouds[v.src[pair]].perm.as<int>(), (int)n,
                       e.d_stage.as<float>());
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(xyz, e.d_stage.p, (size_t)n * 12, hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    return 0;
  });
}

int apdgicp_batch_icp_get_trace(apdgicp_batch* b, int64_t pair, int64_t capacity, float* T_k16, int64_t* n_corr, double* mse, int32_t* similar, int64_t* n_iterations) {
  return guarded([&]() -> int {
    if (!b || !n_iterations || capacity < 0) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
    APD_TRY(icb_check_have(b, pair));
    Engine& e = b->eng;
    IcbState& v = b->ic;
    IcbAux aux;
    std::vector<IcbTrace> tr((size_t)v.trace_cap);
    APD_HIP(hipMemcpyAsync(&aux, v.aux.as<IcbAux>() + pair, sizeof(aux), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipMemcpyAsync(tr.data(), v.trace.as<IcbTrace>() + (size_t)pair * v.trace_cap, tr.size() * sizeof(IcbTrace), hipMemcpyDeviceToHost, e.stream));
    APD_HIP(hipStreamSynchronize(e.stream));
    *n_iterations = aux.n_trace;
    const int64_t m = std::min<int64_t>(std::min<int64_t>(aux.n_trace, v.trace_cap), capacity);
    for (int64_t k = 0; k < m; k++) {
      if (T_k16) memcpy(T_k16 + 16 * k, tr[k].T_k, 16 * sizeof(float));
      if (n_corr) n_corr[k] = tr[k].n_corr;
      if (mse) mse[k] = tr[k].mse;
      if (similar) similar[k] = tr[k].similar;
    }
    return 0;
  });
}

int apdgicp_batch_icp_debug_counts(apdgicp_batch* b, int64_t* launches, int64_t* waits, int64_t* ticks) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (launches) *launches = b->ic.launches;
  if (waits) *waits = b->ic.waits;
  if (ticks) *ticks = b->ic.ticks;
  return 0;
}

int apdgicp_batch_debug_stats(apdgicp_batch* b, unsigned long long out[16]) {
  if (!b || !out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  Engine& e = b->eng;
  memset(out, 0, 16 * sizeof(unsigned long long));
  if (!e.d_stats.p) return 0;
  APD_HIP(hipMemcpyAsync(out, e.d_stats.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipMemsetAsync(e.d_stats.p, 0, 16 * sizeof(unsigned long long), e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  return 0;
}

int apdgicp_batch_debug_block_timeline(apdgicp_batch* b, unsigned long long* out, int64_t capacity_blocks, int64_t* n_blocks) {
  if (!b || !out || !n_blocks || capacity_blocks < 0) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
  Engine& e = b->eng;
  *n_blocks = 0;
  if (!e.d_stats.p || !e.stats_blocks) return 0;
  const int64_t n = std::min<int64_t>(capacity_blocks, e.stats_blocks);
  APD_HIP(hipMemcpyAsync(out, e.d_stats.as<unsigned long long>() + 16, (size_t)n * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
  APD_HIP(hipMemsetAsync(e.d_stats.as<unsigned long long>() + 16, 0, (size_t)e.stats_blocks * 3 * sizeof(unsigned long long), e.stream));
  APD_HIP(hipStreamSynchronize(e.stream));
  *n_blocks = n;
  return 0;
}

int apdgicp_batch_last_nn_profile(apdgicp_batch* b, double* total_ms, int64_t* launches, int64_t* pairs_covered) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (b->eng.pool.on) {  // pooled LM batches: the timed launches harvested since the last call (they belong to no single batch)
    if (total_ms) *total_ms = b->eng.pool.nn_ms;
    if (launches) *launches = b->eng.pool.nn_launches;
    if (pairs_covered) *pairs_covered = b->eng.pool.nn_pairs;
    b->eng.pool.nn_ms = 0, b->eng.pool.nn_launches = 0, b->eng.pool.nn_pairs = 0;
    return 0;
  }
  if (total_ms) *total_ms = b->eng.last_nn_ms;
  if (launches) *launches = b->eng.last_nn_launches;
  if (pairs_covered) *pairs_covered = b->eng.last_nn_pairs;
  return 0;
}

int apdgicp_batch_last_nn_kernel(apdgicp_batch* b, char* name, int capacity) {
  if (!b || !name || capacity < 1) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
  // (pooled LM batches: the kernel of the launches that were timed -- the last launch of all is a few-pair tail of another shape)
  snprintf(name, (size_t)capacity, "%s", b->eng.pool.on && b->eng.pool.timed_kernel[0] ? b->eng.pool.timed_kernel : b->eng.last_nn_kernel);
  return 0;
}

int apdgicp_batch_last_ticks(apdgicp_batch* b, int* ticks, int* nn_sources_per_lane, int* nn_target_splits) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  if (ticks) *ticks = b->eng.last_ticks;
  if (nn_sources_per_lane) *nn_sources_per_lane = b->eng.nn_S;
  if (nn_target_splits) *nn_target_splits = b->eng.work.T;
  return 0;
}


int apdgicp_batch_pool_counters(apdgicp_batch* b, int64_t* chunks, int64_t* ticks, int64_t* slot_ticks) {
  if (!b) return fail(APDGICP_ERR_INVALID_ARG, "batch is null");
  const Engine::Pool& p = b->eng.pool;
  if (chunks) *chunks = p.n_chunks;
  if (ticks) *ticks = p.n_ticks;
  if (slot_ticks) *slot_ticks = p.n_pair_ticks;
  return 0;
}

// ------------------------------------------------------------------ scan-to-submap target assembly (apd_voxel.hpp)
int apdgicp_submap_create(int device, void* stream, apdgicp_submap** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    apdgicp_submap* s = new apdgicp_submap;
    s->device = device;
    if (stream) {
      s->stream = (hipStream_t)stream;
    } else {
      const hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
      if (e != hipSuccess) {
        delete s;
        return fail(APDGICP_ERR_HIP, hipGetErrorString(e));
      }
      s->own_stream = true;
    }
    if (s->h_scal.ensure(2 * sizeof(int)) < 0 || s->scal.ensure(8 * sizeof(int)) < 0) {
      delete s;
      return fail(APDGICP_ERR_HIP, "allocation failed");
    }
    *out = s;
    return 0;
  });
}

int apdgicp_submap_destroy(apdgicp_submap* s) {
  delete s;
  return 0;
}

int apdgicp_submap_set_downsample_method(apdgicp_submap* s, int method) {
  if (!s) return fail(APDGICP_ERR_INVALID_ARG, "submap is null");
  if (method != APDGICP_DOWNSAMPLE_VOXELGRID && method != APDGICP_DOWNSAMPLE_APPROX_VOXELGRID) return fail(APDGICP_ERR_INVALID_ARG, "unknown downsample method");
  s->method = method;
  return 0;
}

// AV1 .. AV7: pcl::ApproximateVoxelGrid of the n points of s->cat into s->out, one wait (for n_out)
static int submap_approx_voxel(apdgicp_submap* s, int n, const float il[3], int64_t* n_out) {
  const int nt = scan_tiles(n), nb = (n + AV_BLK - 1) / AV_BLK;
  APD_TRY(s->av_sort.ensure(n, true));
  APD_TRY(s->av_evict.ensure((size_t)n * 4));
  APD_TRY(s->av_tiles.ensure((size_t)nt * 4));
  APD_TRY(s->av_head.ensure((size_t)n));
  APD_TRY(s->av_words.ensure(AV_WORDS * sizeof(int)));
  APD_TRY(s->out.ensure((size_t)n * 16));
  const float4* cat = s->cat.as<float4>();
  int *evict = s->av_evict.as<int>(), *tiles = s->av_tiles.as<int>(), *words = s->av_words.as<int>();
  unsigned char* head = s->av_head.as<unsigned char>();
  hipLaunchKernelGGL(k_av_keys, dim3(nb), dim3(AV_BLK), 0, s->stream, cat, n, il[0], il[1], il[2], s->av_sort.keys_a.as<unsigned long long>(),
                     s->av_sort.val_a.as<int>(), evict, words);
  const RadixSorted r = enqueue_radix_sort(s->stream, s->av_sort, n, AV_SORT_PASSES, true);
  hipLaunchKernelGGL(k_av_heads, dim3(nb), dim3(AV_BLK), 0, s->stream, r.keys, r.vals, cat, n, il[0], il[1], il[2], head, evict, words);
  enqueue_exclusive_scan(s->stream, evict, n, tiles, words);  // words[0] = evictions
  hipLaunchKernelGGL(k_av_occ, dim3(1), dim3(SCAN_BLK), 0, s->stream, words);
  hipLaunchKernelGGL(k_av_centroids, dim3(nb), dim3(AV_BLK), 0, s->stream, r.keys, r.vals, head, cat, evict, tiles, words, n, s->out.as<float4>(), n);
  APD_HIP(hipGetLastError());
  APD_HIP(hipMemcpyAsync(s->h_scal.p, words + 1, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  APD_HIP(hipStreamSynchronize(s->stream));
  const int total = s->h_scal.as<int>()[0];
  if (total < 0 || total > n) return fail(APDGICP_ERR_INTERNAL, "approximate voxel filter failed");
  s->n_last = total, s->last_is_cat = false;  // (AV6: no bounding box, no leaf that is too small)
  *n_out = total;
  return 0;
}

int apdgicp_submap_assemble(apdgicp_submap* s, int n_clouds, const void* const* xyz, const int64_t* n_points, int64_t stride_bytes,
                            int64_t intensity_offset_bytes, int on_device, const double* rel_poses, const float* leaf, int64_t* n_out) {
  return guarded([&]() -> int {
    if (!s || !xyz || !n_points || !n_out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (n_clouds < 1 || n_clouds > 4096) return fail(APDGICP_ERR_INVALID_ARG, "n_clouds must be in [1, 4096]");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    APD_HIP(hipSetDevice(s->device));
    *n_out = 0;
    s->n_last = 0;
    int64_t total = 0, nmax = 0;
    for (int c = 0; c < n_clouds; c++) {
      if (n_points[c] < 0 || (n_points[c] > 0 && !xyz[c])) return fail(APDGICP_ERR_INVALID_ARG, "bad cloud");
      total += n_points[c], nmax = std::max<int64_t>(nmax, n_points[c]);
    }
    if (total > (1ll << 27)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^27 points");
    if (total == 0) return 0;
    // inputs: device pointers are read in place, host clouds go through one staging buffer
    std::vector<SubmapJob> jobs(n_clouds);
    const int stride_f = (int)(stride_bytes / 4);
    if (!on_device) {
      APD_HIP(hipStreamSynchronize(s->stream));  // the staging buffer may still be read by the previous call
      APD_TRY(s->stage.ensure((size_t)total * stride_bytes));
    }
    int64_t off = 0;
    for (int c = 0; c < n_clouds; c++) {
      SubmapJob& j = jobs[c];
      memset(&j, 0, sizeof(j));
      j.n = n_points[c], j.stride = stride_f, j.out_off = (int)off;
      j.intensity_off = intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1;
      if (on_device) {
        j.xyz = (const float*)xyz[c];
      } else {
        float* dst = s->stage.as<float>() + off * stride_f;
        // the last point may be shorter than the stride in the caller's buffer: copy up to its last used float only
        const size_t used = std::max<int64_t>(12, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 12);
        if (j.n > 0) APD_HIP(hipMemcpyAsync(dst, xyz[c], (size_t)(j.n - 1) * stride_bytes + used, hipMemcpyHostToDevice, s->stream));
        j.xyz = dst;
      }
      for (int r = 0; r < 3; r++)
        for (int q = 0; q < 4; q++) j.T[4 * r + q] = rel_poses ? rel_poses[(size_t)c * 16 + r + 4 * q] : (r == q ? 1.0 : 0.0);
      off += j.n;
    }
    APD_TRY(s->jobs.upload(jobs.data(), jobs.size() * sizeof(SubmapJob), s->stream));
    const int n = (int)total;
    APD_TRY(s->cat.ensure((size_t)n * 16));
    hipLaunchKernelGGL(k_submap_transform, dim3((unsigned)((nmax + 255) / 256), (unsigned)n_clouds), dim3(256), 0, s->stream,
                       s->jobs.as<SubmapJob>(), s->cat.as<float4>());
    APD_HIP(hipGetLastError());
    if (!leaf || !(leaf[0] > 0.f)) {  // downsample_method NONE: downsample() returns the cloud itself (:413-415)
      APD_HIP(hipStreamSynchronize(s->stream));
      s->n_last = n, s->last_is_cat = true;
      *n_out = n;
      return 0;
    }
    if (!(leaf[1] > 0.f) || !(leaf[2] > 0.f)) return fail(APDGICP_ERR_INVALID_ARG, "leaf sizes must be positive");
    const float il[3] = {1.f / leaf[0], 1.f / leaf[1], 1.f / leaf[2]};  // inverse_leaf_size_ = Array4f::Ones() / leaf_size_
    if (s->method == APDGICP_DOWNSAMPLE_APPROX_VOXELGRID) return submap_approx_voxel(s, n, il, n_out);
    const int np2 = bitonic_padded_size(n);
    const int nsb = (np2 + SCAN_BLK * SCAN_ITEMS - 1) / (SCAN_BLK * SCAN_ITEMS);
    APD_TRY(s->keys.ensure((size_t)np2 * 8));
    APD_TRY(s->pos.ensure((size_t)np2 * 4));
    APD_TRY(s->bsum.ensure((size_t)nsb * 4));
    APD_TRY(s->out.ensure((size_t)n * 16));
    int* box6 = s->scal.as<int>();
    int* d_total = box6 + 6;
    int* d_err = box6 + 7;
    const int init[8] = {0x7f800000, 0x7f800000, 0x7f800000, (int)0x807fffff, (int)0x807fffff, (int)0x807fffff, 0, 0};
    APD_HIP(hipMemcpyAsync(box6, init, sizeof(init), hipMemcpyHostToDevice, s->stream));  // pageable source: staged before the call returns
    hipLaunchKernelGGL(k_vox_bbox, dim3(std::min((n + 255) / 256, 256)), dim3(256), 0, s->stream, s->cat.as<float4>(), n, box6);
    unsigned long long* keys = s->keys.as<unsigned long long>();
    hipLaunchKernelGGL(k_vox_keys, dim3((np2 + 255) / 256), dim3(256), 0, s->stream, s->cat.as<float4>(), n, np2, box6, il[0], il[1], il[2], keys, d_err);
    enqueue_bitonic_sort(s->stream, keys, np2);
    hipLaunchKernelGGL(k_vox_heads, dim3(nsb), dim3(SCAN_BLK), 0, s->stream, keys, np2, s->pos.as<int>(), s->bsum.as<int>());
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, s->stream, s->bsum.as<int>(), nsb, d_total);
    hipLaunchKernelGGL(k_vox_centroids, dim3((np2 + 255) / 256), dim3(256), 0, s->stream, keys, s->cat.as<float4>(), s->pos.as<int>(),
                       s->bsum.as<int>(), np2, s->out.as<float4>(), n);
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(s->h_scal.p, d_total, 2 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    APD_HIP(hipStreamSynchronize(s->stream));
    if (s->h_scal.as<int>()[1] == 5) {
      // pcl::VoxelGrid::applyFilter (filters/impl/voxel_grid.hpp): "Leaf size is too small for the input dataset. Integer indices would
      // overflow." is a WARNING there and the output is the input cloud, unfiltered -- so is it here: the assembled (transformed,
      // concatenated) cloud itself, the same line on stderr, success; apdgicp_last_error() holds the message.
      std::fprintf(stderr, "[apdgicp_submap_assemble] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
      g_last_error = "leaf size is too small for the extent of the submap (voxel index overflows int32): the unfiltered cloud is returned, like pcl::VoxelGrid";
      APD_HIP(hipMemsetAsync(d_err, 0, sizeof(int), s->stream));
      s->n_last = n, s->last_is_cat = true;
      *n_out = n;
      return 0;
    }
    if (s->h_scal.as<int>()[1]) return fail(APDGICP_ERR_INTERNAL, "voxel filter failed");
    s->n_last = s->h_scal.as<int>()[0], s->last_is_cat = false;
    *n_out = s->n_last;
    return 0;
  });
}

int apdgicp_submap_points(apdgicp_submap* s, const float** device_xyzi, int64_t* n) {
  if (!s || !device_xyzi || !n) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *device_xyzi = s->n_last ? (s->last_is_cat ? s->cat.as<float>() : s->out.as<float>()) : nullptr;
  *n = s->n_last;
  return 0;
}

int apdgicp_submap_copy(apdgicp_submap* s, float* dst_xyzi, int64_t capacity_points, int dst_on_device) {
  return guarded([&]() -> int {
    if (!s || !dst_xyzi) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (capacity_points < s->n_last) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the assembled cloud");
    if (!s->n_last) return 0;
    APD_HIP(hipSetDevice(s->device));
    const float* src = s->last_is_cat ? s->cat.as<float>() : s->out.as<float>();
    APD_HIP(hipMemcpyAsync(dst_xyzi, src, (size_t)s->n_last * 16, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s->stream));
    APD_HIP(hipStreamSynchronize(s->stream));
    return 0;
  });
}

// ------------------------------------------------------------------ scan preprocessing (apd_filter.hpp)
void apdgicp_scan_filter_default_params(apdgicp_scan_filter_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->use_distance_filter = 1, p->near = 1.0, p->far = 100.0, p->z_low = -5.0, p->z_high = 20.0;  // preprocessing_nodelet.cpp:201-205
  p->leaf[0] = p->leaf[1] = p->leaf[2] = 0.1f;                                                   // :137-144
  p->outlier_method = APDGICP_OUTLIER_STATISTICAL, p->mean_k = 20, p->stddev_mul = 1.0;          // :166-175
  p->radius = 0.8, p->min_neighbors = 2;                                                         // :176-184
}

static int scan_filter_check_params(const apdgicp_scan_filter_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "params is null");
  if (p->leaf[0] > 0.f && (!(p->leaf[1] > 0.f) || !(p->leaf[2] > 0.f))) return fail(APDGICP_ERR_INVALID_ARG, "leaf sizes must be positive");
  if (p->downsample_method != APDGICP_DOWNSAMPLE_VOXELGRID && p->downsample_method != APDGICP_DOWNSAMPLE_APPROX_VOXELGRID)
    return fail(APDGICP_ERR_INVALID_ARG, "unknown downsample method");
  if (p->outlier_method == APDGICP_OUTLIER_STATISTICAL) {
    if (p->mean_k < 1) return fail(APDGICP_ERR_INVALID_ARG, "mean_k must be >= 1");
    if (p->mean_k + 1 > KNN_NC) return fail(APDGICP_ERR_UNSUPPORTED, "mean_k above 31");
    if (!std::isfinite(p->stddev_mul)) return fail(APDGICP_ERR_INVALID_ARG, "stddev_mul is not finite");
  } else if (p->outlier_method == APDGICP_OUTLIER_RADIUS) {
    if (p->min_neighbors < 0) return fail(APDGICP_ERR_INVALID_ARG, "min_neighbors must be >= 0");
    if (p->min_neighbors + 1 > KNN_NC) return fail(APDGICP_ERR_UNSUPPORTED, "min_neighbors above 31");
    if (!(p->radius > 0.0)) return fail(APDGICP_ERR_INVALID_ARG, "radius must be positive");
  } else if (p->outlier_method != APDGICP_OUTLIER_NONE) {
    return fail(APDGICP_ERR_UNSUPPORTED, "unknown outlier removal method");
  }
  return 0;
}

int apdgicp_scan_filter_create(const apdgicp_scan_filter_params* p, int device, void* stream, apdgicp_scan_filter** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_scan_filter_params dflt;
    apdgicp_scan_filter_default_params(&dflt);
    if (!p) p = &dflt;
    APD_TRY(scan_filter_check_params(p));
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_scan_filter> f(new apdgicp_scan_filter);
    f->device = device, f->prm = *p;
    if (stream) {
      f->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
      f->own_stream = true;
    }
    APD_TRY(f->h_scal.ensure(64));
    APD_TRY(f->scal.ensure(64));
    APD_TRY(apdgicp_submap_create(device, f->stream, &f->vox));
    *out = f.release();
    return 0;
  });
}

int apdgicp_scan_filter_destroy(apdgicp_scan_filter* f) {
  return guarded([&]() -> int {
    if (f) (void)hipSetDevice(f->device);
    delete f;
    return 0;
  });
}

int apdgicp_scan_filter_set_params(apdgicp_scan_filter* f, const apdgicp_scan_filter_params* p) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(scan_filter_check_params(p));
    f->prm = *p;
    return 0;
  });
}

int apdgicp_scan_filter_run(apdgicp_scan_filter* f, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device,
                            int64_t* n_out) {
  return guarded([&]() -> int {
    if (!f || !n_out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    f->result = nullptr, f->n_stat = 0, f->mean = f->stddev = f->thr = 0;
    f->counts[0] = f->counts[1] = f->counts[2] = f->counts[3] = 0;
    if (n < 0 || (n > 0 && !xyz)) return fail(APDGICP_ERR_INVALID_ARG, "bad cloud");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    if (n > (1ll << 27)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^27 points");
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(f->device));
    const apdgicp_scan_filter_params& P = f->prm;
    const int ni = (int)n;
    f->counts[0] = n;
    // ---- input: device pointers are read in place, a host scan goes through the staging buffer
    const float* d_in = xyz;
    if (!on_device) {
      APD_HIP(hipStreamSynchronize(f->stream));  // the staging buffer may still be read by the previous run
      APD_TRY(f->stage.ensure((size_t)n * stride_bytes));
      const size_t used = std::max<int64_t>(12, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 12);
      APD_HIP(hipMemcpyAsync(f->stage.p, xyz, (size_t)(n - 1) * stride_bytes + used, hipMemcpyHostToDevice, f->stream));
      d_in = f->stage.as<float>();
    }
    int* d_counts = f->scal.as<int>();
    double* d_thr = (double*)(f->scal.as<char>() + 16);
    int* h_counts = f->h_scal.as<int>();
    APD_TRY(f->gated.ensure((size_t)n * 16));
    APD_TRY(f->bsum.ensure((size_t)((n + FLT_BLK - 1) / FLT_BLK) * 4));
    APD_HIP(hipMemsetAsync(f->scal.p, 0, 64, f->stream));
    // ---- 1. distance_filter (:881-889)
    GateParams g;
    g.near_ = P.near, g.far_ = P.far, g.z_low = P.z_low, g.z_high = P.z_high, g.on = P.use_distance_filter ? 1 : 0, g.pad_ = 0;
    hipLaunchKernelGGL(k_flt_gate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, f->stream, d_in, (long long)n, (int)(stride_bytes / 4),
                       intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1, g, f->gated.as<float4>(), d_counts);
    APD_HIP(hipGetLastError());
    // ---- 2. downsample (:850-866)
    const float4* step2 = nullptr;
    int n2 = -1;  // < 0: still on the device (d_counts[1])
    if (P.leaf[0] > 0.f) {
      const void* src = f->gated.p;
      int64_t nn = n, nv = 0;
      APD_TRY(apdgicp_submap_set_downsample_method(f->vox, P.downsample_method));
      APD_TRY(apdgicp_submap_assemble(f->vox, 1, &src, &nn, 16, 12, 1, nullptr, P.leaf, &nv));
      if (!f->vox->last_is_cat) step2 = f->vox->out.as<float4>(), n2 = (int)nv;  // (else: leaf too small, PCL returns its input: compacted below)
    }
    if (!step2) {  // removeNaNFromPointCloud (:852-857) / what the range gate left, in input order
      APD_TRY(f->dense.ensure((size_t)n * 16));
      APD_TRY((scan_filter_compact<0>(f, f->gated.as<float4>(), nullptr, 0.0, nullptr, ni, f->dense.as<float4>(), nullptr, d_counts + 1)));
      step2 = f->dense.as<float4>();
    }
    auto read_back = [&](bool with_engine_flag) -> int {
      APD_HIP(hipMemcpyAsync(f->h_scal.p, f->scal.p, 40, hipMemcpyDeviceToHost, f->stream));
      if (with_engine_flag) APD_HIP(hipMemcpyAsync(f->h_scal.as<char>() + 40, f->eng->d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, f->stream));
      APD_HIP(hipStreamSynchronize(f->stream));
      return 0;
    };
    if (n2 < 0 || P.outlier_method == APDGICP_OUTLIER_NONE) {
      APD_TRY(read_back(false));
      if (n2 < 0) n2 = h_counts[1];
    }
    f->counts[2] = n2;
    if (P.outlier_method == APDGICP_OUTLIER_NONE || n2 == 0) {
      if (P.outlier_method != APDGICP_OUTLIER_NONE && P.leaf[0] > 0.f && !f->vox->last_is_cat) APD_TRY(read_back(false));  // (the gate's count)
      f->counts[1] = h_counts[0], f->counts[3] = n2;
      f->result = n2 ? (const float*)step2 : nullptr;
      *n_out = n2;
      return 0;
    }
    // ---- 3. outlier_removal (:868-879)
    const bool statistical = P.outlier_method == APDGICP_OUTLIER_STATISTICAL;
    const int k = statistical ? P.mean_k + 1 : P.min_neighbors + 1;
    if (n2 < k) return fail(APDGICP_ERR_TOO_FEW_POINTS, "the downsampled scan has fewer points than the outlier filter's k");
    apdgicp_params ep;
    apdgicp_default_params(&ep);
    ep.k_correspondences = k;
    if (!f->eng) {
      std::unique_ptr<Engine> e(new Engine);
      APD_TRY(e->init(&ep, f->device, f->stream));
      f->eng = e.release();
    } else {
      APD_TRY(f->eng->set_params(&ep));
    }
    Engine& E = *f->eng;
    APD_TRY(E.set_cloud(0, (const float*)step2, n2, 16, 1, 0));  // pack, and (upload_desc) curve sort + 16 / 128 / 8192-point boxes
    APD_TRY(E.upload_desc());
    const int id0 = 0;
    APD_TRY(E.d_ids.upload(&id0, sizeof(int), f->stream));
    APD_TRY(f->stat.ensure((size_t)n2 * 4));
    APD_TRY(f->kept.ensure((size_t)n2));
    APD_TRY(f->out.ensure((size_t)n2 * 16));
    const CloudDesc* desc = E.d_desc.as<CloudDesc>();
    const int* ids = E.d_ids.as<int>();
    int* eflag = E.d_errflag.as<int>();
    float* stat = f->stat.as<float>();
    if (E.knn_pruned) {
      const dim3 grid((unsigned)((n2 + 3) / 4), 1u);
      if (statistical)
        hipLaunchKernelGGL(k_knn_stat_coop<KNN_EPI_MEANDIST>, grid, dim3(64), knn_coop_lds_bytes(4), f->stream, desc, ids, k, eflag, E.d_stats.as<unsigned long long>(), stat);
      else
        hipLaunchKernelGGL(k_knn_stat_coop<KNN_EPI_KTH>, grid, dim3(64), knn_coop_lds_bytes(4), f->stream, desc, ids, k, eflag, E.d_stats.as<unsigned long long>(), stat);
    } else {
      const dim3 grid((unsigned)((n2 + STAT_BRUTE_BLK - 1) / STAT_BRUTE_BLK), 1u);
      if (statistical) hipLaunchKernelGGL(k_knn_stat_brute<KNN_EPI_MEANDIST>, grid, dim3(STAT_BRUTE_BLK), 0, f->stream, desc, ids, k, eflag, stat);
      else hipLaunchKernelGGL(k_knn_stat_brute<KNN_EPI_KTH>, grid, dim3(STAT_BRUTE_BLK), 0, f->stream, desc, ids, k, eflag, stat);
    }
    APD_HIP(hipGetLastError());
    const double r2 = P.radius * P.radius;
    if (statistical) hipLaunchKernelGGL(k_flt_threshold, dim3(1), dim3(FLT_BLK), 0, f->stream, stat, n2, P.stddev_mul, d_thr);
    APD_TRY((scan_filter_compact<1>(f, step2, stat, r2, statistical ? d_thr + 2 : nullptr, n2, f->out.as<float4>(), f->kept.as<unsigned char>(), d_counts + 2)));
    APD_TRY(read_back(true));
    const int flag = *(int*)(f->h_scal.as<char>() + 40);
    if (flag) {
      APD_HIP(hipMemsetAsync(E.d_errflag.p, 0, sizeof(int), f->stream));
      return fail(APDGICP_ERR_INTERNAL, "outlier filter k-NN: " + Engine::errflag_text(flag));
    }
    const double* h_thr = (const double*)(f->h_scal.as<char>() + 16);
    f->n_stat = n2;
    if (statistical) f->mean = h_thr[0], f->stddev = h_thr[1], f->thr = h_thr[2];
    else f->thr = r2;
    f->counts[1] = h_counts[0], f->counts[3] = h_counts[2];
    f->result = h_counts[2] ? f->out.as<float>() : nullptr;
    *n_out = h_counts[2];
    return 0;
  });
}

int apdgicp_scan_filter_points(apdgicp_scan_filter* f, const float** device_xyzi, int64_t* n) {
  return guarded([&]() -> int {
    if (!f || !device_xyzi || !n) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *device_xyzi = f->result;
    *n = f->result ? f->counts[3] : 0;
    return 0;
  });
}

int apdgicp_scan_filter_copy(apdgicp_scan_filter* f, float* dst_xyzi, int64_t capacity_points, int dst_on_device) {
  return guarded([&]() -> int {
    if (!f || (!dst_xyzi && capacity_points > 0)) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t n = f->result ? f->counts[3] : 0;
    if (capacity_points < n) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the filtered scan");
    if (!n) return 0;
    APD_HIP(hipSetDevice(f->device));
    APD_HIP(hipMemcpyAsync(dst_xyzi, f->result, (size_t)n * 16, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));
    return 0;
  });
}

int apdgicp_scan_filter_stage_counts(apdgicp_scan_filter* f, int64_t counts[4]) {
  return guarded([&]() -> int {
    if (!f || !counts) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    for (int q = 0; q < 4; q++) counts[q] = f->counts[q];
    return 0;
  });
}

int apdgicp_scan_filter_scores(apdgicp_scan_filter* f, float* stat, uint8_t* kept, int64_t capacity, double* mean, double* stddev, double* thr) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if ((stat || kept) && capacity < f->n_stat) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer entries than the cloud behind downsample");
    if (mean) *mean = f->mean;
    if (stddev) *stddev = f->stddev;
    if (thr) *thr = f->thr;
    if (!f->n_stat || (!stat && !kept)) return 0;
    APD_HIP(hipSetDevice(f->device));
    if (stat) APD_HIP(hipMemcpyAsync(stat, f->stat.p, (size_t)f->n_stat * 4, hipMemcpyDeviceToHost, f->stream));
    if (kept) APD_HIP(hipMemcpyAsync(kept, f->kept.p, (size_t)f->n_stat, hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));
    return 0;
  });
}

// ------------------------------------------------------------------ Doppler ego velocity (apd_ego.hpp)
static_assert(sizeof(apdgicp_ego_velocity_result) == 88 && offsetof(EgoRecord, mode) == sizeof(apdgicp_ego_velocity_result), "EgoRecord starts with the result");

void apdgicp_ego_velocity_default_params(apdgicp_ego_velocity_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_dist = 0.1f, p->max_dist = 400.f, p->min_db = 5.f, p->elevation_thresh_deg = 60.f, p->azimuth_thresh_deg = 120.f;  // EH:32-36
  p->doppler_velocity_correction_factor = 1.f;                                                                          // EH:37
  p->thresh_zero_velocity = 0.05f, p->allowed_outlier_percentage = 0.30f;                                               // EH:39-40
  p->sigma_zero_velocity_x = 1.0e-03f, p->sigma_zero_velocity_y = 3.2e-03f, p->sigma_zero_velocity_z = 1.0e-02f;        // EH:41-43
  p->max_sigma_x = p->max_sigma_y = p->max_sigma_z = 0.2f;                                                              // EH:49-51
  p->max_r_cond = 1000.f;                                                                                               // EH:52 (uninitialised there)
  p->use_cholesky_instead_of_bdcsvd = 1, p->use_ransac = 1;                                                             // EH:53, 55
  p->outlier_prob = 0.05f, p->success_prob = 0.995f, p->N_ransac_points = 5, p->inlier_thresh = 0.5f;                   // EH:56-59
}

int apdgicp_ego_velocity_hypothesis_count(const apdgicp_ego_velocity_params* p, int32_t* K) {
  if (!p || !K) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *K = 0;
  if (p->n_hypotheses < 0 || p->n_hypotheses > EGO_MAX_K) return fail(APDGICP_ERR_INVALID_ARG, "n_hypotheses must be 0 .. 1024");
  if (p->n_hypotheses) {
    *K = p->n_hypotheses;
    return 0;
  }
  // setRansacIter, EH:138-143: the float fields widened to double, the quotient truncated to uint
  const double it = std::log(1.0 - (double)p->success_prob) / std::log(1.0 - std::pow(1.0 - (double)p->outlier_prob, (double)(float)p->N_ransac_points));
  if (!(it >= 0.0)) return fail(APDGICP_ERR_INVALID_ARG, "success_prob / outlier_prob give no number of RANSAC iterations");
  if (it >= (double)EGO_MAX_K + 1.0) return fail(APDGICP_ERR_UNSUPPORTED, "setRansacIter's formula gives more than 1024 hypotheses: set n_hypotheses");
  *K = (int32_t)it;
  return 0;
}

static int ego_check_params(const apdgicp_ego_velocity_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "params is null");
  if (!p->use_cholesky_instead_of_bdcsvd) return fail(APDGICP_ERR_UNSUPPORTED, "use_cholesky_instead_of_bdcsvd = false (bdcSvd) is not offered");
  if (p->N_ransac_points < 3 || p->N_ransac_points > EGO_MAX_S) return fail(APDGICP_ERR_INVALID_ARG, "N_ransac_points must be 3 .. 8");
  if (!(p->allowed_outlier_percentage >= 0.f && p->allowed_outlier_percentage <= 1.f)) return fail(APDGICP_ERR_INVALID_ARG, "allowed_outlier_percentage must be 0 .. 1");
  int32_t K = 0;
  if (p->use_ransac) APD_TRY(apdgicp_ego_velocity_hypothesis_count(p, &K));
  return 0;
}

int apdgicp_ego_velocity_create(const apdgicp_ego_velocity_params* p, int device, void* stream, apdgicp_ego_velocity** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_ego_velocity_params dflt;
    apdgicp_ego_velocity_default_params(&dflt);
    if (!p) p = &dflt;
    APD_TRY(ego_check_params(p));
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_ego_velocity> e(new apdgicp_ego_velocity);
    e->device = device, e->prm = *p;
    if (stream) {
      e->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
      e->own_stream = true;
    }
    APD_TRY(e->h_rec.ensure(sizeof(EgoRecord)));
    memset(e->h_rec.p, 0, sizeof(EgoRecord));
    APD_TRY(e->rec.ensure(sizeof(EgoRecord)));
    APD_TRY(e->vk.ensure((size_t)EGO_MAX_K * 3 * sizeof(double)));
    APD_TRY(e->n_in.ensure((size_t)EGO_MAX_K * sizeof(int)));
    APD_TRY(e->samples.ensure((size_t)EGO_MAX_K * EGO_MAX_S * sizeof(int)));
    APD_TRY(e->words.ensure((size_t)EGO_MAX_K * EGO_MAX_S * sizeof(unsigned)));
    *out = e.release();
    return 0;
  });
}

int apdgicp_ego_velocity_destroy(apdgicp_ego_velocity* e) {
  return guarded([&]() -> int {
    if (e) (void)hipSetDevice(e->device);
    delete e;
    return 0;
  });
}

int apdgicp_ego_velocity_set_params(apdgicp_ego_velocity* e, const apdgicp_ego_velocity_params* p) {
  return guarded([&]() -> int {
    if (!e) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(ego_check_params(p));
    e->prm = *p;
    return 0;
  });
}

int apdgicp_ego_velocity_run(apdgicp_ego_velocity* e, const float* pts, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes,
                             int64_t doppler_offset_bytes, int on_device, const uint32_t* words, int64_t n_words, apdgicp_ego_velocity_result* result) {
  return guarded([&]() -> int {
    if (!e || !result) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    memset(result, 0, sizeof(*result));
    result->best_in = result->best_out = -1;
    e->ran = false, e->n_last = 0;
    memset(e->h_rec.p, 0, sizeof(EgoRecord));
    if (n < 0 || (n > 0 && !pts)) return fail(APDGICP_ERR_INVALID_ARG, "bad cloud");
    if (stride_bytes < 20 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 20");
    for (int64_t off : {intensity_offset_bytes, doppler_offset_bytes})
      if (off < 12 || off % 4 || off + 4 > stride_bytes) return fail(APDGICP_ERR_INVALID_ARG, "intensity / doppler offset outside the point");
    if (n > (1ll << 24)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    const apdgicp_ego_velocity_params& P = e->prm;
    int32_t K = 0;
    if (P.use_ransac) APD_TRY(apdgicp_ego_velocity_hypothesis_count(&P, &K));
    const int S = P.N_ransac_points;
    if (K > 0 && (n_words < (int64_t)K * S || !words)) return fail(APDGICP_ERR_INVALID_ARG, "fewer random words than hypotheses x N_ransac_points");
    result->K = K;
    e->K_last = K, e->S_last = S;
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(e->device));
    const int ni = (int)n, nb = (ni + EGO_BLK - 1) / EGO_BLK;
    const float* d_in = pts;
    if (!on_device) {
      // (no wait: the copy below is ordered behind the previous run's kernels by the stream; a buffer that grows is freed by hipFree, which waits)
      APD_TRY(e->stage.ensure((size_t)n * stride_bytes));
      const size_t used = (size_t)std::max<int64_t>(12, std::max(intensity_offset_bytes, doppler_offset_bytes) + 4);
      APD_HIP(hipMemcpyAsync(e->stage.p, pts, (size_t)(n - 1) * stride_bytes + used, hipMemcpyHostToDevice, e->stream));
      d_in = e->stage.as<float>();
    }
    APD_TRY(e->rows_all.ensure((size_t)n * 32));
    APD_TRY(e->rows.ensure((size_t)n * 32));
    APD_TRY(e->valid.ensure((size_t)n));
    APD_TRY(e->bsum.ensure((size_t)nb * 3 * sizeof(int)));
    for (DevBuf* b : {&e->src, &e->in_row, &e->in_dop, &e->in_src, &e->out_row, &e->out_dop, &e->out_src}) APD_TRY(b->ensure((size_t)n * 4));
    APD_TRY(e->in_xyzi.ensure((size_t)n * 16));
    APD_TRY(e->out_xyzi.ensure((size_t)n * 16));
    EgoParams D;
    memset(&D, 0, sizeof(D));
    D.min_dist = (double)P.min_dist, D.max_dist = (double)P.max_dist, D.min_db = P.min_db;
    D.az_thr = (double)P.azimuth_thresh_deg * M_PI / 180.0, D.el_thr = (double)P.elevation_thresh_deg * M_PI / 180.0;  // angles::from_degrees
    D.factor = P.doppler_velocity_correction_factor, D.thresh_zero = P.thresh_zero_velocity;
    D.allowed_outlier_percentage = (double)P.allowed_outlier_percentage, D.inlier_thresh = (double)P.inlier_thresh;
    D.sigma_zero[0] = P.sigma_zero_velocity_x, D.sigma_zero[1] = P.sigma_zero_velocity_y, D.sigma_zero[2] = P.sigma_zero_velocity_z;
    D.sigma_offset[0] = P.sigma_offset_radar_x, D.sigma_offset[1] = P.sigma_offset_radar_y, D.sigma_offset[2] = P.sigma_offset_radar_z;
    D.max_sigma[0] = P.max_sigma_x, D.max_sigma[1] = P.max_sigma_y, D.max_sigma[2] = P.max_sigma_z;
    D.use_ransac = P.use_ransac ? 1 : 0, D.S = S, D.K = K;
    EgoRecord* rec = e->rec.as<EgoRecord>();
    int* bsum = e->bsum.as<int>();
    const int stride = (int)(stride_bytes / 4), ioff = (int)(intensity_offset_bytes / 4), doff = (int)(doppler_offset_bytes / 4);
    double4* rows = e->rows.as<double4>();
    double* vk = e->vk.as<double>();
    APD_HIP(hipMemsetAsync(e->rec.p, 0, sizeof(EgoRecord), e->stream));
    if (K > 0) {
      APD_HIP(hipMemcpyAsync(e->words.p, words, (size_t)K * S * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
      APD_HIP(hipMemsetAsync(e->n_in.p, 0, (size_t)EGO_MAX_K * sizeof(int), e->stream));
      APD_HIP(hipMemsetAsync(e->vk.p, 0, (size_t)EGO_MAX_K * 3 * sizeof(double), e->stream));
    }
    // 1. features + in-order compaction (m -> the record)
    hipLaunchKernelGGL(k_ego_features, dim3(nb), dim3(EGO_BLK), 0, e->stream, d_in, ni, stride, ioff, doff, D, e->rows_all.as<double4>(), e->valid.as<unsigned char>(), bsum);
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, e->stream, bsum, nb, &rec->m);
    hipLaunchKernelGGL(k_ego_compact, dim3(nb), dim3(EGO_BLK), 0, e->stream, e->rows_all.as<double4>(), e->valid.as<unsigned char>(), ni, bsum, rows, e->src.as<int>());
    // 2. zero velocity; decides the mode of everything below
    hipLaunchKernelGGL(k_ego_zero_velocity, dim3(1), dim3(EGO_BLK), 0, e->stream, rows, D, rec);
    // 3. - 5. hypotheses, scores, the two best
    if (K > 0) {
      hipLaunchKernelGGL(k_ego_hypotheses, dim3((K + 63) / 64), dim3(64), 0, e->stream, rows, e->words.as<unsigned>(), D, rec, vk, e->samples.as<int>());
      hipLaunchKernelGGL(k_ego_score, dim3((ni + EGO_TILE - 1) / EGO_TILE, (K + EGO_GROUP - 1) / EGO_GROUP), dim3(EGO_TILE), 0, e->stream, rows, vk, D, rec, e->n_in.as<int>());
      hipLaunchKernelGGL(k_ego_select, dim3(1), dim3(EGO_BLK), 0, e->stream, e->n_in.as<int>(), D, rec);
    }
    // the lists and the clouds, then 6. the fit
    hipLaunchKernelGGL(k_ego_emit_count, dim3(nb), dim3(EGO_BLK), 0, e->stream, rows, vk, D, rec, bsum + nb, bsum + 2 * nb);
    hipLaunchKernelGGL(k_ego_emit_scan, dim3(1), dim3(SCAN_BLK), 0, e->stream, bsum + nb, bsum + 2 * nb, nb, rec);
    hipLaunchKernelGGL(k_ego_emit_scatter, dim3(nb), dim3(EGO_BLK), 0, e->stream, rows, e->src.as<int>(), vk, D, rec, bsum + nb, bsum + 2 * nb, d_in, stride, ioff,
                       e->in_row.as<int>(), e->in_xyzi.as<float4>(), e->in_dop.as<float>(), e->in_src.as<int>(), e->out_row.as<int>(), e->out_xyzi.as<float4>(),
                       e->out_dop.as<float>(), e->out_src.as<int>());
    hipLaunchKernelGGL(k_ego_lsq, dim3(1), dim3(EGO_BLK), 0, e->stream, rows, e->in_row.as<int>(), D, rec);
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(e->h_rec.p, e->rec.p, sizeof(EgoRecord), hipMemcpyDeviceToHost, e->stream));
    APD_HIP(hipStreamSynchronize(e->stream));  // the one wait of the call
    memcpy(result, e->h_rec.p, sizeof(*result));
    if (e->record()->mode != EGO_MODE_RANSAC) result->best_in = result->best_out = -1;
    result->K = K;
    e->n_last = n, e->ran = true;
    return 0;
  });
}

static int ego_cloud(apdgicp_ego_velocity* e, int which, const float** xyzi, const float** dop, const int32_t** index, int64_t* n) {
  if (!e || which < 0 || which > 1) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
  const int64_t cnt = e->ran ? (which ? e->record()->n_outlier : e->record()->n_inlier) : 0;
  if (xyzi) *xyzi = cnt ? (which ? e->out_xyzi : e->in_xyzi).as<float>() : nullptr;
  if (dop) *dop = cnt ? (which ? e->out_dop : e->in_dop).as<float>() : nullptr;
  if (index) *index = cnt ? (which ? e->out_src : e->in_src).as<int32_t>() : nullptr;
  if (n) *n = cnt;
  return 0;
}
int apdgicp_ego_velocity_inliers(apdgicp_ego_velocity* e, const float** device_xyzi, const float** device_doppler, const int32_t** device_index, int64_t* n) {
  return guarded([&]() -> int { return ego_cloud(e, 0, device_xyzi, device_doppler, device_index, n); });
}
int apdgicp_ego_velocity_outliers(apdgicp_ego_velocity* e, const float** device_xyzi, const float** device_doppler, const int32_t** device_index, int64_t* n) {
  return guarded([&]() -> int { return ego_cloud(e, 1, device_xyzi, device_doppler, device_index, n); });
}

int apdgicp_ego_velocity_copy(apdgicp_ego_velocity* e, int which, float* xyzi, float* doppler, int32_t* index, int32_t* row, int64_t capacity) {
  return guarded([&]() -> int {
    int64_t n = 0;
    APD_TRY(ego_cloud(e, which, nullptr, nullptr, nullptr, &n));
    if (capacity < n) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the cloud");
    if (!n) return 0;
    APD_HIP(hipSetDevice(e->device));
    if (xyzi) APD_HIP(hipMemcpyAsync(xyzi, (which ? e->out_xyzi : e->in_xyzi).p, (size_t)n * 16, hipMemcpyDeviceToHost, e->stream));
    if (doppler) APD_HIP(hipMemcpyAsync(doppler, (which ? e->out_dop : e->in_dop).p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    if (index) APD_HIP(hipMemcpyAsync(index, (which ? e->out_src : e->in_src).p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    if (row) APD_HIP(hipMemcpyAsync(row, (which ? e->out_row : e->in_row).p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    APD_HIP(hipStreamSynchronize(e->stream));
    return 0;
  });
}

int apdgicp_ego_velocity_hypotheses(apdgicp_ego_velocity* e, double* v_k, int32_t* n_in, int64_t capacity) {
  return guarded([&]() -> int {
    if (!e) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int K = e->ran ? e->K_last : 0;
    if ((v_k || n_in) && capacity < K) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer entries than hypotheses");
    if (!K) return 0;
    APD_HIP(hipSetDevice(e->device));
    if (v_k) APD_HIP(hipMemcpyAsync(v_k, e->vk.p, (size_t)K * 3 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (n_in) APD_HIP(hipMemcpyAsync(n_in, e->n_in.p, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    APD_HIP(hipStreamSynchronize(e->stream));
    return 0;
  });
}

int apdgicp_ego_velocity_debug(apdgicp_ego_velocity* e, uint8_t* valid, int64_t valid_capacity, double* rows, int64_t rows_capacity, int32_t* samples,
                               int64_t samples_capacity, float* selected_abs_v) {
  return guarded([&]() -> int {
    if (!e) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int m = e->ran ? e->record()->m : 0;
    if (e->ran && ((valid && valid_capacity < e->n_last) || (rows && rows_capacity < m) ||
                   (samples && e->record()->mode == EGO_MODE_RANSAC && samples_capacity < (int64_t)e->K_last * e->S_last)))
      return fail(APDGICP_ERR_INVALID_ARG, "a destination holds fewer entries than the last run produced");
    if (selected_abs_v) memcpy(selected_abs_v, &e->record()->sel_bits, 4);
    if (!e->ran) return 0;
    APD_HIP(hipSetDevice(e->device));
    if (valid) APD_HIP(hipMemcpyAsync(valid, e->valid.p, (size_t)e->n_last, hipMemcpyDeviceToHost, e->stream));
    if (rows && m) APD_HIP(hipMemcpyAsync(rows, e->rows.p, (size_t)m * 32, hipMemcpyDeviceToHost, e->stream));
    if (samples && e->record()->mode == EGO_MODE_RANSAC)
      APD_HIP(hipMemcpyAsync(samples, e->samples.p, (size_t)e->K_last * e->S_last * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    APD_HIP(hipStreamSynchronize(e->stream));
    return 0;
  });
}

// ------------------------------------------------------------------ floor detection and under-floor removal (apd_floor.hpp)
static_assert(sizeof(apdgicp_floor_result) == 96 && sizeof(FloorRecord) == sizeof(apdgicp_floor_result) && offsetof(FloorRecord, n_inlier_list) == offsetof(apdgicp_floor_result, reserved),
              "FloorRecord is the result (n_inlier_list in its first reserved word)");
static_assert(sizeof(apdgicp_floor_params) == 96, "apdgicp_floor_params layout");

void apdgicp_floor_default_params(apdgicp_floor_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->tilt_deg = 0.0, p->sensor_height = 2.0, p->height_clip_range = 1.0, p->floor_pts_thresh = 50;                         // F:63-66
  p->floor_normal_thresh = 10.0, p->use_normal_filtering = 1, p->normal_filter_thresh = 20.0, p->floor_tolerance = 0.1;  // F:67-70
  p->distance_threshold = 0.06;                                                                                          // F:185
  p->probability = 0.99, p->max_iterations = 1000;                                                                       // pcl::SampleConsensus
  p->normal_k = 10;                                                                                                      // F:288
  p->n_hypotheses = 64;
}

static int floor_check_params(const apdgicp_floor_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "params is null");
  if (p->normal_k < 3 || p->normal_k > 64) return fail(APDGICP_ERR_INVALID_ARG, "normal_k must be 3 .. 64");
  if (p->n_hypotheses < 1 || p->n_hypotheses > FLOOR_MAX_K) return fail(APDGICP_ERR_INVALID_ARG, "n_hypotheses must be 1 .. 1024");
  if (!(p->distance_threshold > 0.0) || !(p->floor_normal_thresh > 0.0) || !(p->normal_filter_thresh > 0.0) || !(p->height_clip_range > 0.0))
    return fail(APDGICP_ERR_INVALID_ARG, "distance_threshold, floor_normal_thresh, normal_filter_thresh and height_clip_range must be positive");
  if (!(p->probability > 0.0 && p->probability < 1.0)) return fail(APDGICP_ERR_INVALID_ARG, "probability must lie inside (0, 1)");
  if (p->max_iterations < 1 || p->floor_pts_thresh < 0) return fail(APDGICP_ERR_INVALID_ARG, "max_iterations must be >= 1 and floor_pts_thresh >= 0");
  if (!std::isfinite(p->tilt_deg) || !std::isfinite(p->sensor_height) || !std::isfinite(p->floor_tolerance)) return fail(APDGICP_ERR_INVALID_ARG, "a parameter is not finite");
  if (p->use_normal_filtering && p->normal_k > KNN_NC) return fail(APDGICP_ERR_UNSUPPORTED, "normal_k above 32");
  return 0;
}

static float floor_initial_d(const apdgicp_floor_params& P) { return (float)(P.sensor_height - P.height_clip_range); }  // F:80

int apdgicp_floor_create(const apdgicp_floor_params* p, int device, void* stream, apdgicp_floor** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_floor_params dflt;
    apdgicp_floor_default_params(&dflt);
    if (!p) p = &dflt;
    APD_TRY(floor_check_params(p));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(APDGICP_ERR_UNSUPPORTED, "no HIP device: floor detection has no CPU path");
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_floor> f(new apdgicp_floor);
    f->device = device, f->prm = *p;
    if (stream) {
      f->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
      f->own_stream = true;
    }
    APD_TRY(f->h_rec.ensure(sizeof(FloorRecord) + 16));
    memset(f->h_rec.p, 0, sizeof(FloorRecord) + 16);
    APD_TRY(f->rec.ensure(sizeof(FloorRecord)));
    APD_TRY(f->state.ensure(sizeof(FloorState)));
    APD_TRY(f->coef.ensure((size_t)FLOOR_MAX_K * sizeof(float4)));
    APD_TRY(f->bad.ensure((size_t)FLOOR_MAX_K));
    APD_TRY(f->n_in.ensure((size_t)FLOOR_MAX_K * sizeof(int)));
    APD_TRY(f->samples.ensure((size_t)FLOOR_MAX_K * 3 * sizeof(int)));
    APD_TRY(f->words.ensure((size_t)FLOOR_MAX_K * 3 * sizeof(unsigned)));
    hipLaunchKernelGGL(k_floor_reset, dim3(1), dim3(64), 0, f->stream, f->state.as<FloorState>(), floor_initial_d(f->prm));
    APD_HIP(hipGetLastError());
    *out = f.release();
    return 0;
  });
}

int apdgicp_floor_destroy(apdgicp_floor* f) {
  return guarded([&]() -> int {
    if (f) (void)hipSetDevice(f->device);
    delete f;
    return 0;
  });
}

int apdgicp_floor_set_params(apdgicp_floor* f, const apdgicp_floor_params* p) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(floor_check_params(p));
    f->prm = *p;
    return 0;
  });
}

int apdgicp_floor_reset(apdgicp_floor* f) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(f->device));
    hipLaunchKernelGGL(k_floor_reset, dim3(1), dim3(64), 0, f->stream, f->state.as<FloorState>(), floor_initial_d(f->prm));
    APD_HIP(hipGetLastError());
    return 0;
  });
}

int apdgicp_floor_run(apdgicp_floor* f, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device, const uint32_t* words,
                      int64_t n_words, apdgicp_floor_result* result) {
  return guarded([&]() -> int {
    if (!f || !result) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    memset(result, 0, sizeof(*result));
    result->winner = -1;
    f->ran = false, f->stat_valid = false, f->n_last = 0;
    memset(f->h_rec.p, 0, sizeof(FloorRecord) + 16);
    if (n < 0 || (n > 0 && !xyz)) return fail(APDGICP_ERR_INVALID_ARG, "bad cloud");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    if (n > (1ll << 24)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    const apdgicp_floor_params& P = f->prm;
    const int K = P.n_hypotheses;
    if (!words || n_words < (int64_t)K * 3) return fail(APDGICP_ERR_INVALID_ARG, "fewer random words than 3 x n_hypotheses");
    result->K = K;
    f->K_last = K;
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(f->device));
    const int ni = (int)n, nb = (ni + FLOOR_BLK - 1) / FLOOR_BLK;
    const float* d_in = xyz;
    if (!on_device) {
      // (no wait: the copy is ordered behind the previous run's kernels by the stream; a buffer that grows is freed by hipFree, which waits)
      APD_TRY(f->stage.ensure((size_t)n * stride_bytes));
      const size_t used = (size_t)std::max<int64_t>(12, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 12);
      APD_HIP(hipMemcpyAsync(f->stage.p, xyz, (size_t)(n - 1) * stride_bytes + used, hipMemcpyHostToDevice, f->stream));
      d_in = f->stage.as<float>();
    }
    for (DevBuf* b : {&f->tilted, &f->clip, &f->filt, &f->in_xyzi, &f->under_xyzi}) APD_TRY(b->ensure((size_t)n * 16));
    for (DevBuf* b : {&f->clip_src, &f->stat, &f->filt_src, &f->in_src, &f->in_row, &f->under_src}) APD_TRY(b->ensure((size_t)n * 4));
    APD_TRY(f->mask.ensure((size_t)n));
    APD_TRY(f->bsum.ensure((size_t)nb * 4 * sizeof(int)));
    FloorParams D;
    memset(&D, 0, sizeof(D));
    {
      const float angle = (float)(P.tilt_deg * M_PI / 180.0f);  // F:157
      const float c = (float)std::cos((double)angle), s = (float)std::sin((double)angle);
      const float R[9] = {c, 0.f, s, 0.f, (1.f - c) + c, 0.f, -s, 0.f, c};
      for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) D.R[3 * r + q] = R[3 * r + q], D.Ri[3 * q + r] = R[3 * r + q];
      D.ref[0] = D.Ri[2], D.ref[1] = D.Ri[5], D.ref[2] = D.Ri[8];  // tilt^-1 * e_z: the third column of the inverse
    }
    D.d_hi = (float)(P.sensor_height + P.height_clip_range), D.d_lo = (float)(P.sensor_height - P.height_clip_range);
    D.cos_nf = std::cos(P.normal_filter_thresh * M_PI / 180.0), D.cos_fn = std::cos(P.floor_normal_thresh * M_PI / 180.0);
    D.dist_thr = P.distance_threshold, D.log_prob = std::log(1.0 - P.probability), D.floor_tol = P.floor_tolerance;
    D.pts_thresh = P.floor_pts_thresh, D.max_iter = P.max_iterations, D.K = K, D.nf_mode = FLOOR_NF_OFF;
    FloorRecord* rec = f->rec.as<FloorRecord>();
    FloorState* st = f->state.as<FloorState>();
    int* bsum = f->bsum.as<int>();
    const int stride = (int)(stride_bytes / 4), ioff = intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1;
    float4 *clip = f->clip.as<float4>(), *filt = f->filt.as<float4>(), *coef = f->coef.as<float4>();
    unsigned char* bad = f->bad.as<unsigned char>();
    APD_HIP(hipMemsetAsync(f->rec.p, 0, sizeof(FloorRecord), f->stream));
    APD_HIP(hipMemcpyAsync(f->words.p, words, (size_t)K * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, f->stream));
    APD_HIP(hipMemsetAsync(f->n_in.p, 0, (size_t)FLOOR_MAX_K * sizeof(int), f->stream));
    APD_HIP(hipMemsetAsync(f->coef.p, 0, (size_t)FLOOR_MAX_K * sizeof(float4), f->stream));
    APD_HIP(hipMemsetAsync(f->bad.p, 0, (size_t)FLOOR_MAX_K, f->stream));
    // 1. tilt + height clip, in-order compaction (n_clipped -> the record)
    hipLaunchKernelGGL(k_floor_clip, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, d_in, ni, stride, ioff, D, f->tilted.as<float4>(), f->mask.as<unsigned char>(), bsum);
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, f->stream, bsum, nb, &rec->n_clipped);
    hipLaunchKernelGGL(k_floor_compact, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, f->tilted.as<float4>(), f->mask.as<unsigned char>(), ni, bsum, clip, f->clip_src.as<int>());
    APD_HIP(hipGetLastError());
    // 2. the normal filter: the exact k-NN of the registration over the clipped cloud, whose size the host has to know
    bool searched = false;
    if (P.use_normal_filtering) {
      APD_HIP(hipMemcpyAsync(f->h_rec.p, f->rec.p, sizeof(FloorRecord), hipMemcpyDeviceToHost, f->stream));
      APD_HIP(hipStreamSynchronize(f->stream));
      const int nc = f->record()->n_clipped;
      D.nf_mode = nc >= P.normal_k ? FLOOR_NF_STAT : FLOOR_NF_NONE;
      if (nc >= P.normal_k) {
        apdgicp_params ep;
        apdgicp_default_params(&ep);
        ep.k_correspondences = P.normal_k;
        if (!f->eng) {
          std::unique_ptr<Engine> e(new Engine);
          APD_TRY(e->init(&ep, f->device, f->stream));
          f->eng = e.release();
        } else {
          APD_TRY(f->eng->set_params(&ep));
        }
        Engine& E = *f->eng;
        if (!E.knn_pruned) return fail(APDGICP_ERR_UNSUPPORTED, "floor detection needs the pruned k-NN (APDGICP_KNN_MODE)");
        APD_TRY(E.set_cloud(0, (const float*)clip, nc, 16, 1, 0));
        APD_TRY(E.upload_desc());
        const int id0 = 0;
        APD_TRY(E.d_ids.upload(&id0, sizeof(int), f->stream));
        hipLaunchKernelGGL(k_knn_stat_coop<KNN_EPI_NORMALZ>, dim3((unsigned)((nc + 3) / 4), 1u), dim3(64), knn_coop_lds_bytes(4), f->stream, E.d_desc.as<CloudDesc>(),
                           E.d_ids.as<int>(), P.normal_k, E.d_errflag.as<int>(), E.d_stats.as<unsigned long long>(), f->stat.as<float>());
        APD_HIP(hipGetLastError());
        searched = true;
      }
    }
    hipLaunchKernelGGL(k_floor_nf_count, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, f->stat.as<float>(), D, rec, bsum + nb);
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, f->stream, bsum + nb, nb, &rec->n_filtered);
    hipLaunchKernelGGL(k_floor_nf_scatter, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, clip, f->clip_src.as<int>(), f->stat.as<float>(), D, rec, bsum + nb, filt, f->filt_src.as<int>());
    // 3. - 5. hypotheses, scores, the sequential loop over the scores, acceptance and the callback's memory
    hipLaunchKernelGGL(k_floor_hypotheses, dim3((K + 63) / 64), dim3(64), 0, f->stream, filt, f->words.as<unsigned>(), D, rec, coef, bad, f->samples.as<int>());
    hipLaunchKernelGGL(k_floor_score, dim3((ni + FLOOR_TILE - 1) / FLOOR_TILE, (K + FLOOR_GROUP - 1) / FLOOR_GROUP), dim3(FLOOR_TILE), 0, f->stream, filt, coef, bad, D, rec,
                       f->n_in.as<int>());
    hipLaunchKernelGGL(k_floor_replay, dim3(1), dim3(64), 0, f->stream, coef, bad, f->n_in.as<int>(), D, rec, st);
    // the inlier list and the under-floor clip
    hipLaunchKernelGGL(k_floor_emit_count, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, filt, d_in, ni, stride, D, rec, st, bsum + 2 * nb, bsum + 3 * nb);
    hipLaunchKernelGGL(k_floor_emit_scan, dim3(1), dim3(SCAN_BLK), 0, f->stream, bsum + 2 * nb, bsum + 3 * nb, nb, rec);
    hipLaunchKernelGGL(k_floor_emit_scatter, dim3(nb), dim3(FLOOR_BLK), 0, f->stream, filt, f->filt_src.as<int>(), d_in, ni, stride, ioff, D, rec, st, bsum + 2 * nb,
                       bsum + 3 * nb, f->in_xyzi.as<float4>(), f->in_src.as<int>(), f->in_row.as<int>(), f->under_xyzi.as<float4>(), f->under_src.as<int>());
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(f->h_rec.p, f->rec.p, sizeof(FloorRecord), hipMemcpyDeviceToHost, f->stream));
    if (searched) APD_HIP(hipMemcpyAsync(f->h_rec.as<char>() + sizeof(FloorRecord), f->eng->d_errflag.p, sizeof(int), hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));  // the wait for the result record
    const int flag = *(int*)(f->h_rec.as<char>() + sizeof(FloorRecord));
    if (flag) {
      APD_HIP(hipMemsetAsync(f->eng->d_errflag.p, 0, sizeof(int), f->stream));
      return fail(APDGICP_ERR_INTERNAL, "normal filter k-NN: " + Engine::errflag_text(flag));
    }
    FloorRecord* h = f->record();
    h->n_input = ni, h->K = K;
    memcpy(result, h, sizeof(*result));
    result->reserved[0] = 0;
    f->n_last = n, f->ran = true, f->stat_valid = searched;
    return 0;
  });
}

// which: 0 clipped, 1 filtered, 2 inliers, 3 under floor
static int floor_cloud(apdgicp_floor* f, int which, const float** xyzi, const int32_t** index, int64_t* n) {
  if (!f || which < 0 || which > 3) return fail(APDGICP_ERR_INVALID_ARG, "bad argument");
  const FloorRecord* h = f->record();
  const int64_t cnt = !f->ran ? 0 : which == 0 ? h->n_clipped : which == 1 ? h->n_filtered : which == 2 ? h->n_inlier_list : h->n_under_floor;
  DevBuf& pts = which == 0 ? f->clip : which == 1 ? f->filt : which == 2 ? f->in_xyzi : f->under_xyzi;
  DevBuf& idx = which == 0 ? f->clip_src : which == 1 ? f->filt_src : which == 2 ? f->in_src : f->under_src;
  if (xyzi) *xyzi = cnt ? pts.as<float>() : nullptr;
  if (index) *index = cnt ? idx.as<int32_t>() : nullptr;
  if (n) *n = cnt;
  return 0;
}
int apdgicp_floor_inliers(apdgicp_floor* f, const float** device_xyzi, const int32_t** device_index, int64_t* n) {
  return guarded([&]() -> int { return floor_cloud(f, 2, device_xyzi, device_index, n); });
}
int apdgicp_floor_under_floor_filtered(apdgicp_floor* f, const float** device_xyzi, const int32_t** device_index, int64_t* n) {
  return guarded([&]() -> int { return floor_cloud(f, 3, device_xyzi, device_index, n); });
}

int apdgicp_floor_copy(apdgicp_floor* f, int which, float* xyzi, int32_t* index, int64_t capacity) {
  return guarded([&]() -> int {
    int64_t n = 0;
    const float* p = nullptr;
    const int32_t* idx = nullptr;
    APD_TRY(floor_cloud(f, which, &p, &idx, &n));
    if (capacity < n) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the cloud");
    if (!n) return 0;
    APD_HIP(hipSetDevice(f->device));
    if (xyzi) APD_HIP(hipMemcpyAsync(xyzi, p, (size_t)n * 16, hipMemcpyDeviceToHost, f->stream));
    if (index) APD_HIP(hipMemcpyAsync(index, idx, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));
    return 0;
  });
}

int apdgicp_floor_hypotheses(apdgicp_floor* f, float* coeffs, uint8_t* bad, int32_t* n_in, int64_t capacity) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int K = f->ran ? f->K_last : 0;
    if ((coeffs || bad || n_in) && capacity < K) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer entries than hypotheses");
    if (!K) return 0;
    APD_HIP(hipSetDevice(f->device));
    if (coeffs) APD_HIP(hipMemcpyAsync(coeffs, f->coef.p, (size_t)K * 16, hipMemcpyDeviceToHost, f->stream));
    if (bad) APD_HIP(hipMemcpyAsync(bad, f->bad.p, (size_t)K, hipMemcpyDeviceToHost, f->stream));
    if (n_in) APD_HIP(hipMemcpyAsync(n_in, f->n_in.p, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));
    return 0;
  });
}

int apdgicp_floor_debug(apdgicp_floor* f, uint8_t* clip_mask, int64_t mask_capacity, float* normal_stat, int64_t stat_capacity, int32_t* samples, int64_t samples_capacity) {
  return guarded([&]() -> int {
    if (!f) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (!f->ran) return 0;
    const FloorRecord* h = f->record();
    const bool ransac = h->n_filtered >= f->prm.floor_pts_thresh && h->n_filtered >= 3;
    if ((clip_mask && mask_capacity < f->n_last) || (normal_stat && f->stat_valid && stat_capacity < h->n_clipped) || (samples && ransac && samples_capacity < (int64_t)f->K_last * 3))
      return fail(APDGICP_ERR_INVALID_ARG, "a destination holds fewer entries than the last run produced");
    APD_HIP(hipSetDevice(f->device));
    if (clip_mask) APD_HIP(hipMemcpyAsync(clip_mask, f->mask.p, (size_t)f->n_last, hipMemcpyDeviceToHost, f->stream));
    if (normal_stat && f->stat_valid) APD_HIP(hipMemcpyAsync(normal_stat, f->stat.p, (size_t)h->n_clipped * 4, hipMemcpyDeviceToHost, f->stream));
    if (samples && ransac) APD_HIP(hipMemcpyAsync(samples, f->samples.p, (size_t)f->K_last * 3 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    APD_HIP(hipStreamSynchronize(f->stream));
    return 0;
  });
}

// ------------------------------------------------------------------ map cloud generation (apd_map.hpp)
static_assert(sizeof(MapState) == 96 && sizeof(apdgicp_map_cloud_stats) == 112, "map cloud record layouts");

int apdgicp_map_cloud_create(int device, void* stream, apdgicp_map_cloud** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_map_cloud> m(new apdgicp_map_cloud);
    m->device = device;
    m->forget();
    if (stream) {
      m->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
      m->own_stream = true;
    }
    APD_TRY(m->h_state.ensure(sizeof(MapState)));
    APD_TRY(m->state.ensure(sizeof(MapState)));
    for (hipEvent_t& e : m->ev) APD_HIP(hipEventCreate(&e));
    *out = m.release();
    return 0;
  });
}

int apdgicp_map_cloud_destroy(apdgicp_map_cloud* m) {
  return guarded([&]() -> int {
    if (m) (void)hipSetDevice(m->device);
    delete m;
    return 0;
  });
}

int apdgicp_map_cloud_add_keyframe(apdgicp_map_cloud* m, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device, int32_t* id) {
  return guarded([&]() -> int {
    if (!m || !id || (n > 0 && !xyz)) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative point count");
    if (n > 2147483647ll) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^31 - 1 points");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    if (m->kfs.size() >= 2147483647u) return fail(APDGICP_ERR_UNSUPPORTED, "too many keyframes");
    APD_HIP(hipSetDevice(m->device));
    apdgicp_map_cloud::Keyframe kf;
    kf.n = n;
    if (n > 0) {
      APD_TRY(kf.pts.ensure((size_t)n * 16));
      const int rc = [&]() -> int {
        const float* src = xyz;
        if (!on_device) {
          APD_HIP(hipStreamSynchronize(m->stream));  // the staging buffer may still be read by the previous call
          APD_TRY(m->stage.ensure((size_t)n * stride_bytes));
          // the last point may be shorter than the stride in the caller's buffer: copy up to its last used float only
          const size_t used = std::max<int64_t>(12, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 12);
          APD_HIP(hipMemcpyAsync(m->stage.p, xyz, (size_t)(n - 1) * stride_bytes + used, hipMemcpyHostToDevice, m->stream));
          src = m->stage.as<float>();
        }
        hipLaunchKernelGGL(k_map_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, src, (long long)n, (int)(stride_bytes / 4),
                           intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1, kf.pts.as<float4>());
        APD_HIP(hipGetLastError());
        APD_HIP(hipStreamSynchronize(m->stream));  // the caller's memory is free again when the call returns
        return 0;
      }();
      if (rc < 0) return rc;
    }
    m->kfs.push_back(std::move(kf));
    *id = (int32_t)(m->kfs.size() - 1);
    return 0;
  });
}

int apdgicp_map_cloud_clear(apdgicp_map_cloud* m) {
  return guarded([&]() -> int {
    if (!m) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(m->device));
    APD_HIP(hipStreamSynchronize(m->stream));
    m->kfs.clear();  // (frees every keyframe's points)
    m->forget();
    return 0;
  });
}

int apdgicp_map_cloud_generate(apdgicp_map_cloud* m, int32_t n_keyframes, const int32_t* ids, const double* poses, double resolution, int32_t flags, int64_t* n_out) {
  return guarded([&]() -> int {
    if (!m || !n_out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    m->forget();
    if (n_keyframes < 1) return fail(APDGICP_ERR_INVALID_ARG, "no keyframes (the reference returns nullptr)");
    if (!poses) return fail(APDGICP_ERR_INVALID_ARG, "poses is null");
    if (flags & ~APDGICP_FLAG_XF_LINEAR_CHAIN) return fail(APDGICP_ERR_INVALID_ARG, "unknown bit in flags");
    if (!(resolution <= 0.0) && !std::isfinite(resolution)) return fail(APDGICP_ERR_INVALID_ARG, "the resolution is NaN or infinite");
    std::vector<MapJob> jobs((size_t)n_keyframes);
    int64_t total = 0;
    for (int c = 0; c < n_keyframes; c++) {
      const int64_t id = ids ? ids[c] : c;
      if (id < 0 || id >= (int64_t)m->kfs.size()) return fail(APDGICP_ERR_INVALID_ARG, "unknown keyframe id " + std::to_string(id));
      MapJob& j = jobs[(size_t)c];
      memset(&j, 0, sizeof(j));
      j.pts = m->kfs[(size_t)id].pts.as<float4>(), j.in_off = total;
      for (int r = 0; r < 3; r++)
        for (int q = 0; q < 4; q++) j.P[4 * r + q] = (float)poses[(size_t)c * 16 + r + 4 * q];  // pose.matrix().cast<float>() (M:23)
      total += m->kfs[(size_t)id].n;
    }
    if (total > 2147483647ll) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^31 - 1 input points");
    m->info.n_input = total;
    if (total == 0) return 0;
    APD_HIP(hipSetDevice(m->device));
    MapState* st = m->state.as<MapState>();
    auto fetch_state = [&]() -> int {
      APD_HIP(hipGetLastError());
      APD_HIP(hipMemcpyAsync(m->h_state.p, st, sizeof(MapState), hipMemcpyDeviceToHost, m->stream));
      APD_HIP(hipStreamSynchronize(m->stream));
      return 0;
    };
    auto stage_times = [&](int last) {  // events 0 .. last were recorded and have completed
      for (int q = 0; q < last; q++) (void)hipEventElapsedTime(&m->info.stage_ms[q], m->ev[q], m->ev[q + 1]);
    };
    // ---- M1
    APD_TRY(m->jobs.upload(jobs.data(), jobs.size() * sizeof(MapJob), m->stream));
    const unsigned nb = (unsigned)((total + MAP_BLK - 1) / MAP_BLK);
    APD_TRY(m->bsum.ensure((size_t)nb * 4));
    APD_TRY(m->pushed.ensure((size_t)total * 16));
    const int linear = (flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0;
    APD_HIP(hipEventRecord(m->ev[0], m->stream));
    hipLaunchKernelGGL(k_map_reset, dim3(1), dim3(64), 0, m->stream, st);
    hipLaunchKernelGGL(k_map_gate_count, dim3(nb), dim3(MAP_BLK), 0, m->stream, m->jobs.as<MapJob>(), n_keyframes, (long long)total, m->bsum.as<int>());
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, m->stream, m->bsum.as<int>(), (int)nb, &st->n_pushed);
    hipLaunchKernelGGL(k_map_push, dim3(nb), dim3(MAP_BLK), 0, m->stream, m->jobs.as<MapJob>(), n_keyframes, (long long)total, linear, m->bsum.as<int>(),
                       m->pushed.as<float4>(), st);
    APD_HIP(hipEventRecord(m->ev[1], m->stream));
    APD_TRY(fetch_state());
    const MapState& h = *m->h_state.as<MapState>();
    const int n_pushed = h.n_pushed, n_fin = h.n_finite;
    m->info.n_pushed = n_pushed, m->info.n_finite = n_fin;
    if (resolution <= 0.0) {  // M2
      stage_times(1);
      m->result = n_pushed ? m->pushed.as<float>() : nullptr, m->n_last = n_pushed;
      m->info.n_out = *n_out = n_pushed;
      return 0;
    }
    if (n_fin == 0) {
      stage_times(1);
      return 0;
    }
    // ---- M3: rounds until none finds a violator; two are enqueued per look at the state (a round after the last one returns at once)
    const unsigned nfb = (unsigned)(((int64_t)n_pushed + MAP_FIND_TILE - 1) / MAP_FIND_TILE);
    APD_TRY(m->bmin.ensure((size_t)nfb * 4));
    for (;;) {
      for (int r = 0; r < 2; r++) {
        hipLaunchKernelGGL(k_map_find, dim3(nfb), dim3(MAP_BLK), 0, m->stream, m->pushed.as<float4>(), st, m->bmin.as<int>());
        hipLaunchKernelGGL(k_map_grow, dim3(1), dim3(MAP_BLK), 0, m->stream, m->pushed.as<float4>(), m->bmin.as<int>(), (int)nfb, resolution, st);
      }
      APD_TRY(fetch_state());
      if (h.err) return fail(APDGICP_ERR_UNSUPPORTED, "the octree would be deeper than 21 levels at this resolution (extent / resolution > 2^21)");
      if (!h.found) break;
    }
    APD_HIP(hipEventRecord(m->ev[2], m->stream));
    const int depth = h.depth;
    for (int a = 0; a < 3; a++) m->info.min[a] = h.mn[a], m->info.max[a] = h.mx[a];
    m->info.depth = depth, m->info.rounds = h.rounds;
    // ---- M4 + the sort
    const int n = n_fin;
    const unsigned npb = (unsigned)(((int64_t)n_pushed + MAP_BLK - 1) / MAP_BLK);
    APD_TRY(m->sort.ensure(n, false));  // (nothing is in flight: the state was just read)
    hipLaunchKernelGGL(k_map_keys, dim3(npb), dim3(MAP_BLK), 0, m->stream, m->pushed.as<float4>(), resolution, st, m->sort.keys_a.as<unsigned long long>());
    m->info.sort_passes = (3 * depth + 7) / 8;
    const unsigned long long* keys = enqueue_radix_sort(m->stream, m->sort, n, m->info.sort_passes, false).keys;
    APD_HIP(hipEventRecord(m->ev[3], m->stream));
    // ---- M5
    const unsigned nhb = (unsigned)((n + MAP_BLK - 1) / MAP_BLK);
    APD_TRY(m->bsum.ensure((size_t)nhb * 4));
    APD_TRY(m->out.ensure((size_t)n * 16));
    hipLaunchKernelGGL(k_map_heads, dim3(nhb), dim3(MAP_BLK), 0, m->stream, keys, n, m->bsum.as<int>());
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, m->stream, m->bsum.as<int>(), (int)nhb, &st->n_out);
    hipLaunchKernelGGL(k_map_centres, dim3(nhb), dim3(MAP_BLK), 0, m->stream, keys, n, m->bsum.as<int>(), resolution, st, m->out.as<float4>(), n);
    APD_HIP(hipEventRecord(m->ev[4], m->stream));
    APD_TRY(fetch_state());
    stage_times(4);
    if (h.n_keys != n || h.n_out < 1 || h.n_out > n) return fail(APDGICP_ERR_INTERNAL, "map cloud: inconsistent counts");
    m->result = m->out.as<float>(), m->n_last = h.n_out;
    m->info.n_out = *n_out = h.n_out;
    return 0;
  });
}

int apdgicp_map_cloud_points(apdgicp_map_cloud* m, const float** device_xyzi, int64_t* n) {
  if (!m || !device_xyzi || !n) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *device_xyzi = m->n_last ? m->result : nullptr;
  *n = m->n_last;
  return 0;
}

int apdgicp_map_cloud_copy(apdgicp_map_cloud* m, float* dst_xyzi, int64_t capacity_points, int dst_on_device) {
  return guarded([&]() -> int {
    if (!m || !dst_xyzi) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (capacity_points < m->n_last) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the generated cloud");
    if (!m->n_last) return 0;
    APD_HIP(hipSetDevice(m->device));
    APD_HIP(hipMemcpyAsync(dst_xyzi, m->result, (size_t)m->n_last * 16, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m->stream));
    APD_HIP(hipStreamSynchronize(m->stream));
    return 0;
  });
}

int apdgicp_map_cloud_info(apdgicp_map_cloud* m, apdgicp_map_cloud_stats* info) {
  if (!m || !info) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *info = m->info;
  return 0;
}

// ------------------------------------------------------------------ Scan Context place recognition (apd_scan_context.hpp)
static_assert(sizeof(ScRec) == 24 && sizeof(apdgicp_scan_context_match) == 24 && sizeof(apdgicp_scan_context_params) == 56, "scan context record layouts");
static_assert(offsetof(ScRec, distance) == offsetof(apdgicp_scan_context_match, distance) && offsetof(ScRec, ring_rank) == offsetof(apdgicp_scan_context_match, ring_rank),
              "ScRec is apdgicp_scan_context_match");

namespace {
constexpr int kScMaxDescriptors = 65536, kScFirstCapacity = 256;

int sc_check_params(const apdgicp_scan_context_params& p) {
  if (p.num_ring < 1 || p.num_ring > SC_MAX_DIM || p.num_sector < 1 || p.num_sector > SC_MAX_DIM) return fail(APDGICP_ERR_INVALID_ARG, "num_ring and num_sector must be 1 .. 64");
  if (!(p.max_radius > 0.0) || !std::isfinite(p.max_radius)) return fail(APDGICP_ERR_INVALID_ARG, "max_radius must be positive and finite");
  if (!std::isfinite(p.azimuth_max) || !std::isfinite(p.azimuth_min) || !(p.azimuth_max > p.azimuth_min)) return fail(APDGICP_ERR_INVALID_ARG, "azimuth_max must be above azimuth_min");
  if (p.num_exclude_recent < 0) return fail(APDGICP_ERR_INVALID_ARG, "num_exclude_recent is negative");
  if (!std::isfinite(p.search_ratio) || p.search_ratio < 0.0 || p.search_ratio > 2.0) return fail(APDGICP_ERR_INVALID_ARG, "search_ratio must be 0 .. 2");
  if (p.dist_thresh != p.dist_thresh) return fail(APDGICP_ERR_INVALID_ARG, "dist_thresh is NaN");
  return 0;
}

// room for one more descriptor: the capacity doubles (the old contents are copied on the stream), up to 65 536
int sc_reserve(apdgicp_scan_context* h) {
  if (h->size < h->cap) return 0;
  if (h->size >= kScMaxDescriptors) return fail(APDGICP_ERR_UNSUPPORTED, "the database is full (65536 descriptors)");
  const size_t R = (size_t)h->prm.num_ring, S = (size_t)h->prm.num_sector;
  const int ncap = h->cap ? 2 * h->cap : kScFirstCapacity;
  const size_t per[4] = {R * S * 4, R * 4, S * 8, S * 8};
  DevBuf* old[4] = {&h->desc, &h->ring_key, &h->sector_key, &h->col_norm};
  DevBuf fresh[4];
  for (int b = 0; b < 4; b++) APD_TRY(fresh[b].ensure(per[b] * ncap));
  hipError_t e = hipSuccess;
  for (int b = 0; b < 4 && e == hipSuccess; b++)
    if (h->size) e = hipMemcpyAsync(fresh[b].p, old[b]->p, per[b] * h->size, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(APDGICP_ERR_HIP, std::string("scan context: growing the database: ") + hipGetErrorString(e));
  for (int b = 0; b < 4; b++) *old[b] = std::move(fresh[b]);
  h->cap = ncap;
  return 0;
}

int sc_build(apdgicp_scan_context* h, const float* dev_pts, int64_t n, int stride, int ioff, const float* dev_ready) {
  const apdgicp_scan_context_params& p = h->prm;
  const ScGeom g{p.num_ring, p.num_sector, p.max_radius, p.azimuth_max, p.azimuth_min};
  const size_t lds = (size_t)(APD_ATAN_TAB_ROWS * APD_ATAN_TAB_STRIDE + p.num_ring * p.num_sector) * 4;
  hipLaunchKernelGGL(k_sc_build, dim3(1), dim3(SC_BLK), lds, h->stream, dev_pts, (long long)n, stride, ioff, dev_ready, g, h->slot(h->size));
  APD_HIP(hipGetLastError());
  APD_HIP(hipStreamSynchronize(h->stream));  // the caller's memory is free again when the call returns
  h->size++;
  return 0;
}
}  // namespace

int apdgicp_scan_context_default_params(apdgicp_scan_context_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  memset(p, 0, sizeof(*p));
  p->num_ring = 40, p->num_sector = 20, p->max_radius = 80.0;  // Scancontext.h: PC_NUM_RING, PC_NUM_SECTOR, PC_MAX_RADIUS
  p->azimuth_max = 56.5, p->azimuth_min = -56.5;               // SC:67-71 after loop_detector.cpp:89
  p->num_exclude_recent = 10, p->num_candidates = 3;           // NUM_EXCLUDE_RECENT, NUM_CANDIDATES_FROM_TREE
  p->search_ratio = 0.1, p->dist_thresh = 0.5;                 // SEARCH_RATIO, sc_dist_thresh
  return 0;
}

int apdgicp_scan_context_create(const apdgicp_scan_context_params* params, int device, void* stream, apdgicp_scan_context** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_scan_context_params p;
    apdgicp_scan_context_default_params(&p);
    if (params) p = *params;
    APD_TRY(sc_check_params(p));
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_scan_context> h(new apdgicp_scan_context);
    h->prm = p;
    h->device = device;
    if (stream) {
      h->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
      h->own_stream = true;
    }
    *out = h.release();
    return 0;
  });
}

int apdgicp_scan_context_destroy(apdgicp_scan_context* h) {
  return guarded([&]() -> int {
    if (h) (void)hipSetDevice(h->device);
    delete h;
    return 0;
  });
}

int apdgicp_scan_context_set_params(apdgicp_scan_context* h, const apdgicp_scan_context_params* params) {
  return guarded([&]() -> int {
    if (!h || !params) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(sc_check_params(*params));
    const apdgicp_scan_context_params& o = h->prm;
    const bool s1 = params->num_ring != o.num_ring || params->num_sector != o.num_sector || params->max_radius != o.max_radius ||
                    params->azimuth_max != o.azimuth_max || params->azimuth_min != o.azimuth_min;
    if (s1 && h->size) return fail(APDGICP_ERR_INVALID_ARG, "the descriptor's geometry (S1) can change only while the database is empty");
    if (s1) {  // the buffers are laid out by R and S
      APD_HIP(hipSetDevice(h->device));
      APD_HIP(hipStreamSynchronize(h->stream));
      for (DevBuf* b : {&h->desc, &h->ring_key, &h->sector_key, &h->col_norm}) b->release();
      h->cap = 0;
    }
    h->prm = *params;
    return 0;
  });
}

int apdgicp_scan_context_add(apdgicp_scan_context* h, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device, int32_t* id) {
  return guarded([&]() -> int {
    if (!h || !id || (n > 0 && !xyz)) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative point count");
    if (n > 2147483647ll) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^31 - 1 points");
    if (stride_bytes < 8 || stride_bytes % 4 || stride_bytes > (1ll << 20)) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 8");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    APD_HIP(hipSetDevice(h->device));
    APD_TRY(sc_reserve(h));
    const float* src = xyz;
    if (n > 0 && !on_device) {
      APD_TRY(h->stage.ensure((size_t)n * stride_bytes));  // (every earlier call has waited for its own work)
      const size_t used = std::max<int64_t>(8, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 8);  // of the last point
      APD_HIP(hipMemcpyAsync(h->stage.p, xyz, (size_t)(n - 1) * stride_bytes + used, hipMemcpyHostToDevice, h->stream));
      src = h->stage.as<float>();
    }
    APD_TRY(sc_build(h, src, n, (int)(stride_bytes / 4), intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1, nullptr));
    *id = h->size - 1;
    return 0;
  });
}

int apdgicp_scan_context_add_descriptor(apdgicp_scan_context* h, const float* ring_major_RxS, int32_t* id) {
  return guarded([&]() -> int {
    if (!h || !id || !ring_major_RxS) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(h->device));
    APD_TRY(sc_reserve(h));
    const size_t bytes = (size_t)h->prm.num_ring * h->prm.num_sector * 4;
    APD_TRY(h->stage.ensure(bytes));
    APD_HIP(hipMemcpyAsync(h->stage.p, ring_major_RxS, bytes, hipMemcpyHostToDevice, h->stream));
    APD_TRY(sc_build(h, nullptr, 0, 0, -1, h->stage.as<float>()));
    *id = h->size - 1;
    return 0;
  });
}

int apdgicp_scan_context_clear(apdgicp_scan_context* h) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipStreamSynchronize(h->stream));
    h->size = 0;
    return 0;
  });
}

int apdgicp_scan_context_size(apdgicp_scan_context* h, int32_t* n) {
  if (!h || !n) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  *n = h->size;
  return 0;
}

int apdgicp_scan_context_detect_batch(apdgicp_scan_context* h, int32_t n_queries, const int32_t* query_ids, const int32_t* cand_offsets, const int32_t* cand_ids,
                                      int32_t top_k, apdgicp_scan_context_match* matches, int32_t* n_matches, int32_t* loop_ids, float* yaws) {
  return guarded([&]() -> int {
    if (!h || !query_ids || !cand_offsets || !matches || !n_matches) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (n_queries < 1 || n_queries > 65535) return fail(APDGICP_ERR_INVALID_ARG, "n_queries must be 1 .. 65535");
    if (top_k < 1) return fail(APDGICP_ERR_INVALID_ARG, "top_k must be at least 1");
    const apdgicp_scan_context_params& p = h->prm;
    const int R = p.num_ring, S = p.num_sector;
    // ---- S3 on the host: the ids are host memory
    std::vector<ScQuery> qs((size_t)n_queries);
    std::vector<int> cand;
    h->seen.resize((size_t)h->size, 0u);
    int max_n = 0, max_keep = 0, max_out = 0;
    int64_t total_out = 0;
    for (int q = 0; q < n_queries; q++) {
      const int qid = query_ids[q];
      const int64_t c0 = cand_offsets[q], c1 = cand_offsets[q + 1];
      if (qid < 0 || qid >= h->size) return fail(APDGICP_ERR_INVALID_ARG, "unknown query id " + std::to_string(qid));
      if (c0 < 0 || c1 < c0 || (c1 > c0 && !cand_ids)) return fail(APDGICP_ERR_INVALID_ARG, "candidate offsets must ascend from 0");
      if (++h->epoch == 0) {  // the counter wrapped: every mark is stale
        std::fill(h->seen.begin(), h->seen.end(), 0u);
        h->epoch = 1;
      }
      ScQuery& Q = qs[(size_t)q];
      Q.qid = qid, Q.base = (int)cand.size(), Q.out_base = (int)total_out;
      for (int64_t c = c0; c < c1; c++) {
        const int id = cand_ids[c];
        if (id < 0 || id >= h->size) return fail(APDGICP_ERR_INVALID_ARG, "candidate id " + std::to_string(id) + " is not in the database");
        if (h->seen[(size_t)id] == h->epoch) return fail(APDGICP_ERR_INVALID_ARG, "candidate id " + std::to_string(id) + " is given twice");
        h->seen[(size_t)id] = h->epoch;
        if (qid >= p.num_exclude_recent && (int64_t)qid - id >= p.num_exclude_recent) cand.push_back(id);  // SC:284, :300-305
      }
      Q.n = (int)cand.size() - Q.base;
      Q.keep = (p.num_candidates <= 0 || p.num_candidates >= Q.n) ? Q.n : p.num_candidates;
      Q.m_out = std::min(top_k, Q.keep);
      total_out += Q.m_out;
      max_n = std::max(max_n, Q.n), max_keep = std::max(max_keep, Q.keep), max_out = std::max(max_out, Q.m_out);
      if (cand.size() > (size_t)(1 << 30)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^30 candidates in one call");
    }
    const size_t total = cand.size();
    if (total) {
      APD_HIP(hipSetDevice(h->device));
      APD_TRY(h->qtab.upload(qs.data(), qs.size() * sizeof(ScQuery), h->stream));
      APD_TRY(h->cand.upload(cand.data(), total * sizeof(int), h->stream));
      APD_TRY(h->hi1.ensure(total * 8));
      APD_TRY(h->lo1.ensure(total * 4));
      APD_TRY(h->inv1.ensure(total * 4));
      APD_TRY(h->rec.ensure(total * sizeof(ScRec)));
      APD_TRY(h->hi2.ensure(total * 8));
      APD_TRY(h->lo2.ensure(total * 4));
      APD_TRY(h->inv2.ensure(total * 4));
      APD_TRY(h->out.ensure((size_t)total_out * sizeof(ScRec)));
      if ((size_t)total_out * sizeof(ScRec) > h->h_out.cap) {
        APD_TRY(h->h_out.ensure((size_t)total_out * 2 * sizeof(ScRec)));
      }
      const ScQuery* dq = h->qtab.dev.as<ScQuery>();
      const int* dc = h->cand.dev.as<int>();
      const unsigned nq = (unsigned)n_queries;
      const int radius = (int)std::floor(0.5 * p.search_ratio * (double)S + 0.5);  // SC:134 (C's round for a non-negative argument)
      const int region = sc_region_doubles(R, S) * 8;
      const int W = std::max(1, std::min(SC_MAX_WAVES, 65536 / region - 1));
      hipLaunchKernelGGL(k_sc_ring, dim3((unsigned)((max_n + SC_BLK - 1) / SC_BLK), nq), dim3(SC_BLK), 0, h->stream, h->ring_key.as<float>(), R, dq, dc,
                         h->hi1.as<unsigned long long>(), h->lo1.as<unsigned>());
      hipLaunchKernelGGL(k_sc_rank, dim3((unsigned)((max_n + SC_BLK - 1) / SC_BLK), nq), dim3(SC_BLK), 0, h->stream, h->hi1.as<unsigned long long>(),
                         h->lo1.as<unsigned>(), dq, 0, h->inv1.as<int>());
      hipLaunchKernelGGL(k_sc_dist, dim3((unsigned)((max_keep + W - 1) / W), nq), dim3(64 * W), (size_t)(1 + W) * region, h->stream, h->db(), R, S, radius, dq, dc,
                         h->inv1.as<int>(), h->hi1.as<unsigned long long>(), h->rec.as<ScRec>(), h->hi2.as<unsigned long long>(), h->lo2.as<unsigned>());
      hipLaunchKernelGGL(k_sc_rank, dim3((unsigned)((max_keep + SC_BLK - 1) / SC_BLK), nq), dim3(SC_BLK), 0, h->stream, h->hi2.as<unsigned long long>(),
                         h->lo2.as<unsigned>(), dq, 1, h->inv2.as<int>());
      hipLaunchKernelGGL(k_sc_emit, dim3((unsigned)((max_out + SC_BLK - 1) / SC_BLK), nq), dim3(SC_BLK), 0, h->stream, dq, h->inv2.as<int>(), h->rec.as<ScRec>(),
                         h->out.as<ScRec>());
      APD_HIP(hipGetLastError());
      APD_HIP(hipMemcpyAsync(h->h_out.p, h->out.p, (size_t)total_out * sizeof(ScRec), hipMemcpyDeviceToHost, h->stream));
      APD_HIP(hipStreamSynchronize(h->stream));  // the call's one wait
    }
    for (int q = 0; q < n_queries; q++) {
      const ScQuery& Q = qs[(size_t)q];
      n_matches[q] = Q.m_out;
      if (Q.m_out) memcpy(matches + (size_t)q * top_k, h->h_out.as<ScRec>() + Q.out_base, (size_t)Q.m_out * sizeof(ScRec));
      int loop = -1;
      float yaw = 0.f;
      if (Q.m_out) {
        const ScRec& m = h->h_out.as<ScRec>()[Q.out_base];
        if (m.distance < p.dist_thresh) loop = m.id;  // SC:359-361
        yaw = (float)((double)(float)(m.shift * ((p.azimuth_max - p.azimuth_min) / (double)S)) * 3.14159265358979323846 / 180.0);  // SC:374, :18-21
      }
      if (loop_ids) loop_ids[q] = loop;
      if (yaws) yaws[q] = yaw;
    }
    return 0;
  });
}

int apdgicp_scan_context_detect(apdgicp_scan_context* h, int32_t query_id, const int32_t* candidate_ids, int32_t n_candidates, int32_t top_k,
                                apdgicp_scan_context_match* matches, int32_t* n_matches, int32_t* loop_id, float* yaw_rad) {
  if (n_candidates < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative candidate count");
  const int32_t off[2] = {0, n_candidates};
  return apdgicp_scan_context_detect_batch(h, 1, &query_id, off, candidate_ids, top_k, matches, n_matches, loop_id, yaw_rad);
}

int apdgicp_scan_context_descriptors(apdgicp_scan_context* h, int32_t first, int32_t count, float* desc, float* ring_keys, double* sector_keys, double* col_norms) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (first < 0 || count < 0 || (int64_t)first + count > h->size) return fail(APDGICP_ERR_INVALID_ARG, "descriptor range outside the database");
    if (!count) return 0;
    APD_HIP(hipSetDevice(h->device));
    const size_t R = (size_t)h->prm.num_ring, S = (size_t)h->prm.num_sector, c = (size_t)count;
    const ScDb s = h->slot(first);
    if (desc) APD_HIP(hipMemcpyAsync(desc, s.desc, c * R * S * 4, hipMemcpyDeviceToHost, h->stream));
    if (ring_keys) APD_HIP(hipMemcpyAsync(ring_keys, s.ring_key, c * R * 4, hipMemcpyDeviceToHost, h->stream));
    if (sector_keys) APD_HIP(hipMemcpyAsync(sector_keys, s.sector_key, c * S * 8, hipMemcpyDeviceToHost, h->stream));
    if (col_norms) APD_HIP(hipMemcpyAsync(col_norms, s.col_norm, c * S * 8, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

// ------------------------------------------------------------------ DBSCAN clustering (apd_dbscan.hpp)
static_assert(sizeof(apdgicp_dbscan_cluster) == 80 && sizeof(DbCluster) == sizeof(apdgicp_dbscan_cluster) && offsetof(DbCluster, seed) == offsetof(apdgicp_dbscan_cluster, seed),
              "DbCluster is the table row");
static_assert(sizeof(apdgicp_dbscan_params) == 24, "apdgicp_dbscan_params layout");

void apdgicp_dbscan_default_params(apdgicp_dbscan_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->eps = 0.0, p->min_pts = 1, p->min_cluster_size = 1, p->max_cluster_size = std::numeric_limits<int32_t>::max();  // DB:111-114
}

static int dbscan_check_params(const apdgicp_dbscan_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "params is null");
  if (!(p->eps >= 0.0) || !std::isfinite(p->eps)) return fail(APDGICP_ERR_INVALID_ARG, "eps must be finite and >= 0 (and > 0 to run)");
  if (p->min_pts < 1) return fail(APDGICP_ERR_INVALID_ARG, "min_pts must be >= 1");
  if (p->min_cluster_size < 1 || p->max_cluster_size < 1) return fail(APDGICP_ERR_INVALID_ARG, "min_cluster_size and max_cluster_size must be >= 1");
  return 0;
}

int apdgicp_dbscan_create(const apdgicp_dbscan_params* p, int device, void* stream, apdgicp_dbscan** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_dbscan_params dflt;
    apdgicp_dbscan_default_params(&dflt);
    if (!p) p = &dflt;
    APD_TRY(dbscan_check_params(p));
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_dbscan> h(new apdgicp_dbscan);
    h->device = device, h->prm = *p;
    if (stream) {
      h->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
      h->own_stream = true;
    }
    APD_TRY(h->h_scal.ensure(DB_WORDS * sizeof(int)));
    memset(h->h_scal.p, 0, DB_WORDS * sizeof(int));
    APD_TRY(h->scal.ensure(DB_WORDS * sizeof(int)));
    *out = h.release();
    return 0;
  });
}

int apdgicp_dbscan_destroy(apdgicp_dbscan* h) {
  return guarded([&]() -> int {
    if (h) (void)hipSetDevice(h->device);
    delete h;
    return 0;
  });
}

int apdgicp_dbscan_set_params(apdgicp_dbscan* h, const apdgicp_dbscan_params* p) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(dbscan_check_params(p));
    h->prm = *p;
    return 0;
  });
}

static int bits_for(int64_t n) {  // the smallest b with n <= 2^b
  int b = 0;
  while ((1ll << b) < n) b++;
  return b;
}

int apdgicp_dbscan_run(apdgicp_dbscan* h, const float* xyz, int64_t n, int64_t stride_bytes, const float* doppler, int64_t doppler_stride_bytes, int on_device,
                       int32_t* n_clusters) {
  return guarded([&]() -> int {
    if (!h || !n_clusters) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *n_clusters = 0;
    h->ran = false, h->n_last = h->K_last = h->M_last = 0, h->launches = 0;
    const apdgicp_dbscan_params& P = h->prm;
    if (!(P.eps > 0.0)) return fail(APDGICP_ERR_INVALID_ARG, "eps (setClusterTolerance) must be > 0");
    if (n < 0 || (n > 0 && !xyz)) return fail(APDGICP_ERR_INVALID_ARG, "bad cloud");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (doppler && (doppler_stride_bytes < 4 || doppler_stride_bytes % 4)) return fail(APDGICP_ERR_INVALID_ARG, "doppler stride must be a multiple of 4 bytes and >= 4");
    if (n > (1ll << 24)) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    if (n == 0) {
      h->ran = true;
      return 0;
    }
    APD_HIP(hipSetDevice(h->device));
    const int ni = (int)n, nb = (ni + DB_BLK - 1) / DB_BLK, nt = scan_tiles(ni);
    const float *d_xyz = xyz, *d_dop = doppler;
    if (!on_device) {
      // (no wait: the copies are ordered behind the previous run's kernels by the stream; a buffer that grows is freed by hipFree, which waits)
      APD_TRY(h->stage.ensure((size_t)n * stride_bytes));
      APD_HIP(hipMemcpyAsync(h->stage.p, xyz, (size_t)(n - 1) * stride_bytes + 12, hipMemcpyHostToDevice, h->stream));
      d_xyz = h->stage.as<float>();
      if (doppler) {
        APD_TRY(h->stage_dop.ensure((size_t)n * doppler_stride_bytes));
        APD_HIP(hipMemcpyAsync(h->stage_dop.p, doppler, (size_t)(n - 1) * doppler_stride_bytes + 4, hipMemcpyHostToDevice, h->stream));
        d_dop = h->stage_dop.as<float>();
      }
    }
    APD_TRY(h->sort.ensure(ni, true));
    APD_TRY(h->pts.ensure((size_t)n * 16));
    APD_TRY(h->spts.ensure((size_t)n * 16));
    APD_TRY(h->gkeys.ensure((size_t)n * 8));
    for (DevBuf* b : {&h->dop, &h->cnt, &h->parent, &h->root, &h->seed, &h->nextra, &h->size, &h->ncore, &h->rank_of, &h->cseed, &h->csize, &h->mcount, &h->labels})
      APD_TRY(b->ensure((size_t)n * 4));
    APD_TRY(h->core.ensure((size_t)n));
    APD_TRY(h->score.ensure((size_t)n));
    APD_TRY(h->tsum.ensure((size_t)nt * 4));
    APD_TRY(h->msum.ensure((size_t)nt * 4));
    int* scal = h->scal.as<int>();
    const double eps2 = P.eps * P.eps, cell = P.eps * (1.0 + 0x1p-20);
    const int bits = bits_for(n), p1 = std::max(1, (2 * bits + 1 + 7) / 8);
    const dim3 grid(nb), blk(DB_BLK);
    hipStream_t st = h->stream;
    APD_HIP(hipMemsetAsync(scal, 0, DB_WORDS * sizeof(int), st));
    auto mark = [&](int k) { return h->profiling ? hipEventRecord(h->ev[k], st) : hipSuccess; };
    APD_HIP(mark(0));
    // the grid: cells, (cell, index) sorted, the sorted copy
    hipLaunchKernelGGL(k_db_keys, grid, blk, 0, st, d_xyz, ni, (int)(stride_bytes / 4), d_dop, (int)(doppler_stride_bytes / 4), cell, h->pts.as<float4>(), h->dop.as<float>(),
                       h->sort.keys_a.as<unsigned long long>(), h->sort.val_a.as<int>(), scal);
    auto sort_pairs = [&](int count, int passes) {  // what k_db_keys / k_db_rank_keys / k_db_member_emit left in keys_a / val_a
      const RadixSorted r = enqueue_radix_sort(st, h->sort, count, passes, true);
      h->launches += r.launches;
      return r;
    };
    RadixSorted r = sort_pairs(ni, 8);
    const unsigned long long* gk = h->gkeys.as<unsigned long long>();
    const float4* sp = h->spts.as<float4>();
    const unsigned char* sc = h->score.as<unsigned char>();
    hipLaunchKernelGGL(k_db_gather, grid, blk, 0, st, r.keys, r.vals, h->pts.as<float4>(), ni, h->gkeys.as<unsigned long long>(), h->spts.as<float4>());
    APD_HIP(mark(1));
    // D1 - D5
    hipLaunchKernelGGL(k_db_count, grid, blk, 0, st, gk, sp, ni, eps2, P.min_pts, h->cnt.as<int>(), h->core.as<unsigned char>(), h->score.as<unsigned char>(), h->parent.as<int>(),
                       h->size.as<int>(), h->ncore.as<int>());
    APD_HIP(mark(2));
    hipLaunchKernelGGL(k_db_union, grid, blk, 0, st, gk, sp, sc, ni, eps2, h->parent.as<int>());
    hipLaunchKernelGGL(k_db_flatten, grid, blk, 0, st, h->parent.as<int>(), h->core.as<unsigned char>(), ni, h->root.as<int>());
    APD_HIP(mark(3));
    hipLaunchKernelGGL(k_db_border, grid, blk, 0, st, gk, sp, sc, h->root.as<int>(), ni, eps2, h->seed.as<int>(), h->nextra.as<int>(), h->size.as<int>(), h->ncore.as<int>());
    APD_HIP(mark(4));
    // D6 / D7: kept seeds ranked by (size descending, seed ascending), the sizes scanned
    hipLaunchKernelGGL(k_db_rank_keys, grid, blk, 0, st, h->core.as<unsigned char>(), h->root.as<int>(), h->size.as<int>(), ni, bits, P.min_cluster_size, P.max_cluster_size,
                       h->sort.keys_a.as<unsigned long long>(), h->sort.val_a.as<int>(), h->rank_of.as<int>(), scal);
    r = sort_pairs(ni, p1);
    hipLaunchKernelGGL(k_db_rank_table, grid, blk, 0, st, r.keys, h->size.as<int>(), ni, bits, scal, h->rank_of.as<int>(), h->cseed.as<int>(), h->csize.as<int>());
    enqueue_exclusive_scan(st, h->csize.as<int>(), ni, h->tsum.as<int>(), scal + DB_W_M);
    h->launches += 10;
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(h->h_scal.p, h->scal.p, DB_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    APD_HIP(hipStreamSynchronize(st));  // the one wait of the call
    if (h->h_scal.as<int>()[DB_W_BAD] != 0)
      return fail(APDGICP_ERR_UNSUPPORTED, "DBSCAN: point " + std::to_string(DB_BAD_BASE - h->h_scal.as<int>()[DB_W_BAD]) + " lies 2^20 cells or more from the origin (cell side " +
                                               std::to_string(cell) + ")");
    const int K = h->h_scal.as<int>()[DB_W_K];
    const int64_t M = h->h_scal.as<int>()[DB_W_M];
    if (K < 0 || K > ni || M < K || M > (1ll << 30)) return fail(APDGICP_ERR_INTERNAL, "DBSCAN: inconsistent cluster count");
    if (K > 0) {
      const int Mi = (int)M, p2 = std::max(1, (bits_for(K) + 7) / 8);
      APD_TRY(h->sort.ensure(std::max(ni, Mi), true));  // (nothing is in flight)
      APD_TRY(h->offsets.ensure((size_t)(K + 1) * 4));
      APD_TRY(h->members.ensure((size_t)M * 4));
      APD_TRY(h->table.ensure((size_t)K * sizeof(DbCluster)));
      hipLaunchKernelGGL(k_db_offsets, dim3((K + 1 + DB_BLK - 1) / DB_BLK), blk, 0, st, h->csize.as<int>(), h->tsum.as<int>(), K, Mi, h->offsets.as<int>());
      hipLaunchKernelGGL(k_db_member_count, grid, blk, 0, st, gk, sp, sc, h->root.as<int>(), h->seed.as<int>(), h->nextra.as<int>(), h->rank_of.as<int>(), ni, eps2,
                         h->mcount.as<int>());
      enqueue_exclusive_scan(st, h->mcount.as<int>(), ni, h->msum.as<int>(), scal + DB_W_M2);
      hipLaunchKernelGGL(k_db_member_emit, grid, blk, 0, st, gk, sp, sc, h->root.as<int>(), h->seed.as<int>(), h->nextra.as<int>(), h->rank_of.as<int>(), h->mcount.as<int>(),
                         h->msum.as<int>(), ni, eps2, Mi, h->sort.keys_a.as<unsigned long long>(), h->sort.val_a.as<int>());
      r = sort_pairs(Mi, p2);
      APD_HIP(hipMemcpyAsync(h->members.p, r.vals, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_db_table, dim3(K), blk, 0, st, h->offsets.as<int>(), h->members.as<int>(), h->cseed.as<int>(), h->ncore.as<int>(), h->pts.as<float4>(),
                         d_dop ? h->dop.as<float>() : (const float*)nullptr, ni, h->table.as<DbCluster>());
      h->launches += 6;
    }
    hipLaunchKernelGGL(k_db_labels, grid, blk, 0, st, h->seed.as<int>(), h->rank_of.as<int>(), ni, h->labels.as<int>());
    h->launches += 1;
    APD_HIP(hipGetLastError());
    if (h->profiling) {
      APD_HIP(mark(5));
      APD_HIP(hipEventSynchronize(h->ev[5]));
      for (int k = 0; k < 5; k++) {
        float ms = 0.f;
        APD_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->phase_ms[k] = (double)ms;
      }
    }
    h->n_last = n, h->K_last = K, h->M_last = K > 0 ? M : 0, h->ran = true;
    *n_clusters = K;
    return 0;
  });
}

int apdgicp_dbscan_labels(apdgicp_dbscan* h, const int32_t** device_labels, int64_t* n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t cnt = h->ran ? h->n_last : 0;
    if (device_labels) *device_labels = cnt ? h->labels.as<int32_t>() : nullptr;
    if (n) *n = cnt;
    return 0;
  });
}

int apdgicp_dbscan_copy_labels(apdgicp_dbscan* h, int32_t* labels, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t n = h->ran ? h->n_last : 0;
    if (capacity < n || (n && !labels)) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer entries than the cloud has points");
    if (!n) return 0;
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipMemcpyAsync(labels, h->labels.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_dbscan_clusters(apdgicp_dbscan* h, apdgicp_dbscan_cluster* table, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t K = h->ran ? h->K_last : 0;
    if (capacity < K || (K && !table)) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer rows than there are clusters");
    if (!K) return 0;
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipMemcpyAsync(table, h->table.p, (size_t)K * sizeof(DbCluster), hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_dbscan_members(apdgicp_dbscan* h, int32_t* offsets, int64_t offsets_capacity, int32_t* indices, int64_t indices_capacity, int64_t* n_indices) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t K = h->ran ? h->K_last : 0, M = h->ran ? h->M_last : 0;
    if ((offsets && offsets_capacity < K + 1) || (indices && indices_capacity < M)) return fail(APDGICP_ERR_INVALID_ARG, "a destination holds fewer entries than the member lists");
    if (n_indices) *n_indices = M;
    if (!K) {
      if (offsets) offsets[0] = 0;
      return 0;
    }
    APD_HIP(hipSetDevice(h->device));
    if (offsets) APD_HIP(hipMemcpyAsync(offsets, h->offsets.p, (size_t)(K + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    if (indices) APD_HIP(hipMemcpyAsync(indices, h->members.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_dbscan_debug(apdgicp_dbscan* h, int32_t* cnt, uint8_t* core, int32_t* root, int32_t* primary, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    const int64_t n = h->ran ? h->n_last : 0;
    if ((cnt || core || root || primary) && capacity < n) return fail(APDGICP_ERR_INVALID_ARG, "a destination holds fewer entries than the cloud has points");
    if (!n) return 0;
    APD_HIP(hipSetDevice(h->device));
    if (cnt) APD_HIP(hipMemcpyAsync(cnt, h->cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (core) APD_HIP(hipMemcpyAsync(core, h->core.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (root) APD_HIP(hipMemcpyAsync(root, h->root.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (primary) APD_HIP(hipMemcpyAsync(primary, h->seed.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_dbscan_set_profiling(apdgicp_dbscan* h, int enable) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(h->device));
    for (hipEvent_t& e : h->ev)
      if (enable && !e) APD_HIP(hipEventCreate(&e));
    h->profiling = enable != 0;
    return 0;
  });
}

int apdgicp_dbscan_stats(apdgicp_dbscan* h, int64_t* launches, int64_t* waits, double phase_ms[5]) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  if (launches) *launches = h->launches;
  if (waits) *waits = h->launches ? (h->profiling ? 2 : 1) : 0;
  for (int k = 0; k < 5 && phase_ms; k++) phase_ms[k] = h->profiling ? h->phase_ms[k] : 0.0;
  return 0;
}

// ------------------------------------------------------------------ scan ingest and deskew (apd_ingest.hpp)
static_assert(sizeof(apdgicp_scan_ingest_params) == 16, "apdgicp_scan_ingest_params layout");

void apdgicp_scan_ingest_default_params(apdgicp_scan_ingest_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->power_threshold = 0.f, p->gate = 1;  // preprocessing_nodelet.cpp:107
}

static int ingest_check_params(const apdgicp_scan_ingest_params* p) {
  if (!p) return fail(APDGICP_ERR_INVALID_ARG, "params is null");
  if (p->gate != 0 && p->gate != 1) return fail(APDGICP_ERR_INVALID_ARG, "gate must be 0 or 1");
  if (p->flags & ~APDGICP_FLAG_XF_LINEAR_CHAIN) return fail(APDGICP_ERR_INVALID_ARG, "flags: only APDGICP_FLAG_XF_LINEAR_CHAIN is read by this object");
  return 0;
}

int apdgicp_scan_ingest_create(const apdgicp_scan_ingest_params* p, int device, void* stream, apdgicp_scan_ingest** out) {
  return guarded([&]() -> int {
    if (!out) return fail(APDGICP_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    apdgicp_scan_ingest_params dflt;
    apdgicp_scan_ingest_default_params(&dflt);
    if (!p) p = &dflt;
    APD_TRY(ingest_check_params(p));
    int count = 0;
    APD_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(APDGICP_ERR_INVALID_ARG, "device index out of range");
    APD_HIP(hipSetDevice(device));
    std::unique_ptr<apdgicp_scan_ingest> h(new apdgicp_scan_ingest);
    h->device = device, h->prm = *p;
    if (stream) {
      h->stream = (hipStream_t)stream;
    } else {
      APD_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
      h->own_stream = true;
    }
    APD_TRY(h->h_scal.ensure(16));
    memset(h->h_scal.p, 0, 16);
    APD_TRY(h->scal.ensure(16));
    *out = h.release();
    return 0;
  });
}

int apdgicp_scan_ingest_destroy(apdgicp_scan_ingest* h) {
  return guarded([&]() -> int {
    if (h) (void)hipSetDevice(h->device);
    delete h;
    return 0;
  });
}

int apdgicp_scan_ingest_set_params(apdgicp_scan_ingest* h, const apdgicp_scan_ingest_params* p) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_TRY(ingest_check_params(p));
    h->prm = *p;
    return 0;
  });
}

static IngestXf ingest_xf(const float* colmajor16, int flags) {
  IngestXf X;
  memset(&X, 0, sizeof(X));
  X.linear = (flags & APDGICP_FLAG_XF_LINEAR_CHAIN) ? 1 : 0;
  if (colmajor16) {
    X.on = 1;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) X.m[4 * r + c] = colmajor16[r + 4 * c];
  }
  return X;
}

int apdgicp_scan_ingest_run(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t xyz_stride_bytes, const float* intensity, int64_t intensity_stride_bytes,
                            const float* doppler, int64_t doppler_stride_bytes, int on_device, const float* pre_transform, int64_t* n_out) {
  return guarded([&]() -> int {
    if (!h || !n_out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    h->n_rows = 0, h->launches = h->waits = 0;
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative number of points");
    if (n > 0 && (!xyz || !intensity || !doppler)) return fail(APDGICP_ERR_INVALID_ARG, "a lane of the message is null");
    if (xyz_stride_bytes < 12 || xyz_stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "xyz stride must be a multiple of 4 bytes and >= 12");
    if (intensity_stride_bytes < 4 || intensity_stride_bytes % 4 || doppler_stride_bytes < 4 || doppler_stride_bytes % 4)
      return fail(APDGICP_ERR_INVALID_ARG, "intensity / doppler stride must be a multiple of 4 bytes and >= 4");
    if (n > ING_MAX_N) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(h->device));
    const int ni = (int)n, nb = (ni + ING_BLK - 1) / ING_BLK;
    IngestLanes L;
    L.xyz = (const char*)xyz, L.intensity = (const char*)intensity, L.doppler = (const char*)doppler;
    L.xyz_stride = xyz_stride_bytes, L.intensity_stride = intensity_stride_bytes, L.doppler_stride = doppler_stride_bytes;
    if (!on_device) {
      // (no wait: the copies are ordered behind the previous run's kernels by the stream; a buffer that grows is freed by hipFree, which waits)
      const char* base[3] = {L.xyz, L.intensity, L.doppler};
      const int64_t stride[3] = {xyz_stride_bytes, intensity_stride_bytes, doppler_stride_bytes}, width[3] = {12, 4, 4};
      const char* lo = std::min(base[0], std::min(base[1], base[2]));
      const char* hi = std::max(base[0] + width[0], std::max(base[1] + width[1], base[2] + width[2]));
      if (n >= 2 && stride[0] == stride[1] && stride[1] == stride[2] && hi - lo <= stride[0]) {
        // one array of structures: the three lanes overlap from the second point on, so [lo, last byte) is the caller's; one copy
        const size_t bytes = (size_t)(n - 1) * stride[0] + (size_t)(hi - lo);
        APD_TRY(h->stage_xyz.ensure(bytes));
        APD_HIP(hipMemcpyAsync(h->stage_xyz.p, lo, bytes, hipMemcpyHostToDevice, h->stream));
        L.xyz = h->stage_xyz.as<char>() + (base[0] - lo), L.intensity = h->stage_xyz.as<char>() + (base[1] - lo), L.doppler = h->stage_xyz.as<char>() + (base[2] - lo);
      } else {
        DevBuf* st[3] = {&h->stage_xyz, &h->stage_int, &h->stage_dop};
        const char** lane[3] = {&L.xyz, &L.intensity, &L.doppler};
        for (int k = 0; k < 3; k++) {
          const size_t bytes = (size_t)(n - 1) * stride[k] + width[k];
          APD_TRY(st[k]->ensure(bytes));
          APD_HIP(hipMemcpyAsync(st[k]->p, base[k], bytes, hipMemcpyHostToDevice, h->stream));
          *lane[k] = st[k]->as<char>();
        }
      }
    }
    APD_TRY(h->rows.ensure((size_t)n * 32));
    APD_TRY(h->index.ensure((size_t)n * 4));
    APD_TRY(h->bsum.ensure((size_t)nb * sizeof(int)));
    const apdgicp_scan_ingest_params& P = h->prm;
    const IngestXf X = ingest_xf(pre_transform, P.flags);
    int* bsum = h->bsum.as<int>();
    hipLaunchKernelGGL(k_ing_count, dim3(nb), dim3(ING_BLK), 0, h->stream, L, ni, P.gate, P.power_threshold, bsum);
    hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(SCAN_BLK), 0, h->stream, bsum, nb, h->scal.as<int>());
    hipLaunchKernelGGL(k_ing_scatter, dim3(nb), dim3(ING_BLK), 0, h->stream, L, ni, P.gate, P.power_threshold, X, bsum, h->rows.as<float4>(), h->index.as<int>());
    APD_HIP(hipGetLastError());
    APD_HIP(hipMemcpyAsync(h->h_scal.p, h->scal.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));  // the one wait of the call
    h->launches = 3, h->waits = 1;
    h->n_rows = *h->h_scal.as<int>();
    *n_out = h->n_rows;
    return 0;
  });
}

// PI1 .. PI5
int apdgicp_scan_ingest_run_polar(apdgicp_scan_ingest* h, const float* range, int64_t range_stride_bytes, const float* azimuth, int64_t azimuth_stride_bytes,
                                  const float* elevation, int64_t elevation_stride_bytes, const float* snr, int64_t snr_stride_bytes, const float* velocity,
                                  int64_t velocity_stride_bytes, int64_t n, int on_device, int64_t* n_out) {
  return guarded([&]() -> int {
    if (!h || !n_out) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    const char* base[5] = {(const char*)range, (const char*)azimuth, (const char*)elevation, (const char*)snr, (const char*)velocity};
    const int64_t stride[5] = {range_stride_bytes, azimuth_stride_bytes, elevation_stride_bytes, snr_stride_bytes, velocity_stride_bytes};
    // (nothing of the object is touched before the arguments are good: the rows of the last good run stay readable, PI4)
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative number of targets");
    for (int k = 0; k < 5; k++) {
      if (n > 0 && !base[k]) return fail(APDGICP_ERR_INVALID_ARG, "a lane of the message is null");
      if (stride[k] < 4 || stride[k] % 4) return fail(APDGICP_ERR_INVALID_ARG, "a lane stride must be a multiple of 4 bytes and >= 4");
    }
    if (n > ING_MAX_N) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 targets");
    h->n_rows = 0, h->launches = h->waits = 0;
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(h->device));
    if (!on_device) {
      // (no wait, as in run)
      const char* lo = *std::min_element(base, base + 5);
      const char* hi = *std::max_element(base, base + 5) + 4;
      bool one = n >= 2 && hi - lo <= stride[0];
      for (int k = 1; k < 5; k++) one = one && stride[k] == stride[0];
      if (one) {
        // one array of structures (RadarTargetExtended[]: stride 76, the fields at 0 / 4 / 8 / 16 / 12): [lo, last byte) is the caller's; one copy
        const size_t bytes = (size_t)(n - 1) * stride[0] + (size_t)(hi - lo);
        APD_TRY(h->stage_polar[0].ensure(bytes));
        APD_HIP(hipMemcpyAsync(h->stage_polar[0].p, lo, bytes, hipMemcpyHostToDevice, h->stream));
        for (int k = 0; k < 5; k++) base[k] = h->stage_polar[0].as<char>() + (base[k] - lo);
      } else {
        for (int k = 0; k < 5; k++) {
          const size_t bytes = (size_t)(n - 1) * stride[k] + 4;
          DevBuf& st = h->stage_polar[k];
          APD_TRY(st.ensure(bytes));
          APD_HIP(hipMemcpyAsync(st.p, base[k], bytes, hipMemcpyHostToDevice, h->stream));
          base[k] = st.as<char>();
        }
      }
    }
    APD_TRY(h->rows.ensure((size_t)n * 32));
    APD_TRY(h->index.ensure((size_t)n * 4));
    const PolarLanes L{base[0], base[1], base[2], base[3], base[4], stride[0], stride[1], stride[2], stride[3], stride[4]};
    const int ni = (int)n;
    hipLaunchKernelGGL(k_ing_polar, dim3((ni + ING_BLK - 1) / ING_BLK), dim3(ING_BLK), 0, h->stream, L, ni, h->rows.as<float4>(), h->index.as<int>());
    APD_HIP(hipGetLastError());
    h->launches = 1, h->waits = 0;
    h->n_rows = n;  // PI2: no gate, nothing to wait for
    *n_out = n;
    return 0;
  });
}

int apdgicp_scan_ingest_points(apdgicp_scan_ingest* h, const float** device_rows, const int32_t** device_index, int64_t* n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (device_rows) *device_rows = h->n_rows ? h->rows.as<float>() : nullptr;
    if (device_index) *device_index = h->n_rows ? h->index.as<int32_t>() : nullptr;
    if (n) *n = h->n_rows;
    return 0;
  });
}

int apdgicp_scan_ingest_copy(apdgicp_scan_ingest* h, float* rows, int32_t* index, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (capacity < h->n_rows) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer rows than the last run produced");
    if (!h->n_rows || (!rows && !index)) return 0;
    APD_HIP(hipSetDevice(h->device));
    if (rows) APD_HIP(hipMemcpyAsync(rows, h->rows.p, (size_t)h->n_rows * 32, hipMemcpyDeviceToHost, h->stream));
    if (index) APD_HIP(hipMemcpyAsync(index, h->index.p, (size_t)h->n_rows * 4, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_scan_ingest_deskew(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, int on_device,
                               const double* ang_vel, double scan_period, const float* T) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    h->n_desk = 0, h->launches = h->waits = 0;
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative number of points");
    if (n > 0 && !xyz) return fail(APDGICP_ERR_INVALID_ARG, "the cloud is null");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (intensity_offset_bytes >= 0 && (intensity_offset_bytes % 4 || intensity_offset_bytes + 4 > stride_bytes))
      return fail(APDGICP_ERR_INVALID_ARG, "intensity offset outside the point");
    if (n > ING_MAX_N) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    if (n == 0) return 0;
    APD_HIP(hipSetDevice(h->device));
    const char* d_in = (const char*)xyz;
    if (!on_device) {
      // (no wait, as in run)
      const size_t used = (size_t)std::max<int64_t>(12, intensity_offset_bytes >= 0 ? intensity_offset_bytes + 4 : 12);
      const size_t bytes = (size_t)(n - 1) * stride_bytes + used;
      APD_TRY(h->stage_cloud.ensure(bytes));
      APD_HIP(hipMemcpyAsync(h->stage_cloud.p, xyz, bytes, hipMemcpyHostToDevice, h->stream));
      d_in = h->stage_cloud.as<char>();
    }
    APD_TRY(h->desk.ensure((size_t)n * 16));
    DeskewParams D;
    memset(&D, 0, sizeof(D));
    D.scan_period = scan_period;
    if (ang_vel) {
      D.on = 1;
      for (int k = 0; k < 3; k++) D.a[k] = -(float)ang_vel[k];  // ang_v *= -1 (:951-952)
    }
    const IngestXf X = ingest_xf(T, h->prm.flags);
    hipLaunchKernelGGL(k_ing_deskew, dim3((unsigned)((n + ING_DESKEW_BLK - 1) / ING_DESKEW_BLK)), dim3(ING_DESKEW_BLK), 0, h->stream, d_in, (int)n, (long long)stride_bytes,
                       intensity_offset_bytes >= 0 ? (int)(intensity_offset_bytes / 4) : -1, D, X, h->desk.as<float4>());
    APD_HIP(hipGetLastError());
    h->launches = 1, h->waits = 0;
    h->n_desk = n;
    return 0;
  });
}

int apdgicp_scan_ingest_deskewed(apdgicp_scan_ingest* h, const float** device_xyzi, int64_t* n) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (device_xyzi) *device_xyzi = h->n_desk ? h->desk.as<float>() : nullptr;
    if (n) *n = h->n_desk;
    return 0;
  });
}

int apdgicp_scan_ingest_deskewed_copy(apdgicp_scan_ingest* h, float* xyzi, int64_t capacity) {
  return guarded([&]() -> int {
    if (!h || (!xyzi && capacity > 0)) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (capacity < h->n_desk) return fail(APDGICP_ERR_INVALID_ARG, "destination holds fewer points than the deskewed cloud");
    if (!h->n_desk) return 0;
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipMemcpyAsync(xyzi, h->desk.p, (size_t)h->n_desk * 16, hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_scan_ingest_synchronize(apdgicp_scan_ingest* h) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

// H1 .. H4
static int ingest_hist_ensure(apdgicp_scan_ingest* h) {
  if (h->hist_live) return 0;
  APD_TRY(h->hist.ensure(ING_HIST_WORDS * sizeof(int)));
  APD_TRY(h->hist_sum.ensure(ING_HIST_WORDS * sizeof(long long)));
  APD_HIP(hipMemsetAsync(h->hist.p, 0, ING_HIST_WORDS * sizeof(int), h->stream));
  APD_HIP(hipMemsetAsync(h->hist_sum.p, 0, ING_HIST_WORDS * sizeof(long long), h->stream));  // (the reference's vector is never zeroed, H3)
  h->hist_live = true;
  return 0;
}

int apdgicp_scan_ingest_histogram_add(apdgicp_scan_ingest* h, const float* xyz, int64_t n, int64_t stride_bytes, int on_device) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (n < 0) return fail(APDGICP_ERR_INVALID_ARG, "negative number of points");
    if (n > 0 && !xyz) return fail(APDGICP_ERR_INVALID_ARG, "the cloud is null");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(APDGICP_ERR_INVALID_ARG, "stride must be a multiple of 4 bytes and >= 12");
    if (n > ING_MAX_N) return fail(APDGICP_ERR_UNSUPPORTED, "more than 2^24 points");
    h->launches = h->waits = 0;
    APD_HIP(hipSetDevice(h->device));
    APD_TRY(ingest_hist_ensure(h));
    const char* d_in = (const char*)xyz;
    if (n > 0 && !on_device) {
      // (no wait, as in run)
      const size_t bytes = (size_t)(n - 1) * stride_bytes + 12;
      APD_TRY(h->stage_hist.ensure(bytes));
      APD_HIP(hipMemcpyAsync(h->stage_hist.p, xyz, bytes, hipMemcpyHostToDevice, h->stream));
      d_in = h->stage_hist.as<char>();
    }
    const int ni = (int)n, nb = std::max(1, (ni + ING_BLK - 1) / ING_BLK);  // n = 0: one block that counts nothing and adds the frame of zeros
    hipLaunchKernelGGL(k_ing_hist_zero, dim3(1), dim3(128), 0, h->stream, h->hist.as<int>());
    hipLaunchKernelGGL(k_ing_hist, dim3(nb), dim3(ING_BLK), 0, h->stream, d_in, ni, (long long)stride_bytes, h->hist.as<int>(), h->hist_sum.as<long long>());
    APD_HIP(hipGetLastError());
    h->launches = 2, h->waits = 0;
    return 0;
  });
}

int apdgicp_scan_ingest_histogram_last(apdgicp_scan_ingest* h, int32_t counts[100]) {
  return guarded([&]() -> int {
    if (!h || !counts) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    memset(counts, 0, ING_HIST_BINS * sizeof(int32_t));
    if (!h->hist_live) return 0;
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipMemcpyAsync(counts, h->hist.p, ING_HIST_BINS * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    APD_HIP(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int apdgicp_scan_ingest_histogram_read(apdgicp_scan_ingest* h, int64_t sum[100], int64_t* frames) {
  return guarded([&]() -> int {
    if (!h || (!sum && !frames)) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    long long host[ING_HIST_WORDS];
    memset(host, 0, sizeof(host));
    if (h->hist_live) {
      APD_HIP(hipSetDevice(h->device));
      APD_HIP(hipMemcpyAsync(host, h->hist_sum.p, sizeof(host), hipMemcpyDeviceToHost, h->stream));
      APD_HIP(hipStreamSynchronize(h->stream));
    }
    for (int b = 0; b < ING_HIST_BINS && sum; b++) sum[b] = host[b];
    if (frames) *frames = host[ING_HIST_BINS];
    return 0;
  });
}

int apdgicp_scan_ingest_histogram_reset(apdgicp_scan_ingest* h) {
  return guarded([&]() -> int {
    if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
    if (!h->hist_live) return 0;
    APD_HIP(hipSetDevice(h->device));
    APD_HIP(hipMemsetAsync(h->hist.p, 0, ING_HIST_WORDS * sizeof(int), h->stream));
    APD_HIP(hipMemsetAsync(h->hist_sum.p, 0, ING_HIST_WORDS * sizeof(long long), h->stream));
    return 0;
  });
}

int apdgicp_scan_ingest_stats(apdgicp_scan_ingest* h, int64_t* launches, int64_t* waits) {
  if (!h) return fail(APDGICP_ERR_INVALID_ARG, "null argument");
  if (launches) *launches = h->launches;
  if (waits) *waits = h->waits;
  return 0;
}

}  // extern "C"
