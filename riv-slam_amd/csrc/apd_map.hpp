// Map cloud generation on the device: radar_graph_slam::MapCloudGenerator::generate
// (radar_graph_slam/src/radar_graph_slam/map_cloud_generator.cpp:13-53), which rebuilds the global map from all keyframes after every
// graph optimisation (radar_graph_slam_nodelet.cpp:793) and for the save-map service (:1246):
//   .cpp:22-31  every keyframe in order, every point in order: d = src_pt.getVector3fMap().norm() widened to double, skipped iff d > 50
//               (a NaN point is kept); dst = pose.cast<float>() * src_pt.getVector4fMap(); the intensity is copied; push_back;
//   .cpp:38-39  resolution <= 0: the pushed cloud itself;
//   .cpp:41-46  pcl::octree::OctreePointCloud(resolution): addPointsFromInputCloud, getOccupiedVoxelCenters.
// PCL is not part of the reference tree; the kernels follow PCL 1.10 as published:
//   octree/impl/octree_pointcloud.hpp  addPointsFromInputCloud (points in order, isFinite ones only), adoptBoundingBoxToPoint (the box
//        grows towards the violating point, one level per step; the FIRST point gets a box of one voxel around itself, then getKeyBitSize),
//        getKeyBitSize (depth = ceil(log2(max key) - eps), the box is centred in the cube of that depth), genOctreeKeyforPoint
//        (key = unsigned((p - min) / res)), genLeafNodeCenterFromOctreeKey ((key + 0.5) * res + min);
//   octree_base.hpp / octree_key.h     getOccupiedVoxelCentersRecursive, pushBranch: a depth-first walk, child index (x << 2) | (y << 1) | z.
// So the grid origin depends on the ORDER in which the points arrive, and the output order is that of the interleaved key.  The box
// replay is sequential by nature; here a round finds the lowest pushed index at or after a cursor whose finite point violates the
// current box (k_map_find: block minima; k_map_grow: one minimum), one lane applies PCL's loop for that point, and the cursor moves
// behind it: the points between two violators cannot change the box, so the result is that of the sequential loop.  Every growth step
// raises the depth, so there are at most MAP_MAX_DEPTH rounds after the first point's.
//
// Operation orders that belong to Eigen / PCL, all stated in include/apdgicp_hip.h:
//   - the norm is sqrtf((x x + y y) + z z), each fp32 operation rounded on its own (the scan filter's convention);
//   - pose * p per row: xf_row (apd_kernels.hpp), pairwise by default, the linear chain with APDGICP_FLAG_XF_LINEAR_CHAIN;
//   - box, keys and centres in fp64, one IEEE operation at a time; eps = FLT_EPSILON widened to double;
//   - depth = ceil(log2(m) - eps) is evaluated as the smallest d >= 1 with 2^d >= m: the same integer for every m <= 2^21, and a larger m
//     is past the depth limit anyway; PCL shifts an int by the depth and breaks near 31, here a depth above 21 is refused (the
//     interleaved key stays within 63 bits; at 0.05 m depth 21 is a cube of 104 km).
// The distinct keys come from a stable LSD radix sort of the interleaved u64 keys (8-bit digits over the 3 * depth significant bits:
// k_map_rs_hist / k_map_scan_tiles / k_scan_bsum / k_map_rs_scatter).  No floating-point atomics; integer counts use atomicAdd.  Every
// pointer of this file is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_ego.hpp"
#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int MAP_BLK = EGO_BLK;          // compaction kernels: 16 waves, one point per lane (ego_block_counts / ego_block_slot)
constexpr int MAP_FIND_ITEMS = 4;         // points per lane of k_map_find
constexpr int MAP_FIND_TILE = MAP_BLK * MAP_FIND_ITEMS;
constexpr int MAP_MAX_DEPTH = 21;
constexpr int MAP_RS_BLK = 256;           // radix sort: 4 waves ...
constexpr int MAP_RS_ITEMS = 16;          // ... each owning 16 rounds of 64 consecutive keys
constexpr int MAP_RS_TILE = MAP_RS_BLK * MAP_RS_ITEMS;
constexpr int MAP_NONE = 2147483647;
constexpr double MAP_EPS = 1.1920928955078125e-07;  // std::numeric_limits<float>::epsilon()

struct MapJob {  // one keyframe of a generate call
  const float4* pts;
  long long in_off;  // points of the jobs in front of it
  float P[12];       // rows 0..2 of (float)pose, row-major
};

struct MapState {  // the box replay's state and the counts the kernels hand each other and the host
  double mn[3], mx[3];
  int depth, rounds, err, found;
  int cursor, n_pushed, n_finite, n_keys;
  int n_out, pad_[3];
};

__global__ void k_map_pack(const float* pts, long long n, int stride /* floats */, int ioff /* < 0: none */, float4* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + i * stride;
  out[i] = make_float4(p[0], p[1], p[2], ioff >= 0 ? p[ioff] : 0.f);
}

__global__ void k_map_reset(MapState* st) {
  if (threadIdx.x || blockIdx.x) return;
  for (int a = 0; a < 3; a++) st->mn[a] = st->mx[a] = 0.0;
  st->depth = st->rounds = st->err = 0, st->found = 1;
  st->cursor = st->n_pushed = st->n_finite = st->n_keys = st->n_out = 0;
}

// ---- M1 (.cpp:22-31): one lane per input point of the ragged list of keyframes
__device__ __forceinline__ int map_job_of(const MapJob* jobs, int nj, long long i) {  // the last job with in_off <= i (an empty job shares its offset with its successor)
  int lo = 0, hi = nj;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (jobs[mid].in_off <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ bool map_gate(float4 p) {  // skipped iff d > 50: a NaN norm is kept
  const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z));
  return !((double)sqrtf(d2) > 50.0);
}
__global__ __launch_bounds__(MAP_BLK) void k_map_gate_count(const MapJob* jobs, int nj, long long n, int* bsum) {
  __shared__ int wsum[MAP_BLK / 64];
  const long long i = (long long)blockIdx.x * MAP_BLK + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const MapJob* j = jobs + map_job_of(jobs, nj, i);
    ok = map_gate(j->pts[i - j->in_off]);
  }
  ego_block_counts(ok, wsum, bsum);
}
// ... and their in-order compaction (bsum: scanned by k_scan_bsum, which also left n_pushed in the state); the finite ones are counted
__global__ __launch_bounds__(MAP_BLK) void k_map_push(const MapJob* jobs, int nj, long long n, int linear, const int* bsum, float4* pushed, MapState* st) {
  __shared__ int wsum[MAP_BLK / 64];
  const long long i = (long long)blockIdx.x * MAP_BLK + threadIdx.x;
  bool ok = false;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) {
    const MapJob* j = jobs + map_job_of(jobs, nj, i);
    const float4 p = j->pts[i - j->in_off];
    ok = map_gate(p);
    o = make_float4(xf_row(j->P + 0, p.x, p.y, p.z, linear), xf_row(j->P + 4, p.x, p.y, p.z, linear), xf_row(j->P + 8, p.x, p.y, p.z, linear), p.w);
  }
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (ok) pushed[slot] = o;
  const int c = __popcll(__ballot(ok && finite3(o)));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&st->n_finite, c);
}

// ---- M3 (adoptBoundingBoxToPoint over the pushed points in order).  A round = k_map_find + k_map_grow; both return at once when the
// previous round found nothing, so the host may enqueue more rounds than are needed between two looks at `found`.
__global__ __launch_bounds__(MAP_BLK) void k_map_find(const float4* pushed, const MapState* st, int* bmin) {
  __shared__ int wmin[MAP_BLK / 64];
  const int tid = threadIdx.x;
  const int n = st->n_pushed, cursor = st->cursor, depth = st->depth;
  const long long base = (long long)blockIdx.x * MAP_FIND_TILE;
  int cand = MAP_NONE;
  if (st->found && !st->err && base + MAP_FIND_TILE > cursor) {  // (block-uniform)
    const double m0 = st->mn[0], m1 = st->mn[1], m2 = st->mn[2], x0 = st->mx[0], x1 = st->mx[1], x2 = st->mx[2];
    for (int u = 0; u < MAP_FIND_ITEMS; u++) {
      const long long i = base + (long long)u * MAP_BLK + tid;
      if (i < cursor || i >= n) continue;
      const float4 p = pushed[i];
      if (!finite3(p)) continue;
      const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
      if (depth == 0 || x < m0 || y < m1 || z < m2 || x >= x0 || y >= x1 || z >= x2) cand = min(cand, (int)i);  // (depth 0: no box yet, the first finite point)
    }
  }
  for (int off = 32; off; off >>= 1) cand = min(cand, __shfl_xor(cand, off, 64));
  if ((tid & 63) == 0) wmin[tid >> 6] = cand;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < MAP_BLK / 64; w++) cand = min(cand, wmin[w]);
    bmin[blockIdx.x] = cand;
  }
}
// ONE block: the minimum of the block minima, then lane 0 runs PCL's code for that point
__global__ __launch_bounds__(MAP_BLK) void k_map_grow(const float4* pushed, const int* bmin, int nb, double res, MapState* st) {
  __shared__ int wmin[MAP_BLK / 64];
  const int tid = threadIdx.x;
  if (!st->found || st->err) return;  // (uniform; lane 0 writes only behind the barrier below)
  int cand = MAP_NONE;
  for (int b = tid; b < nb; b += MAP_BLK) cand = min(cand, bmin[b]);
  for (int off = 32; off; off >>= 1) cand = min(cand, __shfl_xor(cand, off, 64));
  if ((tid & 63) == 0) wmin[tid >> 6] = cand;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < MAP_BLK / 64; w++) cand = min(cand, wmin[w]);
  if (cand == MAP_NONE) {
    st->found = 0;
    return;
  }
  const float4 q = pushed[cand];
  const double p[3] = {(double)q.x, (double)q.y, (double)q.z};
  double mn[3], mx[3];
  int depth = st->depth;
  if (depth == 0) {  // the first point: a voxel around it (adoptBoundingBoxToPoint), then getKeyBitSize
    const double half = __ddiv_rn(res, 2.0);
    double m = 2.0;
    for (int a = 0; a < 3; a++) {
      mn[a] = __dsub_rn(p[a], half), mx[a] = __dadd_rn(p[a], half);
      m = fmax(m, ceil(__ddiv_rn(__dsub_rn(__dsub_rn(mx[a], mn[a]), MAP_EPS), res)));
    }
    depth = 1;
    while (depth <= MAP_MAX_DEPTH && (double)(1 << depth) < m) depth++;
    if (depth > MAP_MAX_DEPTH) {
      st->err = 1;
      return;
    }
    const double side = __dmul_rn((double)(1 << depth), res);
    for (int a = 0; a < 3; a++) {
      const double o = __ddiv_rn(__dsub_rn(side, __dsub_rn(mx[a], mn[a])), 2.0);
      if (o > MAP_EPS) mn[a] = __dsub_rn(mn[a], o), mx[a] = __dadd_rn(mx[a], o);
    }
  } else {
    for (int a = 0; a < 3; a++) mn[a] = st->mn[a], mx[a] = st->mx[a];
    for (;;) {
      bool up[3], any = false;
      for (int a = 0; a < 3; a++) up[a] = p[a] >= mx[a], any = any || up[a] || p[a] < mn[a];
      if (!any) break;
      if (depth + 1 > MAP_MAX_DEPTH) {
        st->err = 1;
        return;
      }
      const double side = __dmul_rn((double)(1 << depth), res);
      for (int a = 0; a < 3; a++)
        if (!up[a]) mn[a] = __dsub_rn(mn[a], side);
      depth++;
      const double len = __dsub_rn(__dmul_rn((double)(1 << depth), res), MAP_EPS);
      for (int a = 0; a < 3; a++) mx[a] = __dadd_rn(mn[a], len);
    }
    st->rounds++;
  }
  for (int a = 0; a < 3; a++) st->mn[a] = mn[a], st->mx[a] = mx[a];
  st->depth = depth, st->cursor = cand + 1;
}

// ---- M4 (genOctreeKeyforPoint) and the interleaved key: bit triple of level L, from the top, = (kx_L << 2) | (ky_L << 1) | kz_L
__device__ __forceinline__ unsigned long long map_spread3(unsigned v) {
  unsigned long long x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ unsigned map_compact3(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
  x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
  x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
  x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
  x = (x ^ (x >> 32)) & 0x1fffffull;
  return (unsigned)x;
}
// the keys of the finite points, packed (their order does not matter: they are sorted next); a block takes its slots with one atomicAdd
__global__ __launch_bounds__(MAP_BLK) void k_map_keys(const float4* pushed, double res, MapState* st, unsigned long long* keys) {
  __shared__ int wsum[MAP_BLK / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long i = (long long)blockIdx.x * MAP_BLK + tid;
  bool ok = false;
  unsigned long long key = 0;
  if (i < st->n_pushed) {
    const float4 p = pushed[i];
    if (finite3(p)) {
      ok = true;
      const unsigned kx = (unsigned)__ddiv_rn(__dsub_rn((double)p.x, st->mn[0]), res);
      const unsigned ky = (unsigned)__ddiv_rn(__dsub_rn((double)p.y, st->mn[1]), res);
      const unsigned kz = (unsigned)__ddiv_rn(__dsub_rn((double)p.z, st->mn[2]), res);
      key = map_spread3(kx) << 2 | map_spread3(ky) << 1 | map_spread3(kz);
    }
  }
  const unsigned long long m = __ballot(ok);
  if ((tid & 63) == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < MAP_BLK / 64; w++) total += wsum[w];
    s_base = total ? atomicAdd(&st->n_keys, total) : 0;
  }
  __syncthreads();
  int before = s_base;
  for (int w = 0; w < wave; w++) before += wsum[w];
  if (ok) keys[mbcnt_add(m, before)] = key;
}

// ---- the stable LSD radix sort, one 8-bit digit per pass.  A block owns MAP_RS_TILE consecutive keys.
// pass part 1: hist[digit * nblk + block] = keys of the block with that digit
__global__ __launch_bounds__(MAP_RS_BLK) void k_map_rs_hist(const unsigned long long* keys, int n, int shift, int nblk, int* hist) {
  __shared__ int h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * MAP_RS_TILE;
  for (int u = 0; u < MAP_RS_ITEMS; u++) {
    const long long i = base + u * MAP_RS_BLK + tid;
    if (i < n) atomicAdd(&h[(int)(keys[i] >> shift) & 255], 1);
  }
  __syncthreads();
  hist[(size_t)tid * nblk + blockIdx.x] = h[tid];
}
// pass part 2: exclusive scan of v[0..n) in tiles of SCAN_BLK * SCAN_ITEMS (in place) + the tile sums, which k_scan_bsum scans
__global__ __launch_bounds__(SCAN_BLK) void k_map_scan_tiles(int* v, int n, int* bsum) {
  __shared__ int lds[SCAN_BLK / 64];
  const int tid = threadIdx.x, i0 = (blockIdx.x * SCAN_BLK + tid) * SCAN_ITEMS;
  int f[SCAN_ITEMS], s = 0;
  for (int u = 0; u < SCAN_ITEMS; u++) f[u] = i0 + u < n ? v[i0 + u] : 0, s += f[u];
  int total;
  int ex = block_exclusive_scan(s, lds, tid, &total);
  for (int u = 0; u < SCAN_ITEMS; u++) {
    if (i0 + u < n) v[i0 + u] = ex;
    ex += f[u];
  }
  if (tid == 0) bsum[blockIdx.x] = total;
}
// pass part 3: wave w of a block owns keys [w * 1024, (w + 1) * 1024) of the tile and walks them in 16 rounds of 64 consecutive keys.  The
// rank of a key among the keys of its wave with the same digit: the wave's running count of that digit (LDS, one row per wave) + the
// lanes below it with the same digit in this round (eight ballots).  Then the digit's global base for this block (scanned histogram) and
// the counts of the waves in front give every key its place.  Equal digits keep their order: the pass is stable.
// WITH_VALUE: every key carries a 32-bit payload along (vin -> vout; the voxelized GICP map sorts (voxel key, point index) pairs with it).
template <bool WITH_VALUE>
__device__ __forceinline__ void map_rs_scatter(const unsigned long long* in, const int* vin, unsigned long long* out, int* vout, int n, int shift, int nblk, const int* hist,
                                               const int* bsum) {
  __shared__ int cnt[MAP_RS_BLK / 64][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int w = 0; w < MAP_RS_BLK / 64; w++) cnt[w][tid] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1;
  const long long base = (long long)blockIdx.x * MAP_RS_TILE + wave * (64 * MAP_RS_ITEMS);
  unsigned long long key[MAP_RS_ITEMS];
  int rank[MAP_RS_ITEMS];
#pragma unroll
  for (int u = 0; u < MAP_RS_ITEMS; u++) {
    const long long i = base + u * 64 + lane;
    const bool valid = i < n;
    key[u] = valid ? in[i] : 0ull;
    const int d = (int)(key[u] >> shift) & 255;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const unsigned long long mb = __ballot((d >> b) & 1);
      peers &= ((d >> b) & 1) ? mb : ~mb;
    }
    const int before = cnt[wave][d];
    rank[u] = before + __popcll(peers & below);
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers & below) == 0) cnt[wave][d] = before + __popcll(peers);  // the lowest lane of every digit group
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    const size_t e = (size_t)tid * nblk + blockIdx.x;
    int g = hist[e] + bsum[e / (SCAN_BLK * SCAN_ITEMS)];
    for (int w = 0; w < MAP_RS_BLK / 64; w++) {
      const int c = cnt[w][tid];
      cnt[w][tid] = g;
      g += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < MAP_RS_ITEMS; u++) {
    const long long i = base + u * 64 + lane;
    if (i < n) {
      const int pos = cnt[wave][(int)(key[u] >> shift) & 255] + rank[u];
      if (pos >= 0 && pos < n) {
        out[pos] = key[u];
        if constexpr (WITH_VALUE) vout[pos] = vin[i];
      }
    }
  }
}
__global__ __launch_bounds__(MAP_RS_BLK) void k_map_rs_scatter(const unsigned long long* in, unsigned long long* out, int n, int shift, int nblk, const int* hist,
                                                               const int* bsum) {
  map_rs_scatter<false>(in, nullptr, out, nullptr, n, shift, nblk, hist, bsum);
}
__global__ __launch_bounds__(MAP_RS_BLK) void k_map_rs_scatter_pairs(const unsigned long long* in, const int* vin, unsigned long long* out, int* vout, int n, int shift,
                                                                     int nblk, const int* hist, const int* bsum) {
  map_rs_scatter<true>(in, vin, out, vout, n, shift, nblk, hist, bsum);
}

// ---- M5: the first key of every run of equal keys is a voxel; count, scan (k_scan_bsum -> n_out), centres
__device__ __forceinline__ bool map_head(const unsigned long long* keys, long long i, int n) {
  return i < n && (i == 0 || keys[i - 1] != keys[i]);
}
__global__ __launch_bounds__(MAP_BLK) void k_map_heads(const unsigned long long* keys, int n, int* bsum) {
  __shared__ int wsum[MAP_BLK / 64];
  ego_block_counts(map_head(keys, (long long)blockIdx.x * MAP_BLK + threadIdx.x, n), wsum, bsum);
}
__global__ __launch_bounds__(MAP_BLK) void k_map_centres(const unsigned long long* keys, int n, const int* bsum, double res, const MapState* st, float4* out, int out_cap) {
  __shared__ int wsum[MAP_BLK / 64];
  const long long i = (long long)blockIdx.x * MAP_BLK + threadIdx.x;
  const bool ok = map_head(keys, i, n);
  const int slot = ego_block_slot(ok, wsum, bsum[blockIdx.x]);
  if (!ok || slot >= out_cap) return;
  const unsigned long long k = keys[i];
  const double kx = (double)map_compact3(k >> 2), ky = (double)map_compact3(k >> 1), kz = (double)map_compact3(k);
  out[slot] = make_float4((float)__dadd_rn(__dmul_rn(__dadd_rn(kx, 0.5), res), st->mn[0]), (float)__dadd_rn(__dmul_rn(__dadd_rn(ky, 0.5), res), st->mn[1]),
                          (float)__dadd_rn(__dmul_rn(__dadd_rn(kz, 0.5), res), st->mn[2]), 0.f);  // a default-constructed point: intensity 0
}

}  // namespace apd
