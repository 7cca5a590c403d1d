// Exact k-nearest and radius queries of a sorted cloud for arbitrary points (Q1 ... Q9 of include/apdgicp_hip.h).
//
//   k_knn_queries     Q2 / Q9: per query the k smallest keys, ascending; with a radius bound only keys whose distance is below r2
//   k_radius_count    Q5 with max_nn = 0: hits per query
//   k_radius_scan     per-block exclusive scan of the counts (k_scan_bsum of apd_voxel.hpp scans the block sums)
//   k_radius_fill     the hits of every query into its row, in visiting order
//   k_radius_sort_rows  every row into ascending key: one block per row, a bitonic network over the row in place
//
// The key is dist_key(sqdist1(t, q), original target index): unique per target point, so the set of the k smallest keys (or of the
// keys below r2) does not depend on the order the target is visited in, and neither do the bytes that leave.  The order only decides
// how early the bound tightens.  All three searching kernels share one walk (search_walk): one query per lane, queries in the curve
// order of their own sort, so that a wave's queries are neighbours; target groups from the group nearest the wave's query box
// outwards along the target's curve; a super box, a group or a chunk is skipped for the WAVE only when, for every lane, its fp32
// lower bound (lb_point_box: monotone in sqdist1's own rounding) is strictly above the lane's k-th distance or not below r2.  A lane
// whose list is not full has the bound +Inf and never prunes.  Every loop bound is a launch argument; no lane reads another lane's
// state, no block waits for another block, no atomics.
#pragma once
#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int SQ_BLK = 64;    // one wave per block, one query per lane
constexpr int SQ_KMAX = 64;   // keys a lane keeps: SQ_KMAX * SQ_BLK * 8 = 32 KB of static LDS
constexpr int SQ_SORT_BLK = 256;

struct SearchTarget {
  const float4* pts;  // sorted
  const int* perm;    // sorted position -> the caller's index
  const Box* cbox;
  const Box* gbox;    // groups, then super boxes
  int n;
  int pad_;
};

enum { SQ_KNN = 0, SQ_COUNT = 1, SQ_FILL = 2 };

// per-lane state of the walk
template <int MODE>
struct SearchLane;
template <>
struct SearchLane<SQ_KNN> {
  unsigned long long* col;  // the lane's LDS column: col[s * SQ_BLK]
  unsigned long long worst;
  int worst_at, k;
  float bound;  // distance of the k-th key, +Inf while the list is not full
  __device__ __forceinline__ void take(unsigned long long key) {
    if (key < worst) {
      col[worst_at * SQ_BLK] = key;
      worst = 0;
      for (int s = 0; s < k; s++) {
        const unsigned long long v = col[s * SQ_BLK];
        if (v >= worst) worst = v, worst_at = s;
      }
      bound = worst == ~0ull ? __builtin_inff() : __uint_as_float((unsigned)(worst >> 32));
    }
  }
};
template <>
struct SearchLane<SQ_COUNT> {
  int cnt;
  float bound;
  __device__ __forceinline__ void take(unsigned long long) { cnt++; }
};
template <>
struct SearchLane<SQ_FILL> {
  unsigned long long* row;
  int cnt, len;
  float bound;
  __device__ __forceinline__ void take(unsigned long long key) {
    if (cnt < len) row[cnt] = key;  // (len is what k_radius_count found: the same walk, so cnt never reaches it early)
    cnt++;
  }
};

// does a lane with this state still need a box whose lower bound is lb?  (Strict on the k-th distance: a tie may carry a smaller index.
// A hit needs d2 < r2 and lb <= d2, so lb >= r2 holds no hit.)
__device__ __forceinline__ bool sq_need(float lb, float bound, bool bounded, float r2) { return !(lb > bound) && (!bounded || lb < r2); }

// One wave: lane `active` searches T for q.  Returns the number of groups whose points were looked at (wave-uniform).
template <int MODE>
__device__ __forceinline__ int search_walk(const SearchTarget& T, const float4 q, bool active, bool bounded, float r2, SearchLane<MODE>& st, int lane) {
  const int n = T.n, ngr = (n + kGroupPts - 1) / kGroupPts, nch = (n + kChunk - 1) / kChunk;
  const bool use_super = n > SORT_LDS_MAX_N;  // (apd_sort.hpp: only large clouds carry super boxes)
  const float inf = __builtin_inff();
  // the wave's query box (inactive lanes carry a copy of an active lane's query)
  Box wb;
  wb.lx = wave_min(q.x), wb.ly = wave_min(q.y), wb.lz = wave_min(q.z);
  wb.hx = wave_max(q.x), wb.hy = wave_max(q.y), wb.hz = wave_max(q.z);
  // the group nearest that box (ties: the first on the curve)
  float blb = inf;
  int bg = 0x7fffffff;
  for (int g0 = 0; g0 < ngr; g0 += 64) {
    const int g = g0 + lane;
    if (g < ngr) {
      const float lb = lb_box_box(wb, G(T.gbox)[g]);
      if (lb < blb || bg == 0x7fffffff) blb = lb, bg = g;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float olb = __shfl_xor(blb, off, 64);
    const int og = __shfl_xor(bg, off, 64);
    if (og != 0x7fffffff && (bg == 0x7fffffff || olb < blb || (olb == blb && og < bg))) blb = olb, bg = og;
  }
  const int gstart = __builtin_amdgcn_readfirstlane(bg);
  int up = gstart, down = gstart - 1, visited = 0;
  // at most ngr groups upwards and ngr downwards, one per step
  for (int it = 0; it < 2 * ngr; it++) {
    if (up >= ngr && down < 0) break;
    int g;
    if ((it & 1) == 0) {
      if (up >= ngr) continue;
      if (use_super && up % kSuperGroups == 0 && up + kSuperGroups <= ngr) {  // a whole super box ahead
        const Box sb = G(T.gbox)[ngr + up / kSuperGroups];
        if (!__ballot(active && sq_need(lb_point_box(sb, q.x, q.y, q.z), st.bound, bounded, r2))) {
          up += kSuperGroups;
          continue;
        }
      }
      g = up++;
    } else {
      if (down < 0) continue;
      if (use_super && (down + 1) % kSuperGroups == 0) {
        const Box sb = G(T.gbox)[ngr + down / kSuperGroups];
        if (!__ballot(active && sq_need(lb_point_box(sb, q.x, q.y, q.z), st.bound, bounded, r2))) {
          down -= kSuperGroups;
          continue;
        }
      }
      g = down--;
    }
    const Box gb = G(T.gbox)[g];
    if (!__ballot(active && sq_need(lb_point_box(gb, q.x, q.y, q.z), st.bound, bounded, r2))) continue;
    visited++;
    const int c1 = min((g + 1) * kGroupChunks, nch);
    for (int c = g * kGroupChunks; c < c1; c++) {
      const Box cb = G(T.cbox)[c];
      if (!__ballot(active && sq_need(lb_point_box(cb, q.x, q.y, q.z), st.bound, bounded, r2))) continue;
      const int j1 = min((c + 1) * kChunk, n);
      for (int j = c * kChunk; j < j1; j++) {  // (every lane looks: a lane whose bound excluded the chunk finds nothing there)
        const float4 t = G(T.pts)[j];
        const float d = sqdist1(t.x, t.y, t.z, q.x, q.y, q.z);
        if (active && (!bounded || d < r2)) st.take(dist_key(d, G(T.perm)[j]));
      }
    }
  }
  return visited;
}

// the lane's query: sorted position i of the query cloud (clamped: lanes past the end repeat the last query and stay inactive)
__device__ __forceinline__ float4 sq_query(const float4* qpts, int nq, int i) { return G(qpts)[min(i, nq - 1)]; }

// out_keys: [nq][k] in the caller's query order, ascending, ~0 where the row has no further key; out_cnt[nq]: keys of the row
__global__ __launch_bounds__(SQ_BLK) void k_knn_queries(SearchTarget T, const float4* qpts, const int* qperm, int nq, int k, int bounded, float r2,
                                                        unsigned long long* out_keys, int* out_cnt, int* visited) {
  __shared__ unsigned long long best[SQ_KMAX * SQ_BLK];  // [slot][lane]
  const int lane = threadIdx.x, i = blockIdx.x * SQ_BLK + lane;
  const bool active = i < nq;
  const float4 q = sq_query(qpts, nq, i);
  SearchLane<SQ_KNN> st;
  st.col = best + lane, st.worst = ~0ull, st.worst_at = 0, st.k = k, st.bound = __builtin_inff();
  for (int s = 0; s < k; s++) st.col[s * SQ_BLK] = ~0ull;
  const int v = search_walk<SQ_KNN>(T, q, active, bounded != 0, r2, st, lane);
  if (lane == 0) visited[blockIdx.x] = v;
  if (!active) return;
  unsigned long long* out = out_keys + (size_t)G(qperm)[i] * k;
  unsigned long long prev = 0;
  int cnt = 0;
  for (int r = 0; r < k; r++) {  // ascending: the smallest key above the previous one (keys are unique)
    unsigned long long m = ~0ull;
    for (int s = 0; s < k; s++) {
      const unsigned long long v2 = st.col[s * SQ_BLK];
      if ((r == 0 || v2 > prev) && v2 < m) m = v2;
    }
    prev = m;
    cnt += m != ~0ull ? 1 : 0;
    out[r] = m;
  }
  out_cnt[G(qperm)[i]] = cnt;
}

__global__ __launch_bounds__(SQ_BLK) void k_radius_count(SearchTarget T, const float4* qpts, const int* qperm, int nq, float r2, int* out_cnt, int* visited) {
  const int lane = threadIdx.x, i = blockIdx.x * SQ_BLK + lane;
  const bool active = i < nq;
  const float4 q = sq_query(qpts, nq, i);
  SearchLane<SQ_COUNT> st;
  st.cnt = 0, st.bound = __builtin_inff();
  const int v = search_walk<SQ_COUNT>(T, q, active, true, r2, st, lane);
  if (lane == 0) visited[blockIdx.x] = v;
  if (active) out_cnt[G(qperm)[i]] = st.cnt;
}

// pos[i] = counts before i inside its block of SCAN_BLK; bsum[b] = the block's total
__global__ __launch_bounds__(SCAN_BLK) void k_radius_scan(const int* cnt, int n, int* pos, int* bsum) {
  __shared__ int lds[SCAN_BLK / 64];
  const int tid = threadIdx.x, i = blockIdx.x * SCAN_BLK + tid;
  int total;
  const int ex = block_exclusive_scan(i < n ? cnt[i] : 0, lds, tid, &total);
  if (i < n) pos[i] = ex;
  if (tid == 0) bsum[blockIdx.x] = total;
}

// row of query o (the caller's index): rows + pos[o] + bsum[o / SCAN_BLK], cnt[o] keys
__global__ __launch_bounds__(SQ_BLK) void k_radius_fill(SearchTarget T, const float4* qpts, const int* qperm, int nq, float r2, const int* cnt, const int* pos,
                                                        const int* bsum, unsigned long long* rows) {
  const int lane = threadIdx.x, i = blockIdx.x * SQ_BLK + lane;
  const bool active = i < nq;
  const float4 q = sq_query(qpts, nq, i);
  const int o = G(qperm)[min(i, nq - 1)];
  SearchLane<SQ_FILL> st;
  st.row = rows + ((size_t)pos[o] + (size_t)bsum[o / SCAN_BLK]), st.cnt = 0, st.len = active ? cnt[o] : 0, st.bound = __builtin_inff();
  search_walk<SQ_FILL>(T, q, active, true, r2, st, lane);
}

// One block per row.  A bitonic network whose comparators all point the same way (the first step of a merge mirrors, the others
// halve), over the next power of two above the row's length: positions past the end stand for +Inf keys, which no comparator moves.
__global__ __launch_bounds__(SQ_SORT_BLK) void k_radius_sort_rows(const int* cnt, const int* pos, const int* bsum, unsigned long long* rows) {
  const int o = blockIdx.x, tid = threadIdx.x;
  const int len = cnt[o];  // (block-uniform: every barrier below is reached by the whole block)
  if (len < 2) return;
  unsigned long long* a = rows + ((size_t)pos[o] + (size_t)bsum[o / SCAN_BLK]);
  for (unsigned k2 = 2; (k2 >> 1) < (unsigned)len; k2 <<= 1) {  // (len <= 2^30: k2 stops at 2^31 at the latest)
    for (unsigned jj = k2 >> 1; jj > 0; jj >>= 1) {
      const int mask = (int)(jj == (k2 >> 1) ? k2 - 1 : jj);
      for (int lo = tid; lo < len; lo += SQ_SORT_BLK) {
        const int hi = lo ^ mask;
        if (hi > lo && hi < len) {
          const unsigned long long x = a[lo], y = a[hi];
          if (y < x) a[lo] = y, a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace apd
