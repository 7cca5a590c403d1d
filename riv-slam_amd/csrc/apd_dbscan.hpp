// DBSCAN clustering on the device: DBSCANSimpleCluster::extract (radar_graph_slam/include/dbscan/DBSCAN_simple.h:27-90, radiusSearch :118-142;
// DBSCAN_precomp.h stores the same distances), the "dynamic-object clustering" of the moving points that the ego-velocity estimate rejects
// (preprocessing_nodelet.cpp:766-774).  The semantics are the numbered list D1 .. D7 of include/apdgicp_hip.h; the reference's sequential
// loop is restated there as properties of the adjacency graph, and the kernels below compute those properties in parallel:
//   k_db_keys        the integer cell of every point, cell side h = eps * (1 + 2^-20) (why: below); non-finite points get no cell, the first
//                    finite point outside |c| < 2^20 is reported
//   (sort)           the map cloud's stable LSD radix sort (apd_map.hpp) over (cell key, point index) pairs
//   k_db_gather      the sorted copy: point + original index, and the sorted keys (the sort's scratch is reused below)
//   k_db_count       D1 / D2: one lane per point in cell order walks the 27 cells around its own -- 9 binary searches over the sorted keys,
//                    the three cells of a z column are consecutive keys -- and counts the adjacent points; cnt, the core flag, parent = self
//   k_db_union       D3: every core-core edge once (from its larger index): the larger ROOT is hooked under the smaller one with a 32-bit
//                    atomicCAS on the parent array; a parent only ever points to a smaller index, so there are no cycles and the root of a
//                    component is its smallest core index -- D3's seed -- whatever order the atomics land in.  atomicMin shortens the
//                    path of the point a find started from; an edge whose far end already points at this lane's root costs one load.
//   k_db_flatten     every core point walks to its root (pointer jumping over the hook edges); root[] is a second array: no lane reads what
//                    another writes in this launch
//   k_db_border      D4 / D5: a non-core point takes the smallest root among its adjacent cores; adjacent SEED points of other clusters are
//                    counted (second walk for those few points: the sizes of those clusters).  Sizes and core counts: integer atomicAdd.
//   k_db_rank_keys   D6 / D7: a kept seed's key ((2^b - size) << b | seed, b = bits of n), everything else ~0; (sort) again; k_db_rank_table
//                    reads rank -> seed, size back, the sizes are scanned (k_map_scan_tiles / k_scan_bsum): CSR offsets, total
//   -- the host waits ONCE here: first bad point, K, the CSR length --
//   k_db_member_count / k_db_member_emit   every point's memberships in kept clusters, scanned and written in ascending point index as
//                    (rank, index) pairs; the stable sort by rank leaves every cluster's members in ascending index: the CSR indices
//   k_db_labels      the rank of the kept primary cluster or -1
//   k_db_table       one block per kept cluster: fp64 sums in a fixed order (lane t adds members t, t + 256, ... of the CSR row, then a fixed
//                    tree), fp32 min / max, the same for the Doppler lane
// The cell side.  D1 accepts a pair iff dx^2 + dy^2 + dz^2 <= eps^2 with dx = (double)fl32(x_j - x_i), so |fl32(x_j - x_i)| <= eps (1 + 2^-52);
// the fp32 subtraction has relative error <= 2^-24 (a subnormal difference is exact), so the true |x_j - x_i| <= eps (1 + 2^-23).  The cell
// is c = floor(fl64(x / h)): the quotient is monotonic in x and off by at most 2^-53 |x / h| < 2^-32 inside the key range, so the two
// quotients differ by at most eps (1 + 2^-23) / h + 2^-31 < 1 for h = eps (1 + 2^-20), and two reals less than 1 apart have floors at most 1
// apart.  The grid only prunes: every decision is D1's arithmetic on the pair.
// Everything is integer or fp64 / fp32 in written order (no contraction), no floating-point atomics, plain vector stores.  Every pointer
// is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_kernels.hpp"
#include "apd_map.hpp"
#include "apd_vgicp.hpp"

namespace apd {

#pragma clang fp contract(off)

constexpr int DB_BLK = 256;                          // one point (or one cluster's stripe) per lane, 4 waves
constexpr unsigned long long DB_NO_CELL = ~0ull;     // a non-finite point: sorts behind every cell (a cell key has 63 bits)
constexpr int DB_CMAX = 2 * VG_LIM - 1;              // biased cell coordinates are 1 .. DB_CMAX
constexpr int DB_BAD_BASE = 2147483647;              // scal[0] = max over bad points of (DB_BAD_BASE - index); 0: none
enum { DB_W_BAD = 0, DB_W_RADIX = 1, DB_W_K = 2, DB_W_M = 3, DB_W_M2 = 4, DB_WORDS = 8 };

struct DbCluster {  // = apdgicp_dbscan_cluster, byte for byte
  double centroid[3];
  double doppler_mean;
  float mn[3], mx[3];
  float doppler_min, doppler_max;
  int seed, size, n_core, reserved;
};

__global__ __launch_bounds__(DB_BLK) void k_db_keys(const float* xyz, int n, int stride /* floats */, const float* dop_in, int dstride /* floats */, double h, float4* pts,
                                                    float* dop, unsigned long long* keys, int* idx, int* scal) {
  const int i = blockIdx.x * DB_BLK + threadIdx.x;
  if (i >= n) return;
  const float* p = xyz + (size_t)i * stride;
  const float4 q = make_float4(p[0], p[1], p[2], 0.f);
  pts[i] = q;
  if (dop_in) dop[i] = dop_in[(size_t)i * dstride];
  unsigned long long key = DB_NO_CELL;
  if (finite3(q)) {
    const double cx = floor(__ddiv_rn((double)q.x, h)), cy = floor(__ddiv_rn((double)q.y, h)), cz = floor(__ddiv_rn((double)q.z, h));
    if (vg_in_range(cx) && vg_in_range(cy) && vg_in_range(cz)) key = vg_pack((int)cx, (int)cy, (int)cz);
    else atomicMax(scal + DB_W_BAD, DB_BAD_BASE - i);
  }
  keys[i] = key, idx[i] = i;
}

__global__ __launch_bounds__(DB_BLK) void k_db_gather(const unsigned long long* keys, const int* sidx, const float4* pts, int n, unsigned long long* gkeys, float4* spts) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n) return;
  const int o = sidx[s];
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)o < (unsigned)n) p = pts[o];
  p.w = __int_as_float(o);
  spts[s] = p, gkeys[s] = keys[s];
}

// D1 for the pair (q, p)
__device__ __forceinline__ bool db_adjacent(const float4& q, const float4& p, double eps2) {
  const double dx = (double)__fsub_rn(p.x, q.x), dy = (double)__fsub_rn(p.y, q.y), dz = (double)__fsub_rn(p.z, q.z);
  return (dx * dx + dy * dy) + dz * dz <= eps2;
}
// f(t, p) for every sorted position t != s whose point p is adjacent to the point at s
template <typename F>
__device__ __forceinline__ void db_walk(const unsigned long long* keys, const float4* spts, int n, int s, double eps2, F&& f) {
  const unsigned long long k = keys[s];
  if (k == DB_NO_CELL) return;
  const float4 q = spts[s];
  const int cx = (int)(k >> 42), cy = (int)((k >> 21) & 0x1fffff), cz = (int)(k & 0x1fffff);
  const unsigned long long zlo = (unsigned long long)max(cz - 1, 1), zhi = (unsigned long long)min(cz + 1, DB_CMAX);
  for (int ox = -1; ox <= 1; ox++) {
    for (int oy = -1; oy <= 1; oy++) {
      const int bx = cx + ox, by = cy + oy;
      if (bx < 1 || bx > DB_CMAX || by < 1 || by > DB_CMAX) continue;
      const unsigned long long base = ((unsigned long long)bx << 42) | ((unsigned long long)by << 21);
      const unsigned long long klo = base | zlo, khi = base | zhi;
      int lo = 0, hi = n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < klo) lo = mid + 1;
        else hi = mid;
      }
      for (int t = lo; t < n && keys[t] <= khi; t++) {
        if (t == s) continue;
        const float4 p = spts[t];
        if (db_adjacent(q, p, eps2)) f(t, p);
      }
    }
  }
}

__global__ __launch_bounds__(DB_BLK) void k_db_count(const unsigned long long* keys, const float4* spts, int n, double eps2, int min_pts, int* cnt, unsigned char* core,
                                                     unsigned char* score, int* parent, int* size, int* ncore) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n) return;
  const int o = __float_as_int(spts[s].w);
  int c = 1;  // D2: the point itself
  db_walk(keys, spts, n, s, eps2, [&](int, const float4&) { c++; });
  const unsigned char is_core = c >= min_pts ? 1 : 0;
  score[s] = is_core;
  if ((unsigned)o >= (unsigned)n) return;
  cnt[o] = c, core[o] = is_core, parent[o] = o, size[o] = 0, ncore[o] = 0;
}

__device__ __forceinline__ int db_find(const int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
// hooks the trees of a0 and b0 together; returns the root both are under afterwards
__device__ __forceinline__ int db_union(int* parent, int a0, int b0) {
  int a = db_find(parent, a0), b = db_find(parent, b0);
  if (a != a0) atomicMin(parent + a0, a);  // (a0 is not a root and never becomes one again: no CAS below can succeed on it)
  if (b != b0) atomicMin(parent + b0, b);
  for (;;) {
    if (a == b) return a;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return b;
    a = db_find(parent, old), b = db_find(parent, b);  // someone else hooked a first
  }
}
__global__ __launch_bounds__(DB_BLK) void k_db_union(const unsigned long long* keys, const float4* spts, const unsigned char* score, int n, double eps2, int* parent) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n || !score[s]) return;
  const int o = __float_as_int(spts[s].w);
  if ((unsigned)o >= (unsigned)n) return;
  int mine = o;  // an ancestor of o (or o): where the last union left it
  db_walk(keys, spts, n, s, eps2, [&](int t, const float4& p) {
    const int ot = __float_as_int(p.w);
    if (!score[t] || ot >= o || ot < 0) return;
    // Every value parent[ot] ever holds is ot or an ancestor of ot, and hook edges are never removed: if it equals an ancestor of o, the two
    // are in one tree already.  In a dense blob that is nearly every edge after the first few: one load instead of two finds and a CAS.
    if (__hip_atomic_load(parent + ot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mine) return;
    mine = db_union(parent, mine, ot);
  });
}
__global__ __launch_bounds__(DB_BLK) void k_db_flatten(const int* parent, const unsigned char* core, int n, int* root) {
  const int i = blockIdx.x * DB_BLK + threadIdx.x;
  if (i >= n) return;
  root[i] = core[i] ? db_find(parent, i) : -1;
}

__global__ __launch_bounds__(DB_BLK) void k_db_border(const unsigned long long* keys, const float4* spts, const unsigned char* score, const int* root, int n, double eps2,
                                                      int* seed, int* nextra, int* size, int* ncore) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n) return;
  const int o = __float_as_int(spts[s].w);
  if ((unsigned)o >= (unsigned)n) return;
  if (score[s]) {
    const int r = root[o];
    seed[o] = r, nextra[o] = 0;
    if ((unsigned)r < (unsigned)n) atomicAdd(size + r, 1), atomicAdd(ncore + r, 1);
    return;
  }
  int prim = n, first_seed = n, n_seeds = 0;
  db_walk(keys, spts, n, s, eps2, [&](int t, const float4& p) {
    if (!score[t]) return;
    const int ot = __float_as_int(p.w);
    if ((unsigned)ot >= (unsigned)n) return;
    const int r = root[ot];
    prim = min(prim, r);
    if (r == ot) n_seeds++, first_seed = min(first_seed, ot);
  });
  const int extras = n_seeds - (first_seed == prim && n_seeds > 0 ? 1 : 0);  // D5: the seed POINTS of other clusters it is adjacent to
  seed[o] = prim < n ? prim : -1, nextra[o] = extras;
  if ((unsigned)prim < (unsigned)n) atomicAdd(size + prim, 1);
  if (extras > 0)
    db_walk(keys, spts, n, s, eps2, [&](int t, const float4& p) {
      const int ot = __float_as_int(p.w);
      if (score[t] && (unsigned)ot < (unsigned)n && root[ot] == ot && ot != prim) atomicAdd(size + ot, 1);
    });
}

// D6 / D7.  bits: n <= 2^bits
__global__ __launch_bounds__(DB_BLK) void k_db_rank_keys(const unsigned char* core, const int* root, const int* size, int n, int bits, int min_size, int max_size,
                                                         unsigned long long* keys, int* idx, int* rank_of, int* scal) {
  const int i = blockIdx.x * DB_BLK + threadIdx.x;
  bool kept = false;
  if (i < n) {
    const int sz = size[i];
    kept = core[i] && root[i] == i && sz >= min_size && sz <= max_size && sz <= n;
    keys[i] = kept ? ((unsigned long long)((1u << bits) - (unsigned)sz) << bits) | (unsigned)i : ~0ull;
    idx[i] = i, rank_of[i] = -1;
  }
  const int c = __popcll(__ballot(kept));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(scal + DB_W_K, c);
}
__global__ __launch_bounds__(DB_BLK) void k_db_rank_table(const unsigned long long* keys, const int* size, int n, int bits, const int* scal, int* rank_of, int* cseed, int* csize) {
  const int r = blockIdx.x * DB_BLK + threadIdx.x;
  if (r >= n) return;
  int sd = -1, sz = 0;
  if (r < scal[DB_W_K]) {
    sd = (int)(keys[r] & ((1ull << bits) - 1));
    if ((unsigned)sd < (unsigned)n) sz = size[sd], rank_of[sd] = r;
  }
  cseed[r] = sd, csize[r] = sz;
}
// offsets[0 .. K]: csize scanned in tiles (k_map_scan_tiles) + the scanned tile sums; offsets[K] = the total
__global__ __launch_bounds__(DB_BLK) void k_db_offsets(const int* csize, const int* tsum, int K, int total, int* offsets) {
  const int r = blockIdx.x * DB_BLK + threadIdx.x;
  if (r > K) return;
  offsets[r] = r < K ? csize[r] + tsum[r / (SCAN_BLK * SCAN_ITEMS)] : total;
}

// a point's memberships in KEPT clusters: its primary cluster and, for the few border points of D5, the other seeds it touches
__global__ __launch_bounds__(DB_BLK) void k_db_member_count(const unsigned long long* keys, const float4* spts, const unsigned char* score, const int* root, const int* seed,
                                                            const int* nextra, const int* rank_of, int n, double eps2, int* mcount) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n) return;
  const int o = __float_as_int(spts[s].w);
  if ((unsigned)o >= (unsigned)n) return;
  const int prim = seed[o];
  int m = (unsigned)prim < (unsigned)n && rank_of[prim] >= 0 ? 1 : 0;
  if (nextra[o] > 0)
    db_walk(keys, spts, n, s, eps2, [&](int t, const float4& p) {
      const int ot = __float_as_int(p.w);
      if (score[t] && (unsigned)ot < (unsigned)n && root[ot] == ot && ot != prim && rank_of[ot] >= 0) m++;
    });
  mcount[o] = m;
}
__global__ __launch_bounds__(DB_BLK) void k_db_member_emit(const unsigned long long* keys, const float4* spts, const unsigned char* score, const int* root, const int* seed,
                                                           const int* nextra, const int* rank_of, const int* mpos, const int* tsum, int n, double eps2, int M,
                                                           unsigned long long* pkeys, int* pidx) {
  const int s = blockIdx.x * DB_BLK + threadIdx.x;
  if (s >= n) return;
  const int o = __float_as_int(spts[s].w);
  if ((unsigned)o >= (unsigned)n) return;
  int pos = mpos[o] + tsum[o / (SCAN_BLK * SCAN_ITEMS)];
  const int prim = seed[o];
  if ((unsigned)prim < (unsigned)n && rank_of[prim] >= 0) {
    if ((unsigned)pos < (unsigned)M) pkeys[pos] = (unsigned long long)rank_of[prim], pidx[pos] = o;
    pos++;
  }
  if (nextra[o] > 0)
    db_walk(keys, spts, n, s, eps2, [&](int t, const float4& p) {
      const int ot = __float_as_int(p.w);
      if (score[t] && (unsigned)ot < (unsigned)n && root[ot] == ot && ot != prim && rank_of[ot] >= 0) {
        if ((unsigned)pos < (unsigned)M) pkeys[pos] = (unsigned long long)rank_of[ot], pidx[pos] = o;
        pos++;
      }
    });
}

__global__ __launch_bounds__(DB_BLK) void k_db_labels(const int* seed, const int* rank_of, int n, int* labels) {
  const int i = blockIdx.x * DB_BLK + threadIdx.x;
  if (i >= n) return;
  const int sd = seed[i];
  labels[i] = (unsigned)sd < (unsigned)n ? rank_of[sd] : -1;
}

// min / max that hand a NaN on (a cluster with a non-finite member is that member alone: D1)
__device__ __forceinline__ float db_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float db_max(float a, float b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(DB_BLK) void k_db_table(const int* offsets, const int* members, const int* cseed, const int* ncore, const float4* pts, const float* dop, int n,
                                                     DbCluster* out) {
  __shared__ double rs[DB_BLK / 64][4];
  __shared__ float rmn[DB_BLK / 64][4], rmx[DB_BLK / 64][4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = offsets[r], e = offsets[r + 1];
  const float inf = __builtin_inff();
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  float mn[4] = {inf, inf, inf, inf}, mx[4] = {-inf, -inf, -inf, -inf};
  for (int j = b + tid; j < e; j += DB_BLK) {
    const int o = members[j];
    if ((unsigned)o >= (unsigned)n) continue;
    const float4 p = pts[o];
    const float v[4] = {p.x, p.y, p.z, dop ? dop[o] : 0.f};
#pragma unroll
    for (int a = 0; a < 4; a++) sum[a] += (double)v[a], mn[a] = db_min(mn[a], v[a]), mx[a] = db_max(mx[a], v[a]);
  }
#pragma unroll
  for (int a = 0; a < 4; a++) {
    for (int off = 32; off > 0; off >>= 1) {
      sum[a] += __shfl_down(sum[a], off, 64);
      mn[a] = db_min(mn[a], __shfl_down(mn[a], off, 64)), mx[a] = db_max(mx[a], __shfl_down(mx[a], off, 64));
    }
    if (lane == 0) rs[wave][a] = sum[a], rmn[wave][a] = mn[a], rmx[wave][a] = mx[a];
  }
  __syncthreads();
  if (tid != 0) return;
  DbCluster c;
  const double fn = (double)(e - b);
  double tot[4];
  float lo[4], hi[4];
  for (int a = 0; a < 4; a++) {
    tot[a] = (rs[0][a] + rs[1][a]) + (rs[2][a] + rs[3][a]);
    lo[a] = db_min(db_min(rmn[0][a], rmn[1][a]), db_min(rmn[2][a], rmn[3][a]));
    hi[a] = db_max(db_max(rmx[0][a], rmx[1][a]), db_max(rmx[2][a], rmx[3][a]));
  }
  for (int a = 0; a < 3; a++) c.centroid[a] = tot[a] / fn, c.mn[a] = lo[a], c.mx[a] = hi[a];
  c.doppler_mean = dop ? tot[3] / fn : 0.0, c.doppler_min = dop ? lo[3] : 0.f, c.doppler_max = dop ? hi[3] : 0.f;
  const int sd = cseed[r];
  c.seed = sd, c.size = e - b, c.n_core = (unsigned)sd < (unsigned)n ? ncore[sd] : 0, c.reserved = 0;
  out[r] = c;
}

}  // namespace apd
