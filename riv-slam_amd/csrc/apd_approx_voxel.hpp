// downsample_method "APPROX_VOXELGRID" on the device (include/apdgicp_hip.h, AV1 .. AV7): pcl::ApproximateVoxelGrid<PointXYZI>::applyFilter
// (PCL 1.10, filters/impl/approximate_voxel_grid.hpp) -- preprocessing_nodelet.cpp:145-149, scan_matching_odometry_nodelet.cpp:156-160 and the
// only downsampler of fast_apdgicp's own programs (align.cpp:136-147, kitti.cpp:81).
//
// PCL's loop is sequential and order dependent: a table of 512 entries {ix, iy, iz, count, centroid}, addressed by a hash of the voxel; a point
// whose entry holds another voxel flushes that entry to the output and takes it over; what is left at the end is flushed in entry order.  The
// same bytes come out of a parallel form, because an entry only ever sees the points of its own hash, in input order:
//   1. k_av_keys       per point the voxel (AV2) and its hash (AV3); a non-finite point gets AV_SKIP, which sorts last (AV7)
//   2. the stable radix sort of apd_map.hpp by hash (two 8-bit passes), value = point index: inside a hash the points stay in input order
//   3. k_av_heads      a RUN is a maximal stretch of one hash with one voxel -- exactly one stay of that voxel in the entry.  The first point
//                      of a run that is not the first run of its hash is the point that evicted the run before it: evict[point] = 1
//   4. an exclusive scan of evict[] over the INPUT order (k_map_scan_tiles / k_scan_bsum): evictions are emitted in the order of the points
//      that caused them, so a run that is followed by another run of its hash lands at the scanned value of that run's first point
//   5. k_av_occ        the last run of every hash is flushed at the end, in ascending hash: total evictions + occupied hashes below
//   6. k_av_centroids  one lane per run adds its points in sorted = input order (fp32, from zero, as the entry's centroid does) and divides by
//                      (float)count.  A run can be long -- a cloud inside one voxel is ONE run of n points that one lane adds alone: the order
//                      of the additions IS the result, so it is not split.
// No atomics on floats, no second sort, everything on the caller's stream; n_out = the number of runs.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_map.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int AV_HIST = 512;       // histsize_
constexpr int AV_SKIP = AV_HIST;   // hash of a point that takes no part
constexpr int AV_BLK = 256;        // k_av_keys / k_av_heads / k_av_centroids: one point or sorted position per lane
constexpr int AV_SORT_PASSES = 2;  // 10 key bits

// AV2: (int)floorf(c * inv), the product rounded on its own; what does not fit an int -- NaN included -- is INT_MIN, the x86-64 conversion's
// "integer indefinite" (the GPU's own conversion would saturate to INT_MAX on the positive side)
__device__ __forceinline__ int av_index(float c, float inv) {
  const float v = floorf(__fmul_rn(c, inv));
  return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000;
}
struct AvVoxel {
  int x, y, z;
};
__device__ __forceinline__ AvVoxel av_voxel(const float4& p, float ilx, float ily, float ilz) { return AvVoxel{av_index(p.x, ilx), av_index(p.y, ily), av_index(p.z, ilz)}; }
__device__ __forceinline__ bool av_same(const AvVoxel& a, const AvVoxel& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// AV3, in unsigned arithmetic (two's complement wrap-around)
__device__ __forceinline__ int av_hash(const AvVoxel& v) { return (int)(((unsigned)v.x * 7171u + (unsigned)v.y * 3079u + (unsigned)v.z * 4231u) & (unsigned)(AV_HIST - 1)); }

// words: [0] evictions, [1] n_out, [2, 2 + AV_HIST) per hash: occupied (k_av_heads), then the occupied hashes below it (k_av_occ)
constexpr int AV_WORDS = 2 + AV_HIST;

__global__ __launch_bounds__(AV_BLK) void k_av_keys(const float4* pts, int n, float ilx, float ily, float ilz, unsigned long long* keys, int* vals, int* evict, int* words) {
  const int i = blockIdx.x * AV_BLK + threadIdx.x;
  if (blockIdx.x == 0)
    for (int w = threadIdx.x; w < AV_WORDS; w += AV_BLK) words[w] = 0;
  if (i >= n) return;
  const float4 p = pts[i];
  keys[i] = finite3(p) ? (unsigned long long)av_hash(av_voxel(p, ilx, ily, ilz)) : (unsigned long long)AV_SKIP;
  vals[i] = i;
  evict[i] = 0;
}

// head[s]: sorted position s starts a run (or holds a skipped point, which k_av_centroids passes over)
__global__ __launch_bounds__(AV_BLK) void k_av_heads(const unsigned long long* keys, const int* vals, const float4* pts, int n, float ilx, float ily, float ilz,
                                                     unsigned char* head, int* evict, int* words) {
  const int s = blockIdx.x * AV_BLK + threadIdx.x;
  if (s >= n) return;
  const int h = (int)keys[s];
  if (h >= AV_HIST) {
    head[s] = 1;
    return;
  }
  const bool first = s == 0 || (int)keys[s - 1] != h;
  bool hd = first;
  const unsigned cp = (unsigned)vals[s];
  if (!first && cp < (unsigned)n) {
    const unsigned prev = (unsigned)vals[s - 1];
    hd = prev >= (unsigned)n || !av_same(av_voxel(pts[cp], ilx, ily, ilz), av_voxel(pts[prev], ilx, ily, ilz));
    if (hd) evict[cp] = 1;  // AV4: this point found another voxel in its entry
  }
  if (first) words[2 + h] = 1;
  head[s] = hd ? 1 : 0;
}

// AV5: exclusive scan of the occupied flags of the 512 entries; n_out = evictions + occupied entries
__global__ __launch_bounds__(SCAN_BLK) void k_av_occ(int* words) {
  __shared__ int lds[SCAN_BLK / 64];
  const int tid = threadIdx.x;
  int total;
  const int ex = block_exclusive_scan(tid < AV_HIST ? words[2 + tid] : 0, lds, tid, &total);
  if (tid < AV_HIST) words[2 + tid] = ex;
  if (tid == 0) words[1] = words[0] + total;
}

// AV4 / AV5: centroid / (float)count per component, a true fp32 division
__global__ __launch_bounds__(AV_BLK) void k_av_centroids(const unsigned long long* keys, const int* vals, const unsigned char* head, const float4* pts, const int* evict,
                                                         const int* tile_sums, const int* words, int n, float4* out, int out_cap) {
  const int s = blockIdx.x * AV_BLK + threadIdx.x;
  if (s >= n || !head[s]) return;
  const int h = (int)keys[s];
  if (h >= AV_HIST) return;
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
  int cnt = 0, e = s;
  do {
    const unsigned i = (unsigned)vals[e];
    if (i < (unsigned)n) {
      const float4 p = pts[i];
      sx = __fadd_rn(sx, p.x), sy = __fadd_rn(sy, p.y), sz = __fadd_rn(sz, p.z), sw = __fadd_rn(sw, p.w);
    }
    cnt++, e++;
  } while (e < n && !head[e]);
  int slot;
  if (e < n && (int)keys[e] == h) {  // evicted by the first point of the next run of this entry
    const unsigned cp = (unsigned)vals[e];
    slot = cp < (unsigned)n ? evict[cp] + tile_sums[cp / (SCAN_BLK * SCAN_ITEMS)] : -1;
  } else {                           // still in the table at the end
    slot = words[0] + words[2 + h];
  }
  const float fn = (float)cnt;
  if (slot >= 0 && slot < out_cap) out[slot] = make_float4(__fdiv_rn(sx, fn), __fdiv_rn(sy, fn), __fdiv_rn(sz, fn), __fdiv_rn(sw, fn));
}

}  // namespace apd
