// Scan preprocessing on the device: the three filters every cloud passes before it reaches setInputSource
// (PreprocessingNodelet::cloud_callback, radar_graph_slam/apps/preprocessing_nodelet.cpp:812-815):
//   preprocessing_nodelet.cpp:881-889  distance_filter: std::copy_if with  d > near && d < far && z < z_high && z > z_low,
//                                      d = p.getVector3fMap().norm() (fp32) and z widened to double;
//   preprocessing_nodelet.cpp:850-866  downsample: pcl::VoxelGrid (apd_voxel.hpp, the kernels of the submap target) or, without a
//                                      filter, pcl::removeNaNFromPointCloud;
//   preprocessing_nodelet.cpp:868-879  outlier_removal: pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval.
// PCL is not part of the reference tree; the kernels follow its published algorithm (filters/impl/statistical_outlier_removal.hpp,
// filters/impl/radius_outlier_removal.hpp):
//   StatisticalOutlierRemoval::applyFilterIndices  per point the mean_k + 1 nearest neighbours (the point itself first),
//        distances[i] = (float)(sum_{r = 1 .. mean_k} sqrt(d2[r]) / mean_k)  -- std::sqrt(float), double sum in rank order;
//        sum += distances[i], sq_sum += distances[i] * distances[i] (float product, double sums);
//        mean = sum / n, variance = (sq_sum - sum * sum / n) / (n - 1), threshold = mean + std_mul * sqrt(variance);
//        a point stays iff distances[i] <= threshold;
//   RadiusOutlierRemoval::applyFilterIndices (dense cloud)  nearestKSearch(i, min_pts_radius, ...) -- the point itself included, so the
//        reference's "min_neighbors" other points need k = min_neighbors + 1 -- and the point stays iff d2[k - 1] <= radius * radius.
// Both are the exact k-NN of apd_kernels.hpp (knn_cov_coop_wave) with another epilogue; what is new here is the range
// gate, the order-preserving compaction and the threshold.  The one deviation: PCL adds sum / sq_sum point after point, this file in a
// fixed tree (k_flt_threshold) -- the same bits from run to run, the last bits of mean / threshold may differ from PCL's.
#pragma once
#include <hip/hip_runtime.h>

#include "apd_kernels.hpp"
#include "apd_voxel.hpp"

namespace apd {

constexpr int FLT_BLK = 1024;  // threads of a compaction block: 16 waves, one point per lane

// the statistic pass: phases A-C of the covariance k-NN for ONE cloud in the single-cloud (latency) shape, L = 16 lanes per query
template <int EPI>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(APD_KNN_WPE, 8))) void k_knn_stat_coop(const CloudDesc* clouds, const int* cloud_ids, int k, int* err_flag,
                                                                                                       unsigned long long* stats, float* stat_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long knn_smem[];
  unsigned bx, by;
  xcd_remap(bx, by);
  const CloudDesc c = clouds[cloud_ids[by]];
  knn_cov_coop_wave<16, EPI>(c, bx, (int)threadIdx.x, knn_smem, k, 0, err_flag, stats, 0, stat_out);
}
// ... and the cross-check (APDGICP_KNN_MODE=brute), written for this file: one lane per query, every point of the cloud visited in
// curve order, the k smallest keys (fp32 distance bits << 32 | original index: the order of every other k-NN kernel here, sqdist1's
// arithmetic) kept in the lane's own LDS column -- a candidate below the column's largest key replaces it, and the largest is
// looked up again -- then taken out in ascending order.  O(n k) per query in the worst case, a few n in practice.
constexpr int STAT_BRUTE_BLK = 128;
template <int EPI>
__global__ __launch_bounds__(STAT_BRUTE_BLK) void k_knn_stat_brute(const CloudDesc* clouds, const int* cloud_ids, int k, int* err_flag, float* stat_out) {
  __shared__ unsigned long long best[KNN_NC * STAT_BRUTE_BLK];  // [slot][lane]
  const CloudDesc c = clouds[cloud_ids[blockIdx.y]];
  const int n = c.n, tid = threadIdx.x, i = blockIdx.x * STAT_BRUTE_BLK + tid;
  if (i >= n) return;  // (no block barrier below: a lane works on its own column only)
  const float4 q = c.pts[i];
  for (int s = 0; s < k; s++) best[s * STAT_BRUTE_BLK + tid] = ~0ull;
  unsigned long long worst = ~0ull;
  int worst_at = 0;
  for (int j = 0; j < n; j++) {
    const float4 t = c.pts[j];
    const unsigned long long key = dist_key(sqdist1(t.x, t.y, t.z, q.x, q.y, q.z), c.perm[j]);
    if (key < worst) {
      best[worst_at * STAT_BRUTE_BLK + tid] = key;
      worst = 0;
      for (int s = 0; s < k; s++) {
        const unsigned long long v = best[s * STAT_BRUTE_BLK + tid];
        if (v >= worst) worst = v, worst_at = s;
      }
    }
  }
  if (worst == ~0ull) {  // fewer than k points at a finite distance: impossible when n >= k and the cloud is finite
    atomicExch(err_flag, 2);
    return;
  }
  double sum = 0.0;
  float last = 0.f;
  unsigned long long prev = 0;
  for (int r = 0; r < k; r++) {  // ascending: the smallest key above the previous one (keys are unique)
    unsigned long long m = ~0ull;
    for (int s = 0; s < k; s++) {
      const unsigned long long v = best[s * STAT_BRUTE_BLK + tid];
      if ((r == 0 || v > prev) && v < m) m = v;
    }
    prev = m;
    last = __uint_as_float((unsigned)(m >> 32));
    if (r >= 1) sum += (double)sqrtf(last);
  }
  stat_out[c.perm[i]] = EPI == KNN_EPI_MEANDIST ? (float)(sum / (double)(k - 1)) : last;
}

struct GateParams {
  double near_, far_, z_low, z_high;
  int on;
  int pad_;
};

// distance_filter (:881-889) + the {x, y, z, intensity} layout of every later stage.  A point that fails the gate becomes
// {NaN, NaN, NaN, intensity}: the voxel grid skips non-finite points and k_flt_count / k_flt_scatter drop them, both in input order,
// so the gated cloud itself is never compacted on its own.  counts[0] += points that passed (an integer atomic per block).
__global__ __launch_bounds__(256) void k_flt_gate(const float* xyz, long long n, int stride /* floats */, int intensity_off /* floats, < 0: none */, GateParams g,
                                                  float4* out, int* counts) {
  __shared__ int wsum[256 / 64];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool pass = false;
  if (i < n) {
    const float* p = xyz + i * stride;
    float4 o = make_float4(p[0], p[1], p[2], intensity_off >= 0 ? p[intensity_off] : 0.f);
    pass = true;
    if (g.on) {
      // Eigen's norm() of a 3-vector: sqrt of the sum of squares, here ((x x + y y) + z z), every operation rounded on its own
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(o.x, o.x), __fmul_rn(o.y, o.y)), __fmul_rn(o.z, o.z));
      const double d = (double)sqrtf(d2), z = (double)o.z;
      pass = d > g.near_ && d < g.far_ && z < g.z_high && z > g.z_low;  // NaN fails every comparison
      if (!pass) {
        const float qnan = __builtin_nanf("");
        o.x = o.y = o.z = qnan;
      }
    }
    out[i] = o;
  }
  const int c = __popcll(__ballot(pass));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(counts, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// Order-preserving compaction in three launches: k_flt_count (per-block counts), k_scan_bsum (apd_voxel.hpp: their exclusive scan and
// the total), k_flt_scatter (slot = block offset + waves before + lanes before: ballot / v_mbcnt inside the wave).
//   PRED 0: the point is finite (the range gate's survivors; removeNaNFromPointCloud)
//   PRED 1: (double)stat[i] <= threshold (the outlier filters); thr_ptr != null: the threshold k_flt_threshold left on the device
template <int PRED>
__device__ __forceinline__ bool flt_keep(const float4* pts, const float* stat, double thr, int i) {
  if constexpr (PRED == 0) return finite3(pts[i]);
  else return (double)stat[i] <= thr;
}
template <int PRED>
__global__ __launch_bounds__(FLT_BLK) void k_flt_count(const float4* pts, const float* stat, double thr, const double* thr_ptr, int n, int* bsum) {
  __shared__ int wsum[FLT_BLK / 64];
  const int tid = threadIdx.x, i = blockIdx.x * FLT_BLK + tid;
  if (thr_ptr) thr = *thr_ptr;
  const bool keep = i < n && flt_keep<PRED>(pts, stat, thr, i);
  const int c = __popcll(__ballot(keep));
  if ((tid & 63) == 0) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < FLT_BLK / 64; w++) s += wsum[w];
    bsum[blockIdx.x] = s;
  }
}
template <int PRED>
__global__ __launch_bounds__(FLT_BLK) void k_flt_scatter(const float4* pts, const float* stat, double thr, const double* thr_ptr, int n, const int* bsum,
                                                         float4* out, int out_cap, unsigned char* kept) {
  __shared__ int wsum[FLT_BLK / 64];
  const int tid = threadIdx.x, i = blockIdx.x * FLT_BLK + tid, wave = tid >> 6;
  if (thr_ptr) thr = *thr_ptr;
  const bool keep = i < n && flt_keep<PRED>(pts, stat, thr, i);
  const unsigned long long m = __ballot(keep);
  if ((tid & 63) == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = bsum[blockIdx.x];
  for (int w = 0; w < wave; w++) before += wsum[w];
  const int slot = mbcnt_add(m, before);  // + kept lanes below this one
  if (i < n && kept) kept[i] = keep ? 1 : 0;
  if (keep && slot < out_cap) out[slot] = pts[i];
}

// StatisticalOutlierRemoval's threshold from the n mean distances: ONE block, lane t adds elements t, t + 1024, ... in index order,
// then a fixed tree over the 1024 partial sums (shuffles inside the wave, LDS across the 16 waves): no floating-point atomics,
// the same bits on every run.  out = {mean, stddev, threshold}.
__global__ __launch_bounds__(FLT_BLK) void k_flt_threshold(const float* stat, int n, double stddev_mul, double* out) {
  __shared__ double red[2][FLT_BLK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0, q = 0.0;
  for (int i = tid; i < n; i += FLT_BLK) {
    const float d = stat[i];
    s += (double)d;
    q += (double)__fmul_rn(d, d);
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64), q += __shfl_down(q, off, 64);
  if (lane == 0) red[0][wave] = s, red[1][wave] = q;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0, sq = 0.0;
    for (int w = 0; w < FLT_BLK / 64; w += 2) sum += red[0][w] + red[0][w + 1], sq += red[1][w] + red[1][w + 1];
    const double dn = (double)n;
    const double mean = sum / dn;
    const double variance = (sq - sum * sum / dn) / (dn - 1.0);
    const double stddev = sqrt(variance);
    out[0] = mean, out[1] = stddev, out[2] = mean + stddev_mul * stddev;
  }
}

}  // namespace apd
