// Scan Context place recognition on the device: radar_graph_slam::SCManager (radar_graph_slam/src/radar_graph_slam/Scancontext.cpp, "SC:").
// The rules S1 .. S8 and every operation order are in include/apdgicp_hip.h ("Scan Context place recognition").
//
//   k_sc_build   one block per cloud: the R x S bins in LDS, the maximum as an LDS atomicMax on an order-preserving integer image of
//                the float; then S2's keys and norms, one lane per ring / per sector, sequential fp64 sums (SC:162-246)
//   k_sc_ring    one lane per (query, candidate): S4's fp32 d2 against the query's ring key in LDS (SC:322-328)
//   k_sc_rank    rank by counting over (u64, u32) keys, tiles of the segment through LDS; keys are distinct (the low word is a position),
//                so the ranks are a permutation; a block stops as soon as none of its lanes can still rank below `limit`
//   k_sc_dist    one WAVE per (query, kept candidate), lane s = column shift s (S <= 64): S5's S norms, the argmin, then every lane of
//                S6's shift set runs its S x R products sequentially (SC:80-159); query and candidate descriptors in LDS
//   k_sc_emit    the first top_k records in S7's order
// Nothing here assumes 40 x 20: R and S are arguments, LDS is sized by them at launch.
#pragma once

namespace apd {

constexpr int SC_MAX_DIM = 64;  // num_ring, num_sector <= 64: a wave's lanes take the shifts, a block's first / second wave the rings / sectors
constexpr int SC_BLK = 256;
constexpr int SC_MAX_WAVES = 4;  // candidates per k_sc_dist block

struct ScGeom {
  int R, S;
  double max_radius, az_max, az_min;
};
struct ScDb {  // the database: capacity x ...
  float* desc;         // R * S, ring-major
  float* ring_key;     // R
  double* sector_key;  // S
  double* col_norm;    // S
};
struct ScQuery {
  int qid;       // the query's descriptor
  int base;      // where its segment starts in the per-candidate arrays
  int n;         // S3's candidates
  int keep;      // S4: how many are scored
  int m_out;     // S7: min(top_k, keep)
  int out_base;  // where its records start in the output
};
struct ScRec {  // == apdgicp_scan_context_match
  int id, shift;
  double distance;
  float ring_d2;
  int ring_rank;
};

// float -> unsigned, order-preserving (-inf < ... < -0 < +0 < ... < +inf)
__device__ __forceinline__ unsigned sc_image(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sc_unimage(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// double -> u64, order-preserving, every NaN last
__device__ __forceinline__ unsigned long long sc_image64(double d) {
  if (d != d) return ~0ull;
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// S1 + S2 of one cloud into slot `out` (pointers already at the slot).  ready != null: the descriptor is given (R * S floats), S2 only.
// dynamic LDS: (40 + R * S) * 4 bytes
__global__ __launch_bounds__(SC_BLK) void k_sc_build(const float* pts, long long n, int stride /* floats */, int ioff /* < 0: none */, const float* ready,
                                                     ScGeom g, ScDb out) {
  extern __shared__ unsigned sc_lds[];
  float* tab = (float*)sc_lds;
  unsigned* bins = sc_lds + APD_ATAN_TAB_ROWS * APD_ATAN_TAB_STRIDE;
  float* d = (float*)bins;
  const int tid = threadIdx.x, R = g.R, S = g.S, RS = R * S;
  atan_tab_to_lds(tab, tid);
  const unsigned none = sc_image(-1000.f);  // SC:169-170 NO_POINT
  for (int i = tid; i < RS; i += SC_BLK) bins[i] = none;
  __syncthreads();
  if (!ready) {
    for (long long i = tid; i < n; i += SC_BLK) {
      const float* p = pts + i * stride;
      const float x = p[0], y = p[1], in = ioff >= 0 ? p[ioff] : 0.f;
      if (!(isfinite(x) && isfinite(y) && isfinite(in))) continue;                                            // S8
      const float range = sqrtf(x * x + y * y);                                                               // SC:183
      const float angle = (float)(((double)apd_atan2f_tab(x, y, tab) - 1.57079632679489661923) * 180.0 / 3.14159265358979323846);  // SC:185
      if ((double)fabsf(angle) > g.az_max || (double)range > g.max_radius) continue;                          // SC:187-191
      const double fr = ceil(((double)range / g.max_radius) * (double)R);                                     // SC:193
      const double fs = ceil((((double)angle - g.az_min) / (g.az_max - g.az_min)) * (double)S);               // SC:195
      const int ring = (int)fmin(fmax(fr, 1.0), (double)R), sector = (int)fmin(fmax(fs, 1.0), (double)S);     // in 1 .. R, 1 .. S whatever fr, fs are
      if (in > -1000.f) atomicMax(&bins[(ring - 1) * S + (sector - 1)], sc_image(in));                        // SC:201-202
    }
  }
  __syncthreads();
  for (int i = tid; i < RS; i += SC_BLK) {
    float v;
    if (ready) {
      v = ready[i];
    } else {
      v = sc_unimage(bins[i]);
      if (v == -1000.f) v = 0.f;  // SC:206-209
    }
    if (v == 0.f) v = 0.f;  // -0.0 -> +0.0 (S8)
    d[i] = v;               // (bins[i] is this lane's own word)
    out.desc[i] = v;
  }
  __syncthreads();
  if (tid < R) {  // SC:217-230
    double a = 0.0;
    for (int c = 0; c < S; c++) a = a + (double)d[tid * S + c];
    out.ring_key[tid] = (float)(a / (double)S);
  }
  if (tid >= SC_MAX_DIM && tid - SC_MAX_DIM < S) {  // SC:233-246, and the norms of SC:89-92
    const int c = tid - SC_MAX_DIM;
    double m = 0.0, q = 0.0;
    for (int r = 0; r < R; r++) {
      const double v = (double)d[r * S + c];
      m = m + v;
      q = q + v * v;
    }
    out.sector_key[c] = m / (double)R;
    out.col_norm[c] = sqrt(q);
  }
}

// S4: grid (ceil(max n / SC_BLK), queries)
__global__ __launch_bounds__(SC_BLK) void k_sc_ring(const float* ring_key, int R, const ScQuery* qs, const int* cand, unsigned long long* hi, unsigned* lo) {
  __shared__ float qk[SC_MAX_DIM];
  const ScQuery Q = qs[blockIdx.y];
  if ((int)(blockIdx.x * SC_BLK) >= Q.n) return;
  if ((int)threadIdx.x < R) qk[threadIdx.x] = ring_key[(size_t)Q.qid * R + threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * SC_BLK + threadIdx.x;
  if (i >= Q.n) return;
  const float* k = ring_key + (size_t)cand[Q.base + i] * R;
  float d2 = 0.f;
  for (int r = 0; r < R; r++) {
    const float diff = qk[r] - k[r];
    d2 = d2 + diff * diff;
  }
  hi[Q.base + i] = (unsigned long long)__float_as_uint(d2);  // d2 >= 0: its bits order like its value
  lo[Q.base + i] = (unsigned)i;
}

// inv[base + rank] = index, for every element of the segment whose rank by (hi, lo) is below the limit.  stage 0: n candidates, limit
// keep (S4); stage 1: keep scored candidates, limit m_out (S7).  grid (ceil(max segment / SC_BLK), queries)
__global__ __launch_bounds__(SC_BLK) void k_sc_rank(const unsigned long long* hi, const unsigned* lo, const ScQuery* qs, int stage, int* inv) {
  __shared__ unsigned long long s_hi[SC_BLK];
  __shared__ unsigned s_lo[SC_BLK];
  const ScQuery Q = qs[blockIdx.y];
  const int n = stage ? Q.keep : Q.n, limit = stage ? Q.m_out : Q.keep;
  if ((int)(blockIdx.x * SC_BLK) >= n) return;
  const int tid = threadIdx.x, i = blockIdx.x * SC_BLK + tid;
  const bool live = i < n;
  const unsigned long long my_hi = live ? hi[Q.base + i] : 0ull;
  const unsigned my_lo = live ? lo[Q.base + i] : 0u;
  int count = 0;
  for (int t0 = 0; t0 < n; t0 += SC_BLK) {
    const int j = t0 + tid;
    s_hi[tid] = j < n ? hi[Q.base + j] : ~0ull;  // the padding is below no key
    s_lo[tid] = j < n ? lo[Q.base + j] : ~0u;
    __syncthreads();
    for (int t = 0; t < SC_BLK; t++) count += (s_hi[t] < my_hi || (s_hi[t] == my_hi && s_lo[t] < my_lo)) ? 1 : 0;
    if (__syncthreads_and(!live || count >= limit)) break;
  }
  if (live && count < limit) inv[Q.base + count] = i;
}

// bytes of one LDS region of k_sc_dist: a descriptor, its sector key, its column norms, S doubles of scratch
__host__ __device__ inline int sc_region_doubles(int R, int S) { return (R * S + 1) / 2 + 3 * S; }

// S5 + S6 of the kept candidates: grid (ceil(max keep / W), queries), block 64 * W, dynamic LDS (1 + W) regions
__global__ __launch_bounds__(64 * SC_MAX_WAVES) void k_sc_dist(ScDb db, int R, int S, int radius, const ScQuery* qs, const int* cand, const int* inv1,
                                                              const unsigned long long* hi1, ScRec* rec, unsigned long long* hi2, unsigned* lo2) {
  extern __shared__ double sc_dlds[];
  const ScQuery Q = qs[blockIdx.y];
  const int W = blockDim.x >> 6;
  if ((int)(blockIdx.x * W) >= Q.keep) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, RS = R * S, reg = sc_region_doubles(R, S), dd = (RS + 1) / 2;
  const int j = blockIdx.x * W + wave;
  const bool active = j < Q.keep;
  const int pos = active ? inv1[Q.base + j] : 0;
  const int id = active ? cand[Q.base + pos] : Q.qid;
  float* qd = (float*)sc_dlds;
  const double *qv = sc_dlds + dd, *qn = qv + S;
  double* kreg = sc_dlds + (size_t)(1 + wave) * reg;
  float* kd = (float*)kreg;
  double *kv = kreg + dd, *kn = kv + S, *scratch = kn + S;
  for (int i = tid; i < RS; i += blockDim.x) qd[i] = db.desc[(size_t)Q.qid * RS + i];
  for (int i = tid; i < S; i += blockDim.x) {
    sc_dlds[dd + i] = db.sector_key[(size_t)Q.qid * S + i];
    sc_dlds[dd + S + i] = db.col_norm[(size_t)Q.qid * S + i];
  }
  for (int i = lane; i < RS; i += 64) kd[i] = db.desc[(size_t)id * RS + i];
  if (lane < S) {
    kv[lane] = db.sector_key[(size_t)id * S + lane];
    kn[lane] = db.col_norm[(size_t)id * S + lane];
  }
  __syncthreads();
  const int s = lane;
  if (s < S) {  // SC:104-124: the norm of vq - shifted(vk, s)
    double acc = 0.0;
    int cc = s ? S - s : 0;  // (0 - s) mod S
    for (int c = 0; c < S; c++) {
      const double diff = qv[c] - kv[cc];
      acc = acc + diff * diff;
      cc = cc + 1 == S ? 0 : cc + 1;
    }
    scratch[s] = sqrt(acc);
  }
  __syncthreads();
  int a = 0;
  {
    double best = 10000000.0;
    for (int t = 0; t < S; t++) {
      const double v = scratch[t];
      if (v < best) best = v, a = t;
    }
  }
  __syncthreads();
  if (s < S) {  // SC:134-141: is s one of a, (a +- i) mod S, i = 1 .. radius
    const int off = s >= a ? s - a : s - a + S;
    const bool in_set = off == 0 || off <= radius || S - off <= radius;
    double dist = __builtin_inf();
    if (in_set) {  // SC:80-101 against shifted(k, s)
      double sum = 0.0;
      int eff = 0;
      int cc = s ? S - s : 0;
      for (int c = 0; c < S; c++) {
        const double n1 = qn[c], n2 = kn[cc];
        if (!(n1 == 0.0 || n2 == 0.0)) {
          double dot = 0.0;
          for (int r = 0; r < R; r++) dot = dot + (double)qd[r * S + c] * (double)kd[r * S + cc];
          sum = sum + dot / (n1 * n2);
          eff++;
        }
        cc = cc + 1 == S ? 0 : cc + 1;
      }
      dist = 1.0 - sum / (double)eff;
    }
    scratch[s] = dist;  // +inf: not in the set (never below 1e7)
  }
  __syncthreads();
  if (active && lane == 0) {  // SC:144-155
    double best = 10000000.0;
    int arg = 0;
    bool won = false;
    for (int t = 0; t < S; t++) {
      const double v = scratch[t];
      if (v < best) best = v, arg = t, won = true;
    }
    if (!won) best = __builtin_nan(""), arg = 0;
    ScRec r;
    r.id = id, r.shift = arg, r.distance = best;
    r.ring_d2 = __uint_as_float((unsigned)hi1[Q.base + pos]);
    r.ring_rank = j;
    rec[Q.base + j] = r;
    hi2[Q.base + j] = sc_image64(best);
    lo2[Q.base + j] = (unsigned)j;
  }
}

// S7: grid (ceil(max m_out / SC_BLK), queries)
__global__ __launch_bounds__(SC_BLK) void k_sc_emit(const ScQuery* qs, const int* inv2, const ScRec* rec, ScRec* out) {
  const ScQuery Q = qs[blockIdx.y];
  const int f = blockIdx.x * SC_BLK + threadIdx.x;
  if (f < Q.m_out) out[Q.out_base + f] = rec[Q.base + inv2[Q.base + f]];
}

}  // namespace apd
