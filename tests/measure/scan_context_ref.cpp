// Plain single-thread C++ restatement of include/apdgicp_hip.h's Scan Context rules S1 .. S7, the CPU baseline of
// tests/measure/bench_scan_context.py (built by that script: g++ -O3 -ffp-contract=off -shared).  Same operation orders as the device, so
// the records can be compared byte for byte.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "apd_atan2f.h"

namespace {
struct Params {
  int32_t num_ring, num_sector;
  double max_radius, azimuth_max, azimuth_min;
  int32_t num_exclude_recent, num_candidates;
  double search_ratio, dist_thresh;
};
struct Match {
  int32_t id, shift;
  double distance;
  float ring_d2;
  int32_t ring_rank;
};
}  // namespace

extern "C" {

// S1 + S2 of one cloud
void sc_ref_build(const Params* p, const float* pts, int64_t n, int64_t stride_floats, int64_t ioff, float* desc, float* ring_key, double* sector_key, double* col_norm) {
  const int R = p->num_ring, S = p->num_sector;
  for (int i = 0; i < R * S; i++) desc[i] = -1000.f;
  for (int64_t i = 0; i < n; i++) {
    const float *q = pts + i * stride_floats, x = q[0], y = q[1], in = ioff >= 0 ? q[ioff] : 0.f;
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(in))) continue;
    const float range = std::sqrt(x * x + y * y);
    const float angle = (float)(((double)apd::apd_atan2f(x, y) - M_PI_2) * 180.0 / M_PI);
    if ((double)std::fabs(angle) > p->azimuth_max || (double)range > p->max_radius) continue;
    const int ring = std::max(std::min(R, (int)std::ceil(((double)range / p->max_radius) * R)), 1);
    const int sector = std::max(std::min(S, (int)std::ceil((((double)angle - p->azimuth_min) / (p->azimuth_max - p->azimuth_min)) * S)), 1);
    float& d = desc[(ring - 1) * S + sector - 1];
    if (d < in) d = in;
  }
  for (int i = 0; i < R * S; i++)
    if (desc[i] == -1000.f || desc[i] == 0.f) desc[i] = 0.f;
  for (int r = 0; r < R; r++) {
    double a = 0.0;
    for (int c = 0; c < S; c++) a = a + (double)desc[r * S + c];
    ring_key[r] = (float)(a / (double)S);
  }
  for (int c = 0; c < S; c++) {
    double m = 0.0, q = 0.0;
    for (int r = 0; r < R; r++) {
      const double v = (double)desc[r * S + c];
      m = m + v;
      q = q + v * v;
    }
    sector_key[c] = m / (double)R;
    col_norm[c] = std::sqrt(q);
  }
}

// S3 .. S7; returns the number of matches written (at most top_k)
int sc_ref_detect(const Params* p, const float* desc, const float* ring_key, const double* sector_key, const double* col_norm, int32_t query, const int32_t* cand_ids,
                  int32_t n_cand, int32_t top_k, Match* out, int32_t* loop_id, float* yaw) {
  const int R = p->num_ring, S = p->num_sector;
  *loop_id = -1, *yaw = 0.f;
  if (query < p->num_exclude_recent) return 0;
  std::vector<int> cand;
  for (int i = 0; i < n_cand; i++)
    if (query - cand_ids[i] >= p->num_exclude_recent) cand.push_back(cand_ids[i]);
  const int n = (int)cand.size();
  if (!n) return 0;
  std::vector<std::pair<float, int>> key((size_t)n);
  const float* qk = ring_key + (size_t)query * R;
  for (int i = 0; i < n; i++) {
    const float* k = ring_key + (size_t)cand[i] * R;
    float d2 = 0.f;
    for (int r = 0; r < R; r++) {
      const float diff = qk[r] - k[r];
      d2 = d2 + diff * diff;
    }
    key[(size_t)i] = {d2, i};
  }
  const int keep = (p->num_candidates <= 0 || p->num_candidates >= n) ? n : p->num_candidates;
  std::partial_sort(key.begin(), key.begin() + keep, key.end());
  const int radius = (int)std::floor(0.5 * p->search_ratio * S + 0.5);
  const float* qd = desc + (size_t)query * R * S;
  const double *qv = sector_key + (size_t)query * S, *qn = col_norm + (size_t)query * S;
  std::vector<Match> rec((size_t)keep);
  std::vector<char> in_set((size_t)S);
  for (int j = 0; j < keep; j++) {
    const int id = cand[(size_t)key[(size_t)j].second];
    const float* kd = desc + (size_t)id * R * S;
    const double *kv = sector_key + (size_t)id * S, *kn = col_norm + (size_t)id * S;
    int a = 0;
    double best = 10000000.0;
    for (int s = 0; s < S; s++) {
      double acc = 0.0;
      for (int c = 0; c < S; c++) {
        const double diff = qv[c] - kv[((c - s) % S + S) % S];
        acc = acc + diff * diff;
      }
      const double v = std::sqrt(acc);
      if (v < best) best = v, a = s;
    }
    std::fill(in_set.begin(), in_set.end(), 0);
    in_set[(size_t)a] = 1;
    for (int i = 1; i <= radius; i++) in_set[(size_t)(((a + i) % S + S) % S)] = 1, in_set[(size_t)(((a - i) % S + S) % S)] = 1;
    double dmin = 10000000.0;
    int arg = 0;
    bool won = false;
    for (int s = 0; s < S; s++) {
      if (!in_set[(size_t)s]) continue;
      double sum = 0.0;
      int eff = 0;
      for (int c = 0; c < S; c++) {
        const int cc = ((c - s) % S + S) % S;
        const double n1 = qn[c], n2 = kn[cc];
        if (n1 == 0.0 || n2 == 0.0) continue;
        double dot = 0.0;
        for (int r = 0; r < R; r++) dot = dot + (double)qd[r * S + c] * (double)kd[r * S + cc];
        sum = sum + dot / (n1 * n2);
        eff++;
      }
      const double dist = 1.0 - sum / (double)eff;
      if (dist < dmin) dmin = dist, arg = s, won = true;
    }
    Match& m = rec[(size_t)j];
    std::memset(&m, 0, sizeof(m));
    m.id = id, m.shift = won ? arg : 0, m.distance = won ? dmin : std::nan(""), m.ring_d2 = key[(size_t)j].first, m.ring_rank = j;
  }
  std::stable_sort(rec.begin(), rec.end(), [](const Match& x, const Match& y) {
    const bool nx = x.distance != x.distance, ny = y.distance != y.distance;
    if (nx != ny) return ny;
    return !nx && x.distance < y.distance;
  });
  const int m_out = std::min(keep, (int)top_k);
  std::memcpy(out, rec.data(), (size_t)m_out * sizeof(Match));
  if (rec[0].distance < p->dist_thresh) *loop_id = rec[0].id;
  *yaw = (float)((double)(float)(rec[0].shift * ((p->azimuth_max - p->azimuth_min) / (double)S)) * M_PI / 180.0);
  return m_out;
}

}  // extern "C"
