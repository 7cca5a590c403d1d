// The search object of fast_gicp::FastAPDGICPHip beyond k = 1: the batch form of nearestKSearch with k = 5 (one device pass,
// apdgicp_knn_of) against the per-query host scan (host_nn, reached through the single-point call) and against a scan written here,
// and deviceRadiusSearch (apdgicp_radius_search_of / _rows) against a host scan.
// usage: test_search_adapter <pair.bin> [compile-only check when no file is given]
//   pair.bin: int32 n_src, int32 n_tgt, float guess[16] (column-major), src xyz[n_src*3], tgt xyz[n_tgt*3]
// prints one JSON object
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "fast_apdgicp_hip.hpp"

using PointT = pcl::PointXYZI;
using Reg = fast_gicp::FastAPDGICPHip<PointT, PointT>;

static pcl::PointCloud<PointT>::Ptr make_cloud(const float* xyz, int n) {
  pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
  c->resize(n);
  for (int i = 0; i < n; i++) c->at(i).x = xyz[3 * i], c->at(i).y = xyz[3 * i + 1], c->at(i).z = xyz[3 * i + 2], c->at(i).intensity = 1.f;
  return c;
}

// every (distance, index) of the target for q, ascending: FLANN's L2_Simple arithmetic in fp32, ties by index
static std::vector<std::pair<float, int>> scan(const PointT& q, const float* t, int nt) {
  std::vector<std::pair<float, int>> all(nt);
  for (int j = 0; j < nt; j++) {
    const float dx = q.x - t[3 * j], dy = q.y - t[3 * j + 1], dz = q.z - t[3 * j + 2];
    float d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    all[j] = std::make_pair(d, j);
  }
  std::sort(all.begin(), all.end());
  return all;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("compile-only\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n[2];
  float guess[16];
  if (std::fread(n, 4, 2, f) != 2 || std::fread(guess, 4, 16, f) != 16) return 2;
  std::vector<float> s(3 * n[0]), t(3 * n[1]);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 2;
  std::fclose(f);
  const int nt = n[1];

  Reg::Ptr apdgicp(new Reg());
  apdgicp->setTransformationEpsilon(0.1);
  apdgicp->setMaxCorrespondenceDistance(2.0);
  apdgicp->setAzimuthVar(1.0);
  pcl::Registration<PointT, PointT>::Ptr registration = apdgicp;
  Reg& reg = *apdgicp;
  pcl::PointCloud<PointT>::ConstPtr target = make_cloud(t.data(), nt), source = make_cloud(s.data(), n[0]);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  pcl::Registration<PointT, PointT>::Matrix4 g;
  for (int i = 0; i < 16; i++) g.data()[i] = guess[i];
  registration->setInputSource(source), registration->setInputTarget(target);
  registration->align(*aligned, g);
  const int conv0 = registration->hasConverged() ? 1 : 0, lin0 = reg.lastResult().n_linearize;

  // 300 queries that are no transformed source points: near target points, some of them ON target points (distance 0, ties with nothing)
  const int nq = 300;
  pcl::PointCloud<PointT> queries;
  queries.resize(nq);
  for (int i = 0; i < nq; i++) {
    const int j = (i * 53) % nt;
    const float e = i % 4 == 0 ? 0.f : 1.f;
    queries.at(i).x = t[3 * j] + e * 0.013f * (float)(i % 7 - 3), queries.at(i).y = t[3 * j + 1] - e * 0.019f * (float)(i % 5 - 2), queries.at(i).z = t[3 * j + 2] + e * 0.004f * (float)(i % 3);
  }

  // ---- batch k = 5: one device pass, no fall-back
  const int k = 5;
  std::vector<std::vector<int>> bi;
  std::vector<std::vector<float>> bd;
  const long fb0 = reg.deviceSearchStats().fallbacks, dq0 = reg.deviceSearchStats().device_queries;
  registration->getSearchMethodTarget()->nearestKSearch(queries, std::vector<int>(), k, bi, bd);
  const long knn_fallbacks = reg.deviceSearchStats().fallbacks - fb0, knn_device_queries = reg.deviceSearchStats().device_queries - dq0;
  int knn_vs_scan = bi.size() == (size_t)nq && bd.size() == (size_t)nq ? 1 : 0;
  for (int i = 0; i < nq && knn_vs_scan; i++) {
    const auto all = scan(queries.at(i), t.data(), nt);
    knn_vs_scan = bi[i].size() == (size_t)k && bd[i].size() == (size_t)k;
    for (int r = 0; r < k && knn_vs_scan; r++) knn_vs_scan = bi[i][r] == all[r].second && bd[i][r] == all[r].first;
  }
  // an index subset
  std::vector<int> sub = {7, 0, 299, 150};
  std::vector<std::vector<int>> si;
  std::vector<std::vector<float>> sd;
  registration->getSearchMethodTarget()->nearestKSearch(queries, sub, k, si, sd);
  int sub_ok = si.size() == sub.size() ? 1 : 0;
  for (size_t i = 0; i < sub.size() && sub_ok; i++) sub_ok = si[i] == bi[sub[i]] && sd[i] == bd[sub[i]];
  const long fb1 = reg.deviceSearchStats().fallbacks;
  // ... and row for row what the per-query host scan (host_nn, behind the single-point call with k > 1) answers
  int knn_vs_host_nn = 1;
  for (int i = 0; i < nq && knn_vs_host_nn; i++) {
    std::vector<int> pi;
    std::vector<float> pd;
    const int got = registration->getSearchMethodTarget()->nearestKSearch(queries.at(i), k, pi, pd);
    knn_vs_host_nn = got == k && pi == bi[i] && pd == bd[i];
  }
  const long single_fallbacks = reg.deviceSearchStats().fallbacks - fb1;

  // ---- deviceRadiusSearch against the host scan: strict `<` on (float)(radius * radius), ascending (distance, index), max_nn
  int radius_ok = 1, radius_rows_nonempty = 0, radius_rows_cut = 0;
  const double radii[2] = {0.0, 0.6};
  const unsigned caps[3] = {0, 3, 100000};
  for (double radius : radii)
    for (unsigned cap : caps) {
      std::vector<std::vector<int>> ri;
      std::vector<std::vector<float>> rd;
      const bool ok = reg.deviceRadiusSearch(queries, std::vector<int>(), radius, ri, rd, cap);
      radius_ok = radius_ok && ok && ri.size() == (size_t)nq && rd.size() == (size_t)nq;
      const float r2 = (float)(radius * radius);
      for (int i = 0; i < nq && radius_ok; i++) {
        const auto all = scan(queries.at(i), t.data(), nt);
        std::vector<int> wi;
        std::vector<float> wd;
        for (const auto& a : all)
          if (a.first < r2 && !(cap > 0 && cap < (unsigned)nt && wi.size() >= cap)) wi.push_back(a.second), wd.push_back(a.first);
        radius_ok = ri[i] == wi && rd[i] == wd;
        radius_rows_nonempty += wi.empty() ? 0 : 1;
        radius_rows_cut += (cap == 3 && wi.size() == 3) ? 1 : 0;
      }
    }
  const long radius_fallbacks = reg.deviceSearchStats().fallbacks - fb1 - single_fallbacks;

  // the handle still registers afterwards
  registration->align(*aligned, g);
  const int conv1 = registration->hasConverged() ? 1 : 0, lin1 = reg.lastResult().n_linearize;
  std::printf("{\"converged\": %d, \"knn_vs_scan\": %d, \"knn_vs_host_nn\": %d, \"sub_ok\": %d, \"knn_fallbacks\": %ld, \"knn_device_queries\": %ld, "
              "\"single_fallbacks\": %ld, \"radius_ok\": %d, \"radius_rows_nonempty\": %d, \"radius_rows_cut\": %d, \"radius_fallbacks\": %ld, "
              "\"converged_after\": %d, \"same_iterations\": %d, \"n_queries\": %d}\n",
              conv0, knn_vs_scan, knn_vs_host_nn, sub_ok, knn_fallbacks, knn_device_queries, single_fallbacks, radius_ok, radius_rows_nonempty, radius_rows_cut,
              radius_fallbacks, conv1, lin0 == lin1 ? 1 : 0, nq);
  return 0;
}
