// radar_graph_slam::SCManagerHip (riv-slam_amd/cpp/scan_context_hip.hpp) against tests/pcl_shim.
//   test_scan_context                          compile-and-link check (no GPU needed)
//   test_scan_context in.bin out.bin NC RATIO  in: int32 K, then per keyframe int32 n, n x {x, y, z, intensity} floats; int32 query, int32 top_k,
//                                              int32 n_cand, n_cand x int32.  The K clouds go through the class (32-byte pcl::PointXYZI) AND
//                                              through the C ABI called directly (16-byte rows), with num_candidates NC and search_ratio RATIO;
//                                              both detect.  out: int32 n, n x apdgicp_scan_context_match (the class's), int32 loop id, float yaw
//                                              (detectLoopClosureID's pair).  Prints "<class == C ABI, byte for byte> <n> <loop id>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scan_context_hip.hpp"

using SC = radar_graph_slam::SCManagerHip;
using Cloud = pcl::PointCloud<pcl::PointXYZI>;

static Cloud cloud_of(const std::vector<float>& raw) {
  Cloud c;
  c.resize(raw.size() / 4);
  for (size_t i = 0; i < raw.size() / 4; i++) {
    pcl::PointXYZI& p = c.points[i];
    p.x = raw[4 * i], p.y = raw[4 * i + 1], p.z = raw[4 * i + 2], p.intensity = raw[4 * i + 3];
  }
  return c;
}

int main(int argc, char** argv) {
  SC sc;
  sc.setScDistThresh(0.5);
  sc.setAzimuthRange(56.5);
  if (argc < 5) {
    std::printf("compile-only\n");
    return 0;
  }
  const int nc = std::atoi(argv[3]);
  const double ratio = std::atof(argv[4]);
  sc.setNumCandidates(nc);
  sc.setSearchRatio(ratio);
  FILE* in = std::fopen(argv[1], "rb");
  int K = 0;
  if (!in || std::fread(&K, 4, 1, in) != 1 || K < 1) return 2;
  std::vector<std::vector<float>> raw((size_t)K);
  for (int k = 0; k < K; k++) {
    int n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
    raw[(size_t)k].resize((size_t)n * 4);
    if (std::fread(raw[(size_t)k].data(), 16, (size_t)n, in) != (size_t)n) return 2;
  }
  int query = 0, top_k = 0, n_cand = 0;
  if (std::fread(&query, 4, 1, in) != 1 || std::fread(&top_k, 4, 1, in) != 1 || std::fread(&n_cand, 4, 1, in) != 1 || n_cand < 0 || top_k < 1) return 2;
  std::vector<int> cand((size_t)n_cand);
  if (n_cand && std::fread(cand.data(), 4, (size_t)n_cand, in) != (size_t)n_cand) return 2;
  std::fclose(in);
  for (int k = 0; k < K; k++)
    if (sc.makeAndSaveScancontextAndKeys(cloud_of(raw[(size_t)k])) != k) return 3;
  if (sc.size() != K) return 3;
  int loop_k = -2;
  float yaw_k = -1.f;
  const std::vector<SC::Match> got = sc.detectTopK(cand, query, top_k, &loop_k, &yaw_k);
  const std::pair<int, float> pair = sc.detectLoopClosureID(cand, query);
  // the C ABI called directly, with the packed {x, y, z, intensity} rows
  int equal = 0;
  apdgicp_scan_context* h = nullptr;
  apdgicp_scan_context_params p;
  apdgicp_scan_context_default_params(&p);
  p.num_candidates = nc, p.search_ratio = ratio;
  if (apdgicp_scan_context_create(&p, 0, nullptr, &h) == 0) {
    bool ok = true;
    for (int k = 0; k < K && ok; k++) {
      int32_t id = -1;
      ok = apdgicp_scan_context_add(h, raw[(size_t)k].data(), (int64_t)raw[(size_t)k].size() / 4, 16, 12, 0, &id) == 0 && id == k;
    }
    std::vector<SC::Match> direct((size_t)top_k);
    int32_t n = 0, loop = -2;
    float yaw = -1.f;
    ok = ok && apdgicp_scan_context_detect(h, query, cand.data(), n_cand, top_k, direct.data(), &n, &loop, &yaw) == 0 && n == (int32_t)got.size();
    ok = ok && loop == loop_k && loop == pair.first && !std::memcmp(&yaw, &yaw_k, 4) && !std::memcmp(&yaw, &pair.second, 4);
    ok = ok && (n == 0 || !std::memcmp(direct.data(), got.data(), (size_t)n * sizeof(SC::Match)));
    // the descriptors themselves
    const size_t RS = (size_t)p.num_ring * p.num_sector;
    std::vector<float> da(RS * K), db(RS * K);
    ok = ok && apdgicp_scan_context_descriptors(h, 0, K, da.data(), nullptr, nullptr, nullptr) == 0 &&
         apdgicp_scan_context_descriptors(sc.handle(), 0, K, db.data(), nullptr, nullptr, nullptr) == 0 && !std::memcmp(da.data(), db.data(), RS * K * 4);
    equal = ok;
    apdgicp_scan_context_destroy(h);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int n_out = (int)got.size();
  std::fwrite(&n_out, 4, 1, o);
  std::fwrite(got.data(), sizeof(SC::Match), got.size(), o);
  std::fwrite(&pair.first, 4, 1, o);
  std::fwrite(&pair.second, 4, 1, o);
  std::fclose(o);
  std::printf("%d %d %d\n", equal, n_out, pair.first);
  return 0;
}
