// rio::RadarEgoVelocityEstimatorHip (riv-slam_amd/cpp/ego_velocity_hip.hpp) against the C ABI it wraps.
//   test_ego_velocity                     compile-and-link check (no GPU needed)
//   test_ego_velocity scan.bin out.bin S  int32 n, n x {x, y, z, intensity, doppler} floats in; seed S; the inlier cloud (n_in x 5 floats) out;
//                                         prints m, n_inlier, n_outlier and "same" when the class and the C ABI, fed the words of the same
//                                         seeded std::mt19937, give the same record and the same inlier cloud
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ego_velocity_hip.hpp"

int main(int argc, char** argv) {
  rio::RadarEgoVelocityEstimatorHip est;
  if (argc < 4) {
    std::printf("compile-only\n");
    return 0;
  }
  FILE* in = std::fopen(argv[1], "rb");
  int n = 0;
  if (!in || std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
  rio::RadarEgoVelocityEstimatorHip::Cloud scan((size_t)n), inl, outl;
  if (std::fread(scan.data(), sizeof(rio::RadarPointHip), (size_t)n, in) != (size_t)n) return 2;
  std::fclose(in);
  const uint32_t seed = (uint32_t)std::atoi(argv[3]);
  est.setSeed(seed);
  est.setHypotheses(16);
  rio::RadarEgoVelocityEstimatorHip::Vector3 v, sigma;
  if (!est.estimate(scan, v, sigma, inl, outl)) return 3;
  const apdgicp_ego_velocity_result a = est.result();
  // the same through the C ABI
  apdgicp_ego_velocity_params prm;
  apdgicp_ego_velocity_default_params(&prm);
  prm.n_hypotheses = 16;
  apdgicp_ego_velocity* h = nullptr;
  apdgicp_ego_velocity_result b;
  std::mt19937 rng(seed);
  std::vector<uint32_t> words(16 * 5);
  for (uint32_t& w : words) w = (uint32_t)rng();
  if (apdgicp_ego_velocity_create(&prm, 0, nullptr, &h) != 0) return 4;
  if (apdgicp_ego_velocity_run(h, &scan[0].x, n, 20, 12, 16, 0, words.data(), (int64_t)words.size(), &b) != 0) return 4;
  std::vector<float> xyzi((size_t)b.n_inlier * 4), dop((size_t)b.n_inlier);
  if (apdgicp_ego_velocity_copy(h, 0, xyzi.data(), dop.data(), nullptr, nullptr, b.n_inlier) != 0) return 4;
  bool same = !std::memcmp(&a, &b, sizeof(a)) && (size_t)b.n_inlier == inl.size() && (size_t)b.n_outlier == outl.size();
  for (size_t i = 0; same && i < inl.size(); i++) same = !std::memcmp(&inl[i].x, &xyzi[4 * i], 16) && !std::memcmp(&inl[i].doppler, &dop[i], 4);
  apdgicp_ego_velocity_destroy(h);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  std::fwrite(inl.data(), sizeof(rio::RadarPointHip), inl.size(), o);
  std::fclose(o);
  std::printf("%d %d %d %s\n", a.m, a.n_inlier, a.n_outlier, same ? "same" : "DIFFERENT");
  return 0;
}
