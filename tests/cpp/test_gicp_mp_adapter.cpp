// fast_gicp::FastGICPMultiPointsHip (riv-slam_amd/cpp/fast_gicp_mp_hip.hpp) against tests/pcl_shim, used through the pcl::Registration base pointer.
//   test_gicp_mp_adapter                      compile-and-link check (no GPU needed): prints MP8's defaults as the class holds them
//   test_gicp_mp_adapter pair.bin out.bin     pair.bin: int32 n_src, int32 n_tgt, float guess[16] (column-major), double radius, src xyz[n_src * 3], tgt xyz[n_tgt * 3].
//                                             Aligns through the class and through the C ABI called directly with the same settings.
//                                             out.bin: the class's apdgicp_result, then the C ABI's, then two doubles: the class's
//                                             getFitnessScore() and the C ABI's fitness score at the final pose.
//                                             Prints "<results byte-equal> <hasConverged> <iterations> <state> <final transformation equals the record>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "fast_gicp_mp_hip.hpp"

using PointT = pcl::PointXYZI;
using MP = fast_gicp::FastGICPMultiPointsHip<PointT, PointT>;

static pcl::PointCloud<PointT>::Ptr make_cloud(const float* xyz, int n) {
  pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
  c->resize(n);
  for (int i = 0; i < n; i++) {
    c->at(i).x = xyz[3 * i], c->at(i).y = xyz[3 * i + 1], c->at(i).z = xyz[3 * i + 2];
    c->at(i).intensity = 42.f;
  }
  return c;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    MP reg;  // (without a GPU: one line on stderr, ok() == false)
    std::printf("compile-only %d %d %g %g %d %g\n", reg.correspondenceRandomness(), reg.maximumIterations(), reg.rotationEpsilon(), reg.transformationEpsilon(),
                (int)reg.regularizationMethod(), reg.gicpMpParams().neighbor_search_radius);
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n[2];
  float guess[16];
  double radius = 0.0;
  if (std::fread(n, 4, 2, f) != 2 || std::fread(guess, 4, 16, f) != 16 || std::fread(&radius, 8, 1, f) != 1) return 2;
  std::vector<float> s(3 * (size_t)n[0]), t(3 * (size_t)n[1]);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 2;
  std::fclose(f);

  MP::Ptr mp(new MP());
  pcl::Registration<PointT, PointT>::Ptr registration = mp;
  if (!mp->ok()) return 3;
  mp->setNeighborSearchRadius(radius);
  auto source = make_cloud(s.data(), n[0]);
  auto target = make_cloud(t.data(), n[1]);
  registration->setInputTarget(target);
  registration->setInputSource(source);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  pcl::Registration<PointT, PointT>::Matrix4 g;
  for (int i = 0; i < 16; i++) g.data()[i] = guess[i];
  registration->align(*aligned, g);
  const apdgicp_result r_class = mp->lastResult();
  const auto Tf = registration->getFinalTransformation();
  const int same_T = !std::memcmp(Tf.data(), r_class.T, sizeof(r_class.T));
  const double fit_class = registration->getFitnessScore();
  const int state = mp->convergenceState();

  // the C ABI called directly, with MP8's defaults
  apdgicp_params p;
  apdgicp_default_params(&p);
  p.k_correspondences = 20;
  p.max_iterations = 64;
  p.rotation_epsilon = 1e-5;
  p.transformation_epsilon = 1e-5;
  p.regularization = APDGICP_REG_PLANE;
  apdgicp_gicp_mp_params mpp;
  apdgicp_gicp_mp_default_params(&mpp);
  mpp.neighbor_search_radius = radius;
  apdgicp_handle* h = nullptr;
  apdgicp_result r_abi;
  std::memset(&r_abi, 0, sizeof(r_abi));
  double fit_abi = -1.0;
  int32_t state_abi = -1;
  const int ok = apdgicp_create(&p, 0, nullptr, &h) == 0 && apdgicp_set_gicp_mp(h, &mpp) == 0 && apdgicp_set_target(h, t.data(), n[1], 12, 0, 0) == 0 &&
                 apdgicp_set_source(h, s.data(), n[0], 12, 0, 0) == 0 && apdgicp_align(h, guess, &r_abi) == 0 && apdgicp_gicp_mp_state(h, &state_abi) == 0 &&
                 apdgicp_fitness_score(h, r_abi.T, std::numeric_limits<double>::max(), &fit_abi, nullptr) == 0;
  if (h) apdgicp_destroy(h);
  const int equal = ok && state == (int)state_abi && !std::memcmp(&r_class, &r_abi, sizeof(r_class));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  std::fwrite(&r_class, sizeof(r_class), 1, o);
  std::fwrite(&r_abi, sizeof(r_abi), 1, o);
  std::fwrite(&fit_class, sizeof(double), 1, o);
  std::fwrite(&fit_abi, sizeof(double), 1, o);
  std::fclose(o);
  std::printf("%d %d %d %d %d\n", equal, registration->hasConverged() ? 1 : 0, r_class.iterations, state, same_T);
  return 0;
}
