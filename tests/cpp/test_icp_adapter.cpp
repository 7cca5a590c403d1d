// pcl::IterativeClosestPointHip (riv-slam_amd/cpp/icp_hip.hpp) against tests/pcl_shim, created like the ICP branch of
// select_registration_method() (registrations.cpp:71-78) and used through the pcl::Registration base pointer.
//   test_icp_adapter                      compile-and-link check (no GPU needed): prints PCL's defaults as the class holds them
//   test_icp_adapter pair.bin out.bin     pair.bin: int32 n_src, int32 n_tgt, float guess[16] (column-major), src xyz[n_src * 3], tgt xyz[n_tgt * 3].
//                                         Aligns through the class and through the C ABI called directly with the same settings.
//                                         out.bin: the class's apdgicp_result, then the C ABI's, then two doubles: the class's
//                                         getFitnessScore() and the C ABI's fitness score at the final pose.
//                                         Prints "<results byte-equal> <hasConverged> <iterations> <state> <final transformation equals the record>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icp_hip.hpp"

using PointT = pcl::PointXYZI;
using ICP = pcl::IterativeClosestPointHip<PointT, PointT>;

pcl::Registration<PointT, PointT>::Ptr select_registration_method_hip(double eps, int max_iterations, double max_dist, bool reciprocal) {
  ICP::Ptr icp(new ICP());
  icp->setTransformationEpsilon(eps);
  icp->setMaximumIterations(max_iterations);
  icp->setMaxCorrespondenceDistance(max_dist);
  icp->setUseReciprocalCorrespondences(reciprocal);
  return icp;
}

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
    ICP reg;  // (without a GPU: one line on stderr, ok() == false)
    std::printf("compile-only %d %g %d %d\n", reg.maximumIterations(), reg.transformationEpsilon(), reg.maxCorrespondenceDistance() > 1e150 ? 1 : 0,
                reg.icpParams().min_correspondences);
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n[2];
  float guess[16];
  if (std::fread(n, 4, 2, f) != 2 || std::fread(guess, 4, 16, f) != 16) return 2;
  std::vector<float> s(3 * (size_t)n[0]), t(3 * (size_t)n[1]);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 2;
  std::fclose(f);

  auto registration = select_registration_method_hip(1e-8, 6, 2.5, true);
  auto* hip = dynamic_cast<ICP*>(registration.get());
  if (!hip || !hip->ok()) return 3;
  hip->setTransformationRotationEpsilon(2.0);
  hip->setEuclideanFitnessEpsilon(1e-9);
  auto source = make_cloud(s.data(), n[0]);
  auto target = make_cloud(t.data(), n[1]);
  registration->setInputTarget(target);
  registration->setInputSource(source);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  pcl::Registration<PointT, PointT>::Matrix4 g;
  for (int i = 0; i < 16; i++) g.data()[i] = guess[i];
  registration->align(*aligned, g);
  const apdgicp_result r_class = hip->lastResult();
  const auto Tf = registration->getFinalTransformation();
  const int same_T = !std::memcmp(Tf.data(), r_class.T, sizeof(r_class.T));
  const double fit_class = registration->getFitnessScore();
  const int state = hip->convergenceState();

  // the C ABI called directly
  apdgicp_params p;
  apdgicp_default_params(&p);
  p.transformation_epsilon = 1e-8;
  p.max_iterations = 6;
  p.max_correspondence_distance = 2.5;
  apdgicp_icp_params ip;
  apdgicp_icp_default_params(&ip);
  ip.use_reciprocal_correspondences = 1;
  ip.rotation_epsilon = 2.0;
  ip.euclidean_fitness_epsilon = 1e-9;
  apdgicp_handle* h = nullptr;
  apdgicp_result r_abi;
  std::memset(&r_abi, 0, sizeof(r_abi));
  double fit_abi = -1.0;
  int32_t state_abi = -1;
  const int ok = apdgicp_create(&p, 0, nullptr, &h) == 0 && apdgicp_set_icp(h, &ip) == 0 && apdgicp_set_target(h, t.data(), n[1], 12, 0, 0) == 0 &&
                 apdgicp_set_source(h, s.data(), n[0], 12, 0, 0) == 0 && apdgicp_align(h, guess, &r_abi) == 0 &&
                 apdgicp_icp_convergence_state(h, &state_abi) == 0 &&
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
