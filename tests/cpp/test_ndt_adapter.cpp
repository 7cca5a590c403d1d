// fast_gicp::NDTHip (riv-slam_amd/cpp/ndt_hip.hpp) against tests/pcl_shim, created like the NDT branch of select_registration_method()
// (registrations.cpp:101-134) and used through the pcl::Registration base pointer.
//   test_ndt_adapter                      compile-and-link check (no GPU needed)
//   test_ndt_adapter pair.bin out.bin     pair.bin: int32 n_src, int32 n_tgt, float guess[16] (column-major), src xyz[n_src * 3], tgt xyz[n_tgt * 3].
//                                         Aligns through the class (setResolution(2.0), D2D, DIRECT7) and through the C ABI called directly with
//                                         the same settings.  out.bin: the class's apdgicp_result, then the C ABI's.
//                                         Prints "<results byte-equal> <converged> <iterations> <target voxels> <source voxels> <refused settings leave the mode alone>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ndt_hip.hpp"

using PointT = pcl::PointXYZI;
using NDT = fast_gicp::NDTHip<PointT, PointT>;

pcl::Registration<PointT, PointT>::Ptr select_registration_method_hip(double ndt_resolution, fast_gicp::NeighborSearchMethod search) {
  NDT::Ptr ndt(new NDT());
  ndt->setNumThreads(0);
  ndt->setTransformationEpsilon(0.01);
  ndt->setMaximumIterations(64);
  ndt->setResolution(ndt_resolution);
  ndt->setNeighborSearchMethod(search);
  return ndt;
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
    NDT reg;  // (without a GPU: one line on stderr, ok() == false)
    std::printf("compile-only %d %d\n", reg.ndtParams().distance_mode, reg.ndtParams().neighbor_search);
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

  auto registration = select_registration_method_hip(2.0, fast_gicp::NeighborSearchMethod::DIRECT7);
  auto* hip = dynamic_cast<NDT*>(registration.get());
  if (!hip || !hip->ok()) return 3;
  hip->setDistanceMode(fast_gicp::NDTDistanceMode::P2D);
  hip->setDistanceMode(fast_gicp::NDTDistanceMode::D2D);
  // refused settings: the mode keeps the last accepted parameters
  hip->setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT_RADIUS, 1.5);
  hip->setResolution(-1.0);
  const int kept = hip->ndtParams().distance_mode == APDGICP_NDT_D2D && hip->ndtParams().neighbor_search == APDGICP_VGICP_DIRECT7 && hip->ndtParams().resolution == 2.0;
  auto source = make_cloud(s.data(), n[0]);
  auto target = make_cloud(t.data(), n[1]);
  registration->setInputTarget(target);
  registration->setInputSource(source);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  pcl::Registration<PointT, PointT>::Matrix4 g;
  for (int i = 0; i < 16; i++) g.data()[i] = guess[i];
  registration->align(*aligned, g);
  const apdgicp_result r_class = hip->lastResult();
  const long voxels_t = hip->voxelCount(APDGICP_TARGET), voxels_s = hip->voxelCount(APDGICP_SOURCE);
  registration->setInputTarget(target);  // the same pointer: the maps stay
  registration->align(*aligned, g);
  const long builds = hip->buildCount();
  const int again = !std::memcmp(&r_class, &hip->lastResult(), sizeof(r_class)) && builds == 2;

  // the C ABI called directly
  apdgicp_params p;
  apdgicp_default_params(&p);
  p.transformation_epsilon = 0.01;
  p.max_iterations = 64;
  apdgicp_ndt_params np;
  apdgicp_ndt_default_params(&np);
  np.resolution = 2.0;
  apdgicp_handle* h = nullptr;
  apdgicp_result r_abi;
  std::memset(&r_abi, 0, sizeof(r_abi));
  int64_t vt_abi = -1, vs_abi = -1;
  const int ok = apdgicp_create(&p, 0, nullptr, &h) == 0 && apdgicp_set_ndt(h, &np) == 0 && apdgicp_set_target(h, t.data(), n[1], 12, 0, 0) == 0 &&
                 apdgicp_set_source(h, s.data(), n[0], 12, 0, 0) == 0 && apdgicp_align(h, guess, &r_abi) == 0 &&
                 apdgicp_ndt_voxel_count(h, APDGICP_TARGET, &vt_abi) == 0 && apdgicp_ndt_voxel_count(h, APDGICP_SOURCE, &vs_abi) == 0;
  if (h) apdgicp_destroy(h);
  const int equal = ok && again && voxels_t == (long)vt_abi && voxels_s == (long)vs_abi && !std::memcmp(&r_class, &r_abi, sizeof(r_class));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  std::fwrite(&r_class, sizeof(r_class), 1, o);
  std::fwrite(&r_abi, sizeof(r_abi), 1, o);
  std::fclose(o);
  std::printf("%d %d %d %ld %ld %d\n", equal, registration->hasConverged() ? 1 : 0, r_class.iterations, voxels_t, voxels_s, kept);
  return 0;
}
