// fast_gicp::FastVGICPHip (riv-slam_amd/cpp/fast_vgicp_hip.hpp) against tests/pcl_shim, created like the FAST_VGICP branch of
// select_registration_method() (registrations.cpp:62-70) and used through the pcl::Registration base pointer.
//   test_vgicp_adapter                    compile-and-link check (no GPU needed)
//   test_vgicp_adapter pair.bin out.bin   pair.bin: int32 n_src, int32 n_tgt, float guess[16] (column-major), src xyz[n_src * 3], tgt xyz[n_tgt * 3].
//                                         Aligns through the class (setResolution(0.5), DIRECT7, reg_transformation_epsilon 0.1) and through the
//                                         C ABI called directly with the same settings.  out.bin: the class's apdgicp_result, then the C ABI's.
//                                         Prints "<results byte-equal> <converged> <iterations> <voxels> <refused settings leave the mode alone>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fast_vgicp_hip.hpp"

using PointT = pcl::PointXYZI;
using VGICP = fast_gicp::FastVGICPHip<PointT, PointT>;

pcl::Registration<PointT, PointT>::Ptr select_registration_method_hip(double reg_resolution) {
  VGICP::Ptr vgicp(new VGICP());
  vgicp->setNumThreads(0);
  vgicp->setResolution(reg_resolution);
  vgicp->setTransformationEpsilon(0.1);
  vgicp->setMaximumIterations(64);
  vgicp->setCorrespondenceRandomness(20);
  return vgicp;
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
    VGICP reg;  // (without a GPU: one line on stderr, ok() == false)
    std::printf("compile-only %d\n", reg.vgicpParams().neighbor_search);
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

  auto registration = select_registration_method_hip(0.5);
  auto* hip = dynamic_cast<VGICP*>(registration.get());
  if (!hip || !hip->ok()) return 3;
  hip->setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT7);
  // refused settings: the mode keeps the last accepted parameters
  hip->setVoxelAccumulationMode(fast_gicp::VoxelAccumulationMode::MULTIPLICATIVE);
  hip->setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT_RADIUS);
  const int kept = hip->vgicpParams().voxel_mode == APDGICP_VGICP_ADDITIVE && hip->vgicpParams().neighbor_search == APDGICP_VGICP_DIRECT7 &&
                   hip->vgicpParams().resolution == 0.5;
  auto source = make_cloud(s.data(), n[0]);
  auto target = make_cloud(t.data(), n[1]);
  registration->setInputTarget(target);
  registration->setInputSource(source);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  pcl::Registration<PointT, PointT>::Matrix4 g;
  for (int i = 0; i < 16; i++) g.data()[i] = guess[i];
  registration->align(*aligned, g);
  const apdgicp_result r_class = hip->lastResult();
  const long voxels = hip->voxelCount();
  registration->setInputTarget(target);  // the same pointer: the map stays
  registration->align(*aligned, g);
  const int again = !std::memcmp(&r_class, &hip->lastResult(), sizeof(r_class));

  // the C ABI called directly
  apdgicp_params p;
  apdgicp_default_params(&p);
  p.transformation_epsilon = 0.1;
  p.max_iterations = 64;
  p.k_correspondences = 20;
  apdgicp_vgicp_params vp;
  apdgicp_vgicp_default_params(&vp);
  vp.resolution = 0.5;
  vp.neighbor_search = APDGICP_VGICP_DIRECT7;
  apdgicp_handle* h = nullptr;
  apdgicp_result r_abi;
  std::memset(&r_abi, 0, sizeof(r_abi));
  int64_t voxels_abi = -1;
  const int ok = apdgicp_create(&p, 0, nullptr, &h) == 0 && apdgicp_set_vgicp(h, &vp) == 0 && apdgicp_set_target(h, t.data(), n[1], 12, 0, 0) == 0 &&
                 apdgicp_set_source(h, s.data(), n[0], 12, 0, 0) == 0 && apdgicp_align(h, guess, &r_abi) == 0 && apdgicp_vgicp_voxel_count(h, &voxels_abi) == 0;
  if (h) apdgicp_destroy(h);
  const int equal = ok && again && voxels == (long)voxels_abi && !std::memcmp(&r_class, &r_abi, sizeof(r_class));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  std::fwrite(&r_class, sizeof(r_class), 1, o);
  std::fwrite(&r_abi, sizeof(r_abi), 1, o);
  std::fclose(o);
  std::printf("%d %d %d %ld %d\n", equal, registration->hasConverged() ? 1 : 0, r_class.iterations, voxels, kept);
  return 0;
}
