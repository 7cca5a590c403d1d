// radar_graph_slam::FloorDetectionHip (riv-slam_amd/cpp/floor_detection_hip.hpp) against tests/pcl_shim.
//   test_floor_detection                     compile-and-link check (no GPU needed)
//   test_floor_detection scan.bin out.bin S  int32 n, n x {x, y, z, intensity} floats in; seed S; 32 hypotheses.  out: the 96-byte result
//                                            record, int32 n_floor, the floor points (x 4 floats), int32 n_under, the under-floor-filtered
//                                            cloud (x 4 floats); prints 1 when the device pointer of the under-floor-filtered cloud,
//                                            set as a registration source, holds the same points
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "floor_detection_hip.hpp"

static std::vector<float> flat(const pcl::PointCloud<pcl::PointXYZI>& c) {
  std::vector<float> f(c.size() * 4);
  for (size_t i = 0; i < c.size(); i++) f[4 * i] = c.points[i].x, f[4 * i + 1] = c.points[i].y, f[4 * i + 2] = c.points[i].z, f[4 * i + 3] = c.points[i].intensity;
  return f;
}

int main(int argc, char** argv) {
  radar_graph_slam::FloorDetectionHip det;
  if (argc < 4) {
    std::printf("compile-only\n");
    return 0;
  }
  FILE* in = std::fopen(argv[1], "rb");
  int n = 0;
  if (!in || std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
  std::vector<float> raw((size_t)n * 4);
  if (std::fread(raw.data(), 16, (size_t)n, in) != (size_t)n) return 2;
  std::fclose(in);
  pcl::PointCloud<pcl::PointXYZI> cloud;
  cloud.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    pcl::PointXYZI& p = cloud.points[(size_t)i];
    p.x = raw[4 * i], p.y = raw[4 * i + 1], p.z = raw[4 * i + 2], p.intensity = raw[4 * i + 3];
  }
  det.setSeed((uint32_t)std::atoi(argv[3]));
  det.setHypotheses(32);
  const auto d = det.detect(cloud);
  const apdgicp_floor_result r = det.result();
  const std::vector<float> fp = flat(*d.floor_points), uf = flat(*d.underfloor_filtered);
  const float* dev = nullptr;
  int64_t nd = 0;
  int same = 0;
  if (det.deviceUnderFloorFiltered(&dev, nullptr, &nd) && nd == (int64_t)d.underfloor_filtered->size() && nd > 0) {
    apdgicp_params prm;
    apdgicp_default_params(&prm);
    apdgicp_handle* h = nullptr;
    std::vector<float> back((size_t)nd * 3);
    if (apdgicp_create(&prm, 0, nullptr, &h) == 0 && apdgicp_set_source(h, dev, nd, 16, 1, 0) == 0 && apdgicp_get_points(h, APDGICP_SOURCE, back.data(), nd) == 0) {
      same = 1;
      for (int64_t i = 0; i < nd; i++) same &= !std::memcmp(&back[3 * i], &uf[4 * i], 12);
    }
    if (h) apdgicp_destroy(h);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int n_floor = (int)d.floor_points->size(), n_under = (int)d.underfloor_filtered->size();
  std::fwrite(&r, sizeof(r), 1, o);
  std::fwrite(&n_floor, 4, 1, o);
  std::fwrite(fp.data(), 4, fp.size(), o);
  std::fwrite(&n_under, 4, 1, o);
  std::fwrite(uf.data(), 4, uf.size(), o);
  std::fclose(o);
  std::printf("%d %d %d %d %d\n", r.detected, r.n_filtered, n_floor, n_under, same);
  return 0;
}
