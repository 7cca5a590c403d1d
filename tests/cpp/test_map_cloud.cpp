// radar_graph_slam::MapCloudGeneratorHip (riv-slam_amd/cpp/map_cloud_generator_hip.hpp) against tests/pcl_shim.
//   test_map_cloud                     compile-and-link check (no GPU needed)
//   test_map_cloud in.bin out.bin RES  in: int32 K, then per keyframe int32 n, 16 doubles (the pose, column-major), n x {x, y, z, intensity}
//                                      floats.  Runs the worked example of include/apdgicp_hip.h's M3 in both point orders through the class,
//                                      then the K keyframes at resolution RES through the class AND through the C ABI called directly.
//                                      out: int32 n, n x 4 floats (the class's cloud).  Prints "<worked example ok> <class == C ABI, byte for
//                                      byte> <n> <depth>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "map_cloud_generator_hip.hpp"

using Gen = radar_graph_slam::MapCloudGeneratorHip;
using Cloud = pcl::PointCloud<pcl::PointXYZI>;

static std::vector<float> flat(const Cloud& c) {
  std::vector<float> f(c.size() * 4);
  for (size_t i = 0; i < c.size(); i++) f[4 * i] = c.points[i].x, f[4 * i + 1] = c.points[i].y, f[4 * i + 2] = c.points[i].z, f[4 * i + 3] = c.points[i].intensity;
  return f;
}
static Cloud cloud_of(const std::vector<float>& raw) {
  Cloud c;
  c.resize(raw.size() / 4);
  for (size_t i = 0; i < raw.size() / 4; i++) {
    pcl::PointXYZI& p = c.points[i];
    p.x = raw[4 * i], p.y = raw[4 * i + 1], p.z = raw[4 * i + 2], p.intensity = raw[4 * i + 3];
  }
  return c;
}

// res = 1, identity pose, (0,0,0) then (1.5,0,0): centres (0.5,0.5,0.5), (1.5,0.5,0.5); the other order: min = (-1.5,-3,-3), centres (0,0.5,0.5), (2,0.5,0.5)
static bool worked_example(bool swapped) {
  Gen g;
  const std::vector<float> a = {0.f, 0.f, 0.f, 7.f, 1.5f, 0.f, 0.f, 9.f}, b = {1.5f, 0.f, 0.f, 9.f, 0.f, 0.f, 0.f, 7.f};
  if (g.addKeyframe(cloud_of(swapped ? b : a)) != 0) return false;
  Gen::Pose I{};
  I[0] = I[5] = I[10] = I[15] = 1.0;
  const Cloud::Ptr out = g.generate({I}, 1.0);
  const float want[2][8] = {{0.5f, 0.5f, 0.5f, 0.f, 1.5f, 0.5f, 0.5f, 0.f}, {0.f, 0.5f, 0.5f, 0.f, 2.f, 0.5f, 0.5f, 0.f}};
  const double mn[2][3] = {{-1.0, -3.0, -3.0}, {-1.5, -3.0, -3.0}};
  if (!out || out->size() != 2 || g.info().depth != 2 || std::memcmp(g.info().min, mn[swapped], sizeof(mn[0]))) return false;
  return !std::memcmp(flat(*out).data(), want[swapped], sizeof(want[0]));
}

int main(int argc, char** argv) {
  Gen gen;
  if (argc < 4) {
    std::printf("compile-only\n");
    return 0;
  }
  const int worked = worked_example(false) && worked_example(true);
  FILE* in = std::fopen(argv[1], "rb");
  int K = 0;
  if (!in || std::fread(&K, 4, 1, in) != 1 || K < 1) return 2;
  std::vector<std::vector<float>> raw((size_t)K);
  std::vector<Gen::Pose> poses((size_t)K);
  for (int k = 0; k < K; k++) {
    int n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0 || std::fread(poses[(size_t)k].data(), 8, 16, in) != 16) return 2;
    raw[(size_t)k].resize((size_t)n * 4);
    if (std::fread(raw[(size_t)k].data(), 16, (size_t)n, in) != (size_t)n) return 2;
  }
  std::fclose(in);
  const double res = std::atof(argv[3]);
  for (int k = 0; k < K; k++)
    if (gen.addKeyframe(cloud_of(raw[(size_t)k])) != k) return 3;
  const Cloud::Ptr out = gen.generate(poses, res);
  if (!out) return 3;
  const std::vector<float> got = flat(*out);
  // the C ABI called directly, with the packed {x, y, z, intensity} arrays
  int equal = 0;
  apdgicp_map_cloud* m = nullptr;
  if (apdgicp_map_cloud_create(0, nullptr, &m) == 0) {
    bool ok = true;
    std::vector<int32_t> ids((size_t)K);
    std::vector<double> flat_poses;
    for (int k = 0; k < K && ok; k++) {
      ok = apdgicp_map_cloud_add_keyframe(m, raw[(size_t)k].data(), (int64_t)raw[(size_t)k].size() / 4, 16, 12, 0, &ids[(size_t)k]) == 0 && ids[(size_t)k] == k;
      flat_poses.insert(flat_poses.end(), poses[(size_t)k].begin(), poses[(size_t)k].end());
    }
    int64_t n = 0;
    ok = ok && apdgicp_map_cloud_generate(m, K, ids.data(), flat_poses.data(), res, 0, &n) == 0 && n == (int64_t)out->size();
    std::vector<float> direct((size_t)n * 4);
    ok = ok && (n == 0 || apdgicp_map_cloud_copy(m, direct.data(), n, 0) == 0);
    apdgicp_map_cloud_stats st;
    ok = ok && apdgicp_map_cloud_info(m, &st) == 0 && st.depth == gen.info().depth && !std::memcmp(st.min, gen.info().min, sizeof(st.min));
    equal = ok && (n == 0 || !std::memcmp(direct.data(), got.data(), direct.size() * 4));
    apdgicp_map_cloud_destroy(m);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int n_out = (int)out->size();
  std::fwrite(&n_out, 4, 1, o);
  std::fwrite(got.data(), 4, got.size(), o);
  std::fclose(o);
  std::printf("%d %d %d %d\n", worked, equal, n_out, gen.info().depth);
  return 0;
}
