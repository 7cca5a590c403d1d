// radar_graph_slam::MapCloudGeneratorHip -- MapCloudGenerator::generate (radar_graph_slam/src/radar_graph_slam/map_cloud_generator.cpp:13-53)
// on an MI355X through the C ABI of libapdgicp_hip.so (include/apdgicp_hip.h, apdgicp_map_cloud_*).
//
// The reference takes a vector of KeyFrameSnapshot (cloud + pose) on every call and walks all of it on the CPU.  The clouds never change
// between two calls, so here they are handed over once: addKeyframe() copies a keyframe's cloud to the device and returns its id;
// generate() takes the ids to visit with their current poses (4x4 doubles, column-major: Eigen::Isometry3d::data()) and the resolution,
// and returns what the reference returns -- the occupied voxel centres of its pcl::octree::OctreePointCloud in the octree's depth-first
// order, or, with resolution <= 0, the transformed and gated cloud itself with its intensities.  nullptr where the reference returns
// nullptr (no keyframes) and when a call fails.  The cloud also stays on the device (devicePoints), valid until the next generate():
// what apdgicp_set_target accepts.
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/point_types.h> and apdgicp_hip.h.  No exceptions: a failed call prints one line on stderr.
#ifndef RADAR_GRAPH_SLAM_MAP_CLOUD_GENERATOR_HIP_HPP
#define RADAR_GRAPH_SLAM_MAP_CLOUD_GENERATOR_HIP_HPP

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "apdgicp_hip.h"

namespace radar_graph_slam {

class MapCloudGeneratorHip {
 public:
  using PointT = pcl::PointXYZI;
  using Cloud = pcl::PointCloud<PointT>;
  using Pose = std::array<double, 16>;  // column-major 4x4

  explicit MapCloudGeneratorHip(int device = 0, void* stream = nullptr) : device_(device), stream_(stream) {}
  ~MapCloudGeneratorHip() {
    if (h_) apdgicp_map_cloud_destroy(h_);
  }
  MapCloudGeneratorHip(const MapCloudGeneratorHip&) = delete;
  MapCloudGeneratorHip& operator=(const MapCloudGeneratorHip&) = delete;

  void setLinearChain(bool v) { flags_ = v ? APDGICP_FLAG_XF_LINEAR_CHAIN : 0; }  // Eigen 3.2's summation order of pose * point

  // uploads a keyframe's cloud (an empty one is allowed); the id to pass to generate(), -1 on failure
  int addKeyframe(const Cloud& cloud) {
    if (!ready()) return -1;
    static_assert(sizeof(PointT) == 32 && offsetof(PointT, intensity) == 16, "pcl::PointXYZI layout");
    int32_t id = -1;
    const float* first = cloud.empty() ? nullptr : &cloud.points[0].x;
    if (check(apdgicp_map_cloud_add_keyframe(h_, first, (int64_t)cloud.size(), sizeof(PointT), offsetof(PointT, intensity), 0, &id), "add_keyframe")) return -1;
    n_keyframes_ = id + 1;
    return id;
  }
  bool clear() {
    n_keyframes_ = 0;
    return !h_ || !check(apdgicp_map_cloud_clear(h_), "clear");
  }
  int size() const { return n_keyframes_; }

  // every keyframe, in the order they were added
  Cloud::Ptr generate(const std::vector<Pose>& poses, double resolution) {
    std::vector<int32_t> ids(poses.size());
    for (std::size_t i = 0; i < ids.size(); i++) ids[i] = (int32_t)i;
    return generate(ids, poses, resolution);
  }
  Cloud::Ptr generate(const std::vector<int32_t>& ids, const std::vector<Pose>& poses, double resolution) {
    info_ = apdgicp_map_cloud_stats();
    if (ids.empty() || ids.size() != poses.size()) {
      std::fprintf(stderr, "warning: keyframes empty!!\n");  // map_cloud_generator.cpp:15
      return Cloud::Ptr();
    }
    if (!ready()) return Cloud::Ptr();
    int64_t n = 0;
    if (check(apdgicp_map_cloud_generate(h_, (int32_t)ids.size(), ids.data(), poses[0].data(), resolution, flags_, &n), "generate")) return Cloud::Ptr();
    apdgicp_map_cloud_info(h_, &info_);
    Cloud::Ptr out(new Cloud());
    if (n > 0) {
      std::vector<float> buf((std::size_t)n * 4);
      if (check(apdgicp_map_cloud_copy(h_, buf.data(), n, 0), "copy")) return Cloud::Ptr();
      out->points.resize((std::size_t)n);
      for (int64_t i = 0; i < n; i++) {
        PointT& p = out->points[(std::size_t)i];
        p.x = buf[4 * i], p.y = buf[4 * i + 1], p.z = buf[4 * i + 2], p.intensity = buf[4 * i + 3];
      }
    }
    return out;
  }
  const apdgicp_map_cloud_stats& info() const { return info_; }
  bool devicePoints(const float** xyzi, int64_t* n) { return h_ && !check(apdgicp_map_cloud_points(h_, xyzi, n), "points"); }
  apdgicp_map_cloud* handle() { return ready() ? h_ : nullptr; }

 private:
  bool ready() { return h_ || !check(apdgicp_map_cloud_create(device_, stream_, &h_), "create"); }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[MapCloudGeneratorHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  apdgicp_map_cloud* h_ = nullptr;
  apdgicp_map_cloud_stats info_ = apdgicp_map_cloud_stats();
  int32_t flags_ = 0;
  int n_keyframes_ = 0;
};

}  // namespace radar_graph_slam
#endif
