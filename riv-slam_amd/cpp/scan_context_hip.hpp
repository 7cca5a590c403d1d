// radar_graph_slam::SCManagerHip -- SCManager (radar_graph_slam/src/radar_graph_slam/Scancontext.cpp, include/scan_context/Scancontext.h)
// on an MI355X through the C ABI of libapdgicp_hip.so (include/apdgicp_hip.h, apdgicp_scan_context_*; rules S1 .. S8 there).
//
// The descriptors, ring keys, sector keys and column norms of every keyframe live in device memory.  makeAndSaveScancontextAndKeys() adds a
// keyframe's descriptor (ids count from 0, like KeyFrame::index in the reference); detectLoopClosureID() takes the INDICES of the candidate
// keyframes and of the new keyframe, where the reference takes the KeyFrame::Ptr themselves and reads ->index (Scancontext.cpp:278, :292),
// and returns the reference's pair {loop id or -1, yaw difference in radians}.  detectTopK() returns the best k matches for the batched
// verifier (loop_verifier_hip.hpp).  setNumCandidates(0) + setSearchRatio(1.0): every candidate, every shift.
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/point_types.h> and apdgicp_hip.h.  No exceptions: a failed call prints one line on stderr.
#ifndef RADAR_GRAPH_SLAM_SCAN_CONTEXT_HIP_HPP
#define RADAR_GRAPH_SLAM_SCAN_CONTEXT_HIP_HPP

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "apdgicp_hip.h"

namespace radar_graph_slam {

class SCManagerHip {
 public:
  using SCPointType = pcl::PointXYZI;
  using Match = apdgicp_scan_context_match;

  explicit SCManagerHip(int device = 0, void* stream = nullptr) : device_(device), stream_(stream) {
    apdgicp_scan_context_default_params(&params_);
    applied_ = params_;
  }
  ~SCManagerHip() {
    if (h_) apdgicp_scan_context_destroy(h_);
  }
  SCManagerHip(const SCManagerHip&) = delete;
  SCManagerHip& operator=(const SCManagerHip&) = delete;

  void setScDistThresh(double thresh) {  // Scancontext.cpp:64-66
    params_.dist_thresh = thresh;
    push("setScDistThresh");
  }
  void setAzimuthRange(double range) {  // Scancontext.cpp:67-71; only while no descriptor is stored
    params_.azimuth_max = range, params_.azimuth_min = -range;
    push("setAzimuthRange");
  }
  void setNumCandidates(int n) {  // NUM_CANDIDATES_FROM_TREE; 0: all
    params_.num_candidates = n;
    push("setNumCandidates");
  }
  void setSearchRatio(double ratio) {  // SEARCH_RATIO; 1.0: every shift
    params_.search_ratio = ratio;
    push("setSearchRatio");
  }

  // Scancontext.cpp:255-269; returns the descriptor's id, -1 on failure
  int makeAndSaveScancontextAndKeys(const pcl::PointCloud<SCPointType>& scan_down) {
    if (!ready()) return -1;
    static_assert(sizeof(SCPointType) == 32 && offsetof(SCPointType, intensity) == 16, "pcl::PointXYZI layout");
    int32_t id = -1;
    const float* first = scan_down.empty() ? nullptr : &scan_down.points[0].x;
    if (check(apdgicp_scan_context_add(h_, first, (int64_t)scan_down.size(), sizeof(SCPointType), offsetof(SCPointType, intensity), 0, &id), "add")) return -1;
    return id;
  }
  // the same from a cloud that is still on the device (ScanFilterHip's output: 16-byte rows {x, y, z, intensity})
  int makeAndSaveScancontextAndKeys(const float* device_xyzi, int64_t n) {
    if (!ready()) return -1;
    int32_t id = -1;
    if (check(apdgicp_scan_context_add(h_, device_xyzi, n, 16, 12, 1, &id), "add")) return -1;
    return id;
  }
  int size() {
    int32_t n = 0;
    return h_ && !check(apdgicp_scan_context_size(h_, &n), "size") ? n : 0;
  }
  bool clear() { return !h_ || !check(apdgicp_scan_context_clear(h_), "clear"); }

  // Scancontext.cpp:272-379: {loop id or -1, yaw difference [rad]}
  std::pair<int, float> detectLoopClosureID(const std::vector<int>& candidate_indices, int new_index) {
    std::pair<int, float> result{-1, 0.0f};
    Match best;
    int32_t n = 0, loop = -1;
    float yaw = 0.0f;
    if (!ready() || check(apdgicp_scan_context_detect(h_, new_index, ids(candidate_indices), (int32_t)candidate_indices.size(), 1, &best, &n, &loop, &yaw), "detect"))
      return result;
    result.first = loop, result.second = yaw;
    return result;
  }
  // the best k matches, best first; loop_id / yaw_rad as detectLoopClosureID returns them (either may be null)
  std::vector<Match> detectTopK(const std::vector<int>& candidate_indices, int new_index, int k, int* loop_id = nullptr, float* yaw_rad = nullptr) {
    std::vector<Match> out((std::size_t)(k > 0 ? k : 0));
    int32_t n = 0, loop = -1;
    float yaw = 0.0f;
    if (loop_id) *loop_id = -1;
    if (yaw_rad) *yaw_rad = 0.0f;
    if (k < 1 || !ready() ||
        check(apdgicp_scan_context_detect(h_, new_index, ids(candidate_indices), (int32_t)candidate_indices.size(), k, out.data(), &n, &loop, &yaw), "detect")) {
      out.clear();
      return out;
    }
    out.resize((std::size_t)n);
    if (loop_id) *loop_id = loop;
    if (yaw_rad) *yaw_rad = yaw;
    return out;
  }
  apdgicp_scan_context* handle() { return ready() ? h_ : nullptr; }

 private:
  static const int32_t* ids(const std::vector<int>& v) {
    static_assert(sizeof(int) == sizeof(int32_t), "int is 32 bits");
    return v.empty() ? nullptr : reinterpret_cast<const int32_t*>(v.data());
  }
  bool ready() { return h_ || !check(apdgicp_scan_context_create(&params_, device_, stream_, &h_), "create"); }
  void push(const char* what) {  // a refused change (the geometry of a database that is not empty) is taken back
    if (h_ && check(apdgicp_scan_context_set_params(h_, &params_), what)) params_ = applied_;
    else applied_ = params_;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[SCManagerHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  apdgicp_scan_context* h_ = nullptr;
  apdgicp_scan_context_params params_, applied_;
};

}  // namespace radar_graph_slam
#endif
