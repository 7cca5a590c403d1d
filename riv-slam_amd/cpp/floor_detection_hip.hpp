// radar_graph_slam::FloorDetectionHip -- FloorDetectionNodelet's detect() and under-floor clip
// (radar_graph_slam/apps/floor_detection_nodelet.cpp:88-137, 154-249) on an MI355X through the C ABI of libapdgicp_hip.so
// (include/apdgicp_hip.h, apdgicp_floor_*).
//
// The setters carry the nodelet's parameter names (initialize_params, :62-70); detect() takes the scan cloud_callback receives and
// returns what it publishes: the floor coefficients (`detected` plays boost::optional's part: without a floor `coeffs` holds what
// floor_pub publishes instead, :112-130), floor_points (:222) and /underfloor_filtered_points (:137).  The object remembers prev_coeffs
// like the nodelet does (reset() forgets).  PCL's sampler cannot be reproduced: the three random words per hypothesis come from a
// std::mt19937 that is seeded once (setSeed) and advances from call to call, so a run can be repeated.  Both clouds also stay on the
// device (deviceInliers / deviceUnderFloorFiltered): what apdgicp_scan_filter_run(..., on_device = 1) and apdgicp_set_source accept,
// valid until the next detect().
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/point_types.h> and apdgicp_hip.h.  No exceptions: a failed call prints one line on stderr
// and detect() returns an undetected result with empty clouds.
#ifndef RADAR_GRAPH_SLAM_FLOOR_DETECTION_HIP_HPP
#define RADAR_GRAPH_SLAM_FLOOR_DETECTION_HIP_HPP

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "apdgicp_hip.h"

namespace radar_graph_slam {

class FloorDetectionHip {
 public:
  using PointT = pcl::PointXYZI;
  using Cloud = pcl::PointCloud<PointT>;
  struct Detection {
    bool detected = false;                      // detect() returned coefficients (boost::optional's engaged state)
    std::array<float, 4> coeffs{{0, 0, 1, 0}};  // what floor_pub publishes
    Cloud::Ptr floor_points;                    // :222 (empty without a floor)
    Cloud::Ptr underfloor_filtered;             // :137
  };

  explicit FloorDetectionHip(int device = 0, void* stream = nullptr, uint32_t seed = 0) : device_(device), stream_(stream), rng_(seed) { apdgicp_floor_default_params(&prm_); }
  ~FloorDetectionHip() {
    if (h_) apdgicp_floor_destroy(h_);
  }
  FloorDetectionHip(const FloorDetectionHip&) = delete;
  FloorDetectionHip& operator=(const FloorDetectionHip&) = delete;

  void setTiltDeg(double v) { prm_.tilt_deg = v, dirty_ = true; }                          // "tilt_deg"
  void setSensorHeight(double v) { prm_.sensor_height = v, dirty_ = true; }                // "sensor_height"
  void setHeightClipRange(double v) { prm_.height_clip_range = v, dirty_ = true; }         // "height_clip_range"
  void setFloorPtsThresh(int v) { prm_.floor_pts_thresh = v, dirty_ = true; }              // "floor_pts_thresh"
  void setFloorNormalThresh(double v) { prm_.floor_normal_thresh = v, dirty_ = true; }     // "floor_normal_thresh"
  void setUseNormalFiltering(bool v) { prm_.use_normal_filtering = v ? 1 : 0, dirty_ = true; }  // "use_normal_filtering"
  void setNormalFilterThresh(double v) { prm_.normal_filter_thresh = v, dirty_ = true; }   // "normal_filter_thresh"
  void setFloorTolerance(double v) { prm_.floor_tolerance = v, dirty_ = true; }            // "floor_tolerance"
  void setDistanceThreshold(double v) { prm_.distance_threshold = v, dirty_ = true; }      // ransac.setDistanceThreshold (:185)
  void setHypotheses(int k) { prm_.n_hypotheses = k, dirty_ = true; }                      // 1 .. 1024
  void setSeed(uint32_t seed) { rng_.seed(seed); }
  apdgicp_floor_params& params() {
    dirty_ = true;
    return prm_;
  }
  bool reset() { return ready() && !check(apdgicp_floor_reset(h_), "reset"); }            // :75-80

  Detection detect(const Cloud& cloud) {
    Detection out;
    out.floor_points.reset(new Cloud()), out.underfloor_filtered.reset(new Cloud());
    res_ = apdgicp_floor_result();
    if (!ready() || cloud.empty()) return out;  // :92-94
    static_assert(sizeof(PointT) == 32 && offsetof(PointT, intensity) == 16, "pcl::PointXYZI layout");
    std::vector<uint32_t> words((std::size_t)prm_.n_hypotheses * 3);
    for (uint32_t& w : words) w = (uint32_t)rng_();
    if (check(apdgicp_floor_run(h_, &cloud.points[0].x, (int64_t)cloud.size(), sizeof(PointT), offsetof(PointT, intensity), 0, words.data(), (int64_t)words.size(), &res_), "run"))
      return out;
    out.detected = res_.detected != 0;
    for (int q = 0; q < 4; q++) out.coeffs[(std::size_t)q] = res_.coeffs[q];
    int64_t n_in = 0;
    if (check(apdgicp_floor_inliers(h_, nullptr, nullptr, &n_in), "inliers")) return out;
    fetch(2, n_in, *out.floor_points);
    fetch(3, res_.n_under_floor, *out.underfloor_filtered);
    return out;
  }
  const apdgicp_floor_result& result() const { return res_; }
  bool deviceInliers(const float** xyzi, const int32_t** index, int64_t* n) { return h_ && !check(apdgicp_floor_inliers(h_, xyzi, index, n), "inliers"); }
  bool deviceUnderFloorFiltered(const float** xyzi, const int32_t** index, int64_t* n) {
    return h_ && !check(apdgicp_floor_under_floor_filtered(h_, xyzi, index, n), "under_floor_filtered");
  }
  apdgicp_floor* handle() { return ready() ? h_ : nullptr; }

 private:
  bool fetch(int which, int64_t n, Cloud& out) {
    if (n <= 0) return true;
    std::vector<float> buf((std::size_t)n * 4);
    if (check(apdgicp_floor_copy(h_, which, buf.data(), nullptr, n), "copy")) return false;
    out.points.resize((std::size_t)n);
    for (int64_t i = 0; i < n; i++) {
      PointT& p = out.points[(std::size_t)i];
      p.x = buf[4 * i], p.y = buf[4 * i + 1], p.z = buf[4 * i + 2], p.intensity = buf[4 * i + 3];
    }
    return true;
  }
  bool ready() {
    if (h_ && !dirty_) return true;
    const int rc = h_ ? apdgicp_floor_set_params(h_, &prm_) : apdgicp_floor_create(&prm_, device_, stream_, &h_);
    if (check(rc, h_ ? "set_params" : "create")) return false;
    dirty_ = false;
    return true;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[FloorDetectionHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  std::mt19937 rng_;
  apdgicp_floor* h_ = nullptr;
  apdgicp_floor_params prm_;
  apdgicp_floor_result res_ = apdgicp_floor_result();
  bool dirty_ = true;
};

}  // namespace radar_graph_slam
#endif
