// radar_graph_slam::ScanFilterHip -- the three filters of PreprocessingNodelet::cloud_callback
// (radar_graph_slam/apps/preprocessing_nodelet.cpp:812-815: distance_filter :881-889, downsample :850-866,
// outlier_removal :868-879) on an MI355X through the C ABI of libapdgicp_hip.so (include/apdgicp_hip.h, apdgicp_scan_filter_*).
//
// The setters carry the nodelet's parameter names (initialize_params, :136-206); filter() returns the cloud points_pub would publish
// (:826).  The filtered scan also stays on the device: devicePoints() is what apdgicp_set_source(..., on_device = 1) and
// apdgicp_batch_set_cloud accept, valid until the next filter().
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/point_types.h> and apdgicp_hip.h.  Error convention of the nodelet's filters: no
// exceptions -- a failed call prints one line on stderr and returns an empty cloud.
#ifndef RADAR_GRAPH_SLAM_SCAN_FILTER_HIP_HPP
#define RADAR_GRAPH_SLAM_SCAN_FILTER_HIP_HPP

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "apdgicp_hip.h"

namespace radar_graph_slam {

class ScanFilterHip {
 public:
  using PointT = pcl::PointXYZI;
  using Cloud = pcl::PointCloud<PointT>;

  explicit ScanFilterHip(int device = 0, void* stream = nullptr) : device_(device), stream_(stream) { apdgicp_scan_filter_default_params(&prm_); }
  ~ScanFilterHip() {
    if (h_) apdgicp_scan_filter_destroy(h_);
  }
  ScanFilterHip(const ScanFilterHip&) = delete;
  ScanFilterHip& operator=(const ScanFilterHip&) = delete;

  // "use_distance_filter", "distance_near_thresh", "distance_far_thresh", "z_low_thresh", "z_high_thresh" (:201-205)
  void setUseDistanceFilter(bool on) { prm_.use_distance_filter = on ? 1 : 0, dirty_ = true; }
  void setDistanceNearThresh(double v) { prm_.near = v, dirty_ = true; }
  void setDistanceFarThresh(double v) { prm_.far = v, dirty_ = true; }
  void setZLowThresh(double v) { prm_.z_low = v, dirty_ = true; }
  void setZHighThresh(double v) { prm_.z_high = v, dirty_ = true; }
  // "downsample_method" (VOXELGRID / APPROX_VOXELGRID / NONE; an unknown name falls to NONE with a warning, like :150-156) and
  // "downsample_resolution" (:137-138)
  void setDownsampleMethod(const std::string& m) {
    const bool approx = m == "APPROX_VOXELGRID";
    voxelgrid_ = approx || m == "VOXELGRID";
    prm_.downsample_method = approx ? APDGICP_DOWNSAMPLE_APPROX_VOXELGRID : APDGICP_DOWNSAMPLE_VOXELGRID;
    if (!voxelgrid_ && m != "NONE") std::fprintf(stderr, "[ScanFilterHip] downsample_method %s is not offered: no downsampling\n", m.c_str());
    dirty_ = true;
  }
  void setDownsampleResolution(double r) { resolution_ = (float)r, dirty_ = true; }
  // "outlier_removal_method" (STATISTICAL / RADIUS / anything else: none, :166-191)
  void setOutlierRemovalMethod(const std::string& m) {
    prm_.outlier_method = m == "STATISTICAL" ? APDGICP_OUTLIER_STATISTICAL : m == "RADIUS" ? APDGICP_OUTLIER_RADIUS : APDGICP_OUTLIER_NONE;
    dirty_ = true;
  }
  void setStatisticalMeanK(int k) { prm_.mean_k = k, dirty_ = true; }             // "statistical_mean_k"
  void setStatisticalStddev(double s) { prm_.stddev_mul = s, dirty_ = true; }     // "statistical_stddev"
  void setRadiusRadius(double r) { prm_.radius = r, dirty_ = true; }              // "radius_radius"
  void setRadiusMinNeighbors(int n) { prm_.min_neighbors = n, dirty_ = true; }    // "radius_min_neighbors"

  // distance_filter -> downsample -> outlier_removal (:812-815); the result is the cloud cloud_callback publishes
  Cloud::Ptr filter(const Cloud& cloud) {
    Cloud::Ptr out(new Cloud());
    n_out_ = 0;
    if (!ready()) return out;
    static_assert(sizeof(PointT) == 32 && offsetof(PointT, intensity) == 16, "pcl::PointXYZI layout");
    int64_t n = 0;
    const float* xyz = cloud.empty() ? nullptr : &cloud.points[0].x;
    if (check(apdgicp_scan_filter_run(h_, xyz, (int64_t)cloud.size(), sizeof(PointT), offsetof(PointT, intensity), 0, &n), "run") || n == 0) return out;
    std::vector<float> buf((std::size_t)n * 4);
    if (check(apdgicp_scan_filter_copy(h_, buf.data(), n, 0), "copy")) return out;
    out->points.resize((std::size_t)n);
    for (int64_t i = 0; i < n; i++) {
      PointT& p = out->points[(std::size_t)i];
      p.x = buf[4 * i], p.y = buf[4 * i + 1], p.z = buf[4 * i + 2], p.intensity = buf[4 * i + 3];
    }
    n_out_ = n;
    return out;
  }
  // the filtered scan of the last filter() in device memory: n points of {x, y, z, intensity} floats, 16 bytes apart
  bool devicePoints(const float** device_xyzi, int64_t* n) {
    *device_xyzi = nullptr, *n = 0;
    return h_ && !check(apdgicp_scan_filter_points(h_, device_xyzi, n), "points");
  }
  // sizes of the last filter(): the input, behind distance_filter, behind downsample, the output
  bool stageCounts(int64_t counts[4]) { return h_ && !check(apdgicp_scan_filter_stage_counts(h_, counts), "stage_counts"); }
  apdgicp_scan_filter* handle() { return ready() ? h_ : nullptr; }

 private:
  bool ready() {
    if (h_ && !dirty_) return true;
    for (int a = 0; a < 3; a++) prm_.leaf[a] = voxelgrid_ ? resolution_ : 0.f;
    const int rc = h_ ? apdgicp_scan_filter_set_params(h_, &prm_) : apdgicp_scan_filter_create(&prm_, device_, stream_, &h_);
    if (check(rc, h_ ? "set_params" : "create")) return false;
    dirty_ = false;
    return true;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[ScanFilterHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  apdgicp_scan_filter* h_ = nullptr;
  apdgicp_scan_filter_params prm_;
  bool voxelgrid_ = true, dirty_ = true;
  float resolution_ = 0.1f;
  int64_t n_out_ = 0;
};

}  // namespace radar_graph_slam
#endif
