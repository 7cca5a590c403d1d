// rio::RadarEgoVelocityEstimatorHip -- rio::RadarEgoVelocityEstimator (radar_graph_slam/include/radar_ego_velocity_estimator.h,
// src/radar_ego_velocity_estimator.cpp) on an MI355X through the C ABI of libapdgicp_hip.so (include/apdgicp_hip.h,
// apdgicp_ego_velocity_*): the call PreprocessingNodelet::cloud_callback makes at preprocessing_nodelet.cpp:708-741.
//
// configure() takes anything with the members of RadarEgoVelocityEstimatorConfig, like the reference's (:152-188); estimate() has the
// reference's two shapes, on a cloud of {x, y, z, intensity, doppler} points instead of a sensor_msgs::PointCloud2.  The reference seeds
// its std::mt19937 from std::random_device; here the generator is seeded once (setSeed) and advances from call to call, so a run can
// be repeated.  The inlier / outlier clouds also stay on the device (deviceInliers / deviceOutliers): what apdgicp_scan_filter_run(...,
// on_device = 1) and apdgicp_set_source accept, valid until the next estimate().
//
// Header-only; needs only apdgicp_hip.h.  No exceptions: a failed call prints one line on stderr and estimate() returns false.
#ifndef RIO_RADAR_EGO_VELOCITY_ESTIMATOR_HIP_HPP
#define RIO_RADAR_EGO_VELOCITY_ESTIMATOR_HIP_HPP

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "apdgicp_hip.h"

namespace rio {

struct RadarPointHip {  // rio_utils/radar_point_cloud.h's RadarPointCloudType without its padding
  float x, y, z, intensity, doppler;
};

class RadarEgoVelocityEstimatorHip {
 public:
  using Vector3 = std::array<double, 3>;
  using Cloud = std::vector<RadarPointHip>;

  explicit RadarEgoVelocityEstimatorHip(int device = 0, void* stream = nullptr, uint32_t seed = 0) : device_(device), stream_(stream), rng_(seed) {
    apdgicp_ego_velocity_default_params(&prm_);
  }
  ~RadarEgoVelocityEstimatorHip() {
    if (h_) apdgicp_ego_velocity_destroy(h_);
  }
  RadarEgoVelocityEstimatorHip(const RadarEgoVelocityEstimatorHip&) = delete;
  RadarEgoVelocityEstimatorHip& operator=(const RadarEgoVelocityEstimatorHip&) = delete;

  void setSeed(uint32_t seed) { rng_.seed(seed); }
  void setHypotheses(int k) { prm_.n_hypotheses = k, dirty_ = true; }  // 0: setRansacIter's formula (3 at the defaults), up to 1024
  apdgicp_ego_velocity_params& params() {
    dirty_ = true;
    return prm_;
  }

  template <class Config>
  bool configure(const Config& c) {  // radar_ego_velocity_estimator.h:152-188
    prm_.min_dist = c.min_dist, prm_.max_dist = c.max_dist, prm_.min_db = c.min_db;
    prm_.elevation_thresh_deg = c.elevation_thresh_deg, prm_.azimuth_thresh_deg = c.azimuth_thresh_deg;
    prm_.doppler_velocity_correction_factor = c.doppler_velocity_correction_factor;
    prm_.thresh_zero_velocity = c.thresh_zero_velocity, prm_.allowed_outlier_percentage = c.allowed_outlier_percentage;
    prm_.sigma_zero_velocity_x = c.sigma_zero_velocity_x, prm_.sigma_zero_velocity_y = c.sigma_zero_velocity_y, prm_.sigma_zero_velocity_z = c.sigma_zero_velocity_z;
    prm_.sigma_offset_radar_x = c.sigma_offset_radar_x, prm_.sigma_offset_radar_y = c.sigma_offset_radar_y, prm_.sigma_offset_radar_z = c.sigma_offset_radar_z;
    prm_.max_sigma_x = c.max_sigma_x, prm_.max_sigma_y = c.max_sigma_y, prm_.max_sigma_z = c.max_sigma_z, prm_.max_r_cond = c.max_r_cond;
    prm_.use_cholesky_instead_of_bdcsvd = c.use_cholesky_instead_of_bdcsvd ? 1 : 0, prm_.use_ransac = c.use_ransac ? 1 : 0;
    prm_.outlier_prob = c.outlier_prob, prm_.success_prob = c.success_prob, prm_.N_ransac_points = (int32_t)c.N_ransac_points;
    prm_.inlier_thresh = c.inlier_thresh;
    dirty_ = true;
    return ready();
  }

  bool estimate(const Cloud& scan, Vector3& v_r, Vector3& sigma_v_r) {
    res_ = apdgicp_ego_velocity_result();
    if (!ready()) return false;
    int32_t K = 0;
    if (prm_.use_ransac && check(apdgicp_ego_velocity_hypothesis_count(&prm_, &K), "hypothesis_count")) return false;
    std::vector<uint32_t> words((std::size_t)K * (std::size_t)prm_.N_ransac_points);
    for (uint32_t& w : words) w = (uint32_t)rng_();
    const float* p = scan.empty() ? nullptr : &scan[0].x;
    if (check(apdgicp_ego_velocity_run(h_, p, (int64_t)scan.size(), sizeof(RadarPointHip), offsetof(RadarPointHip, intensity), offsetof(RadarPointHip, doppler), 0,
                                       words.data(), (int64_t)words.size(), &res_), "run"))
      return false;
    for (int q = 0; q < 3; q++) v_r[q] = res_.v[q], sigma_v_r[q] = res_.sigma[q];
    return res_.success != 0;
  }
  bool estimate(const Cloud& scan, Vector3& v_r, Vector3& sigma_v_r, Cloud& inlier_scan, Cloud& outlier_scan) {
    inlier_scan.clear(), outlier_scan.clear();
    const bool ok = estimate(scan, v_r, sigma_v_r);
    return fetch(0, res_.n_inlier, inlier_scan) && fetch(1, res_.n_outlier, outlier_scan) && ok;
  }
  const apdgicp_ego_velocity_result& result() const { return res_; }
  bool deviceInliers(const float** xyzi, const float** doppler, int64_t* n) { return h_ && !check(apdgicp_ego_velocity_inliers(h_, xyzi, doppler, nullptr, n), "inliers"); }
  bool deviceOutliers(const float** xyzi, const float** doppler, int64_t* n) { return h_ && !check(apdgicp_ego_velocity_outliers(h_, xyzi, doppler, nullptr, n), "outliers"); }
  apdgicp_ego_velocity* handle() { return ready() ? h_ : nullptr; }

 private:
  bool fetch(int which, int64_t n, Cloud& out) {
    if (!h_ || n <= 0) return true;
    std::vector<float> xyzi((std::size_t)n * 4), dop((std::size_t)n);
    if (check(apdgicp_ego_velocity_copy(h_, which, xyzi.data(), dop.data(), nullptr, nullptr, n), "copy")) return false;
    out.resize((std::size_t)n);
    for (int64_t i = 0; i < n; i++) out[(std::size_t)i] = RadarPointHip{xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], xyzi[4 * i + 3], dop[(std::size_t)i]};
    return true;
  }
  bool ready() {
    if (h_ && !dirty_) return true;
    const int rc = h_ ? apdgicp_ego_velocity_set_params(h_, &prm_) : apdgicp_ego_velocity_create(&prm_, device_, stream_, &h_);
    if (check(rc, h_ ? "set_params" : "create")) return false;
    dirty_ = false;
    return true;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[RadarEgoVelocityEstimatorHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  std::mt19937 rng_;
  apdgicp_ego_velocity* h_ = nullptr;
  apdgicp_ego_velocity_params prm_;
  apdgicp_ego_velocity_result res_ = apdgicp_ego_velocity_result();
  bool dirty_ = true;
};

}  // namespace rio
#endif
