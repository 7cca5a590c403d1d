// radar_graph_slam::ScanIngestHip -- the two ends of PreprocessingNodelet::cloud_callback
// (radar_graph_slam/apps/preprocessing_nodelet.cpp) on an MI355X through the C ABI of libapdgicp_hip.so (include/apdgicp_hip.h,
// apdgicp_scan_ingest_*, I1 .. I7, PI1 .. PI5 and H1 .. H4 there):
//   ingest()  the power gate and the packing of the message's arrays into {x, y, z, intensity, doppler} rows (:667-697; setGate(false):
//             the hugin callback, :497-506), with an optional fixed transform (:477-480);
//   deskew()  deskewing (:914-975) with the IMU message the reference picks from its queue (:939-949), then the transform into the
//             base-link frame (:796-810).
//   runPolar()  the head of cloud_callback_scan (:331-340, PI1 .. PI5): range / azimuth / elevation targets into the same rows;
//   histogramAdd() / histogramLast() / pointDistribution()  the distance histogram that ends all three callbacks (:451-461, H1 .. H4).
// The rows and the deskewed cloud stay on the device: deviceRows() is what apdgicp_ego_velocity_run(handle, rows, n, 32, 12, 16, 1, ...)
// accepts (RadarEgoVelocityEstimatorHip::handle()), deviceDeskewed() what apdgicp_scan_filter_run(handle, xyzi, n, 16, 12, 1, ...)
// accepts (ScanFilterHip::handle()) after synchronize() -- those objects run on streams of their own.
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/point_types.h> and apdgicp_hip.h.  No exceptions: a failed call prints one line on stderr
// and returns false / an empty cloud.
#ifndef RADAR_GRAPH_SLAM_SCAN_INGEST_HIP_HPP
#define RADAR_GRAPH_SLAM_SCAN_INGEST_HIP_HPP

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <utility>
#include <vector>

#include "apdgicp_hip.h"

namespace radar_graph_slam {

class ScanIngestHip {
 public:
  using PointT = pcl::PointXYZI;
  using Cloud = pcl::PointCloud<PointT>;
  struct Imu {  // what deskewing reads of a sensor_msgs::Imu
    double stamp;
    double angular_velocity[3];
  };

  explicit ScanIngestHip(int device = 0, void* stream = nullptr) : device_(device), stream_(stream) { apdgicp_scan_ingest_default_params(&prm_); }
  ~ScanIngestHip() {
    if (h_) apdgicp_scan_ingest_destroy(h_);
  }
  ScanIngestHip(const ScanIngestHip&) = delete;
  ScanIngestHip& operator=(const ScanIngestHip&) = delete;

  void setPowerThreshold(float t) { prm_.power_threshold = t, dirty_ = true; }   // "power_threshold", :107
  void setGate(bool on) { prm_.gate = on ? 1 : 0, dirty_ = true; }
  void setLinearChain(bool on) { prm_.flags = on ? APDGICP_FLAG_XF_LINEAR_CHAIN : 0, dirty_ = true; }
  void setScanPeriod(double s) { scan_period_ = s; }                             // "scan_period", :961

  // imu_callback (:626-633): the queue deskewing reads
  void pushImu(double stamp, double wx, double wy, double wz) { imu_queue_.push_back(Imu{stamp, {wx, wy, wz}}); }
  std::size_t imuQueueSize() const { return imu_queue_.size(); }
  // :939-949 -> (index of the message used, messages erased from the front): the first message with a stamp later than the scan's, or else
  // the last one; everything in front of the pick goes, everything when there is no later message.  An empty queue: (-1, 0).
  static std::pair<int, std::size_t> selectImu(const std::deque<Imu>& q, double scan_stamp) {
    if (q.empty()) return {-1, 0};
    for (std::size_t i = 0; i < q.size(); i++)
      if (q[i].stamp > scan_stamp) return {(int)i, i};
    return {(int)q.size() - 1, q.size()};
  }

  // I1 .. I4 of one message (raw lanes: Point32[] + channels, or the fields of a PointCloud2); returns the number of rows, -1 on failure
  int64_t ingest(const float* xyz, int64_t n, int64_t xyz_stride_bytes, const float* intensity, int64_t intensity_stride_bytes, const float* doppler,
                 int64_t doppler_stride_bytes, bool on_device = false, const float* pre_transform = nullptr) {
    int64_t n_out = 0;
    if (!ready()) return -1;
    if (check(apdgicp_scan_ingest_run(h_, xyz, n, xyz_stride_bytes, intensity, intensity_stride_bytes, doppler, doppler_stride_bytes, on_device ? 1 : 0, pre_transform,
                                      &n_out), "run"))
      return -1;
    return n_out;
  }
  bool deviceRows(const float** rows, const int32_t** index, int64_t* n) { return h_ && !check(apdgicp_scan_ingest_points(h_, rows, index, n), "points"); }
  bool copyRows(std::vector<float>& rows, std::vector<int32_t>& index) {
    int64_t n = 0;
    rows.clear(), index.clear();
    if (!deviceRows(nullptr, nullptr, &n)) return false;
    rows.resize((std::size_t)n * 8), index.resize((std::size_t)n);
    return n == 0 || !check(apdgicp_scan_ingest_copy(h_, rows.data(), index.data(), n), "copy");
  }

  // PI1 .. PI5 of one msgs_radar::RadarScanExtended (cloud_callback_scan, :331-340): every target becomes a row, no gate, no wait.  TargetT is
  // msgs_radar::RadarTargetExtended or any structure with float members range, azimuth, elevation, snr, velocity: the lanes are the member
  // addresses of targets[0], the stride is sizeof(TargetT).  Returns the number of rows (= n), -1 on failure.
  template <class TargetT>
  int64_t runPolar(const TargetT* targets, std::size_t n, bool on_device = false) {
    int64_t n_out = 0;
    if (!ready()) return -1;
    const TargetT* t = targets;  // (the lanes: the member addresses of targets[0]; no target, no lanes)
    const int64_t s = (int64_t)sizeof(TargetT);
    if (check(apdgicp_scan_ingest_run_polar(h_, t ? &t->range : nullptr, s, t ? &t->azimuth : nullptr, s, t ? &t->elevation : nullptr, s, t ? &t->snr : nullptr, s,
                                            t ? &t->velocity : nullptr, s, (int64_t)n, on_device ? 1 : 0, &n_out), "run_polar"))
      return -1;
    return n_out;
  }

  // H1 .. H4: the distance histogram of the filtered cloud (:451-461, :618-628, :818-828) as one more frame; does not wait
  bool histogramAdd(const float* xyz, int64_t n, int64_t stride_bytes, bool on_device) {
    return ready() && !check(apdgicp_scan_ingest_histogram_add(h_, xyz, n, stride_bytes, on_device ? 1 : 0), "histogram_add");
  }
  bool histogramAdd(const Cloud& cloud) {
    static_assert(sizeof(PointT) == 32, "pcl::PointXYZI layout");
    return histogramAdd(cloud.empty() ? nullptr : &cloud.points[0].x, (int64_t)cloud.size(), sizeof(PointT), false);
  }
  // the 100 counts of the last frame (num_at_dist, :454); empty on failure
  std::vector<int32_t> histogramLast() {
    std::vector<int32_t> counts(100, 0);
    if (!ready() || check(apdgicp_scan_ingest_histogram_last(h_, counts.data()), "histogram_last")) counts.clear();
    return counts;
  }
  // the point_distribution command (:1009-1021): the sum of the frames divided by their number, element-wise, as integer division
  // (zeros without a frame); empty on failure
  std::vector<int64_t> pointDistribution() {
    std::vector<int64_t> sum(100, 0);
    int64_t frames = 0;
    if (!ready() || check(apdgicp_scan_ingest_histogram_read(h_, sum.data(), &frames), "histogram_read")) return {};
    for (int64_t& v : sum) v = frames ? v / frames : 0;
    return sum;
  }
  bool histogramReset() { return ready() && !check(apdgicp_scan_ingest_histogram_reset(h_), "histogram_reset"); }

  // I5 .. I7 of a device or host cloud with the IMU message selectImu picks for `scan_stamp` (the queue loses what the reference erases);
  // an empty queue: the cloud passes through.  T: float[16] column-major into the base-link frame, or nullptr.  Does not wait.
  bool deskew(const float* xyz, int64_t n, int64_t stride_bytes, int64_t intensity_offset_bytes, bool on_device, double scan_stamp, const float* T = nullptr) {
    if (!ready()) return false;
    const double* w = nullptr;
    Imu used;
    const std::pair<int, std::size_t> sel = selectImu(imu_queue_, scan_stamp);
    if (sel.first >= 0) {
      used = imu_queue_[(std::size_t)sel.first];
      w = used.angular_velocity;
      imu_queue_.erase(imu_queue_.begin(), imu_queue_.begin() + (std::ptrdiff_t)sel.second);
    }
    return !check(apdgicp_scan_ingest_deskew(h_, xyz, n, stride_bytes, intensity_offset_bytes, on_device ? 1 : 0, w, scan_period_, T), "deskew");
  }
  // the same on a pcl cloud; returns the deskewed (and transformed) cloud
  Cloud::Ptr deskew(const Cloud& cloud, double scan_stamp, const float* T = nullptr) {
    Cloud::Ptr out(new Cloud());
    static_assert(sizeof(PointT) == 32 && offsetof(PointT, intensity) == 16, "pcl::PointXYZI layout");
    if (cloud.empty()) return out;  // (:788-790: the callback returns before deskewing)
    const int64_t n = (int64_t)cloud.size();
    if (!deskew(&cloud.points[0].x, n, sizeof(PointT), offsetof(PointT, intensity), false, scan_stamp, T)) return out;
    std::vector<float> buf((std::size_t)n * 4);
    if (check(apdgicp_scan_ingest_deskewed_copy(h_, buf.data(), n), "deskewed_copy")) return out;
    out->points = cloud.points;
    for (int64_t i = 0; i < n; i++) {
      PointT& p = out->points[(std::size_t)i];
      p.x = buf[4 * i], p.y = buf[4 * i + 1], p.z = buf[4 * i + 2], p.intensity = buf[4 * i + 3];
    }
    return out;
  }
  // the cloud of the last deskew in device memory: n points of {x, y, z, intensity} floats, 16 bytes apart, valid until the next deskew
  bool deviceDeskewed(const float** device_xyzi, int64_t* n) { return h_ && !check(apdgicp_scan_ingest_deskewed(h_, device_xyzi, n), "deskewed"); }
  bool synchronize() { return h_ && !check(apdgicp_scan_ingest_synchronize(h_), "synchronize"); }
  apdgicp_scan_ingest* handle() { return ready() ? h_ : nullptr; }

 private:
  bool ready() {
    if (h_ && !dirty_) return true;
    const int rc = h_ ? apdgicp_scan_ingest_set_params(h_, &prm_) : apdgicp_scan_ingest_create(&prm_, device_, stream_, &h_);
    if (check(rc, h_ ? "set_params" : "create")) return false;
    dirty_ = false;
    return true;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[ScanIngestHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  int device_;
  void* stream_;
  apdgicp_scan_ingest* h_ = nullptr;
  apdgicp_scan_ingest_params prm_;
  std::deque<Imu> imu_queue_;
  double scan_period_ = 0.1;
  bool dirty_ = true;
};

}  // namespace radar_graph_slam
#endif
