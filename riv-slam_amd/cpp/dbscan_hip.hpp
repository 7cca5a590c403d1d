// DBSCANClusterHip<PointT> -- DBSCANSimpleCluster<PointT> (radar_graph_slam/include/dbscan/DBSCAN_simple.h) on an MI355X through the C ABI
// of libapdgicp_hip.so (include/apdgicp_hip.h, apdgicp_dbscan_*; the semantics are D1 .. D7 there).
//
// The surface is the reference class's: setInputCloud, setSearchMethod (accepted and ignored: the search is the device grid), the four
// setters, extract(cluster_indices) -- member lists in ascending index, largest cluster first, equal sizes by ascending seed.  Beyond it:
// clusters() is the per-cluster table of the last extract (centre, extent, sizes, Doppler columns), labels() the per-point label, and
// extractDevice() clusters a cloud that is already in device memory, e.g. apdgicp_ego_velocity_outliers' xyzi and Doppler pointers.
//
// Header-only; needs <pcl/point_cloud.h>, <pcl/PointIndices.h>, <pcl/search/kdtree.h> and apdgicp_hip.h.  No exceptions: a failed call prints
// one line on stderr and extract leaves cluster_indices empty.
#ifndef RADAR_GRAPH_SLAM_DBSCAN_HIP_HPP
#define RADAR_GRAPH_SLAM_DBSCAN_HIP_HPP

#include <pcl/PointIndices.h>
#include <pcl/point_cloud.h>
#include <pcl/search/kdtree.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "apdgicp_hip.h"

template <typename PointT>
class DBSCANClusterHip {
 public:
  typedef typename pcl::PointCloud<PointT>::Ptr PointCloudPtr;
  typedef typename pcl::search::KdTree<PointT>::Ptr KdTreePtr;

  explicit DBSCANClusterHip(int device = 0, void* stream = nullptr) : device_(device), stream_(stream) { apdgicp_dbscan_default_params(&prm_); }
  virtual ~DBSCANClusterHip() {
    if (h_) apdgicp_dbscan_destroy(h_);
  }
  DBSCANClusterHip(const DBSCANClusterHip&) = delete;
  DBSCANClusterHip& operator=(const DBSCANClusterHip&) = delete;

  virtual void setInputCloud(PointCloudPtr cloud) { input_cloud_ = cloud; }
  void setSearchMethod(KdTreePtr tree) { search_method_ = tree; }
  void setClusterTolerance(double tolerance) { prm_.eps = tolerance, dirty_ = true; }
  void setMinClusterSize(int min_cluster_size) { prm_.min_cluster_size = min_cluster_size, dirty_ = true; }
  void setMaxClusterSize(int max_cluster_size) { prm_.max_cluster_size = max_cluster_size, dirty_ = true; }
  void setCorePointMinPts(int core_point_min_pts) { prm_.min_pts = core_point_min_pts, dirty_ = true; }

  void extract(std::vector<pcl::PointIndices>& cluster_indices) {
    cluster_indices.clear();
    if (!input_cloud_) return;
    const auto& pts = input_cloud_->points;
    if (!run(pts.empty() ? nullptr : &pts[0].x, (int64_t)pts.size(), (int64_t)sizeof(PointT), nullptr, 0, 0)) return;
    std::vector<int32_t> off((std::size_t)n_clusters_ + 1), idx;
    int64_t m = 0;
    if (check(apdgicp_dbscan_members(h_, off.data(), (int64_t)off.size(), nullptr, 0, &m), "members")) return;
    idx.resize((std::size_t)m);
    if (m && check(apdgicp_dbscan_members(h_, nullptr, 0, idx.data(), m, nullptr), "members")) return;
    cluster_indices.resize((std::size_t)n_clusters_);
    for (int32_t r = 0; r < n_clusters_; r++) {
      pcl::PointIndices& out = cluster_indices[(std::size_t)r];
      out.indices.assign(idx.begin() + off[(std::size_t)r], idx.begin() + off[(std::size_t)r + 1]);
      copy_header(out, *input_cloud_, 0);  // DB:85
    }
  }
  // a cloud in device memory: n points of {x, y, z, .} floats 16 bytes apart, one Doppler float per point beside it (or null)
  bool extractDevice(const float* dev_xyzi, int64_t n, const float* dev_doppler) { return run(dev_xyzi, n, 16, dev_doppler, 4, 1); }

  int32_t clusterCount() const { return n_clusters_; }
  // the table of the last extract, one row per kept cluster in the order of cluster_indices
  std::vector<apdgicp_dbscan_cluster> clusters() {
    std::vector<apdgicp_dbscan_cluster> t((std::size_t)n_clusters_);
    if (n_clusters_ && check(apdgicp_dbscan_clusters(h_, t.data(), n_clusters_), "clusters")) t.clear();
    return t;
  }
  // per point: the position of its cluster in cluster_indices, or -1
  std::vector<int32_t> labels() {
    std::vector<int32_t> l((std::size_t)n_);
    if (n_ && check(apdgicp_dbscan_copy_labels(h_, l.data(), n_), "copy_labels")) l.clear();
    return l;
  }
  apdgicp_dbscan* handle() { return ready() ? h_ : nullptr; }

 protected:
  PointCloudPtr input_cloud_;
  KdTreePtr search_method_;

 private:
  bool run(const float* xyz, int64_t n, int64_t stride, const float* doppler, int64_t dstride, int on_device) {
    n_ = 0, n_clusters_ = 0;
    if (!ready()) return false;
    int32_t K = 0;
    if (check(apdgicp_dbscan_run(h_, xyz, n, stride, doppler, dstride, on_device, &K), "run")) return false;
    n_ = n, n_clusters_ = K;
    return true;
  }
  bool ready() {
    if (h_ && !dirty_) return true;
    const int rc = h_ ? apdgicp_dbscan_set_params(h_, &prm_) : apdgicp_dbscan_create(&prm_, device_, stream_, &h_);
    if (check(rc, h_ ? "set_params" : "create")) return false;
    dirty_ = false;
    return true;
  }
  static bool check(int rc, const char* what) {
    if (rc < 0) std::fprintf(stderr, "[DBSCANClusterHip] %s failed (%d): %s\n", what, rc, apdgicp_last_error());
    return rc < 0;
  }
  template <typename Cloud>
  static auto copy_header(pcl::PointIndices& r, const Cloud& c, int) -> decltype((void)(r.header = c.header)) {
    r.header = c.header;
  }
  template <typename Cloud>
  static void copy_header(pcl::PointIndices&, const Cloud&, long) {}

  int device_;
  void* stream_;
  apdgicp_dbscan* h_ = nullptr;
  apdgicp_dbscan_params prm_;
  bool dirty_ = true;
  int64_t n_ = 0;
  int32_t n_clusters_ = 0;
};

#endif
