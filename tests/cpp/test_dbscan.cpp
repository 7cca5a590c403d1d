// DBSCANClusterHip<pcl::PointXYZI> (riv-slam_amd/cpp/dbscan_hip.hpp) against tests/pcl_shim.
//   test_dbscan                                          compile-and-link check (no GPU needed)
//   test_dbscan cloud.bin out.bin EPS MINPTS MINSZ MAXSZ int32 n, n x {x, y, z, intensity} floats in.  The class clusters 32-byte pcl::PointXYZI,
//                                                        the C ABI called directly the 16-byte rows; out: int32 K, M, labels [n], offsets [K + 1],
//                                                        indices [M], the table [K x 80 bytes] of the class; prints 1 when both paths gave the same bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbscan_hip.hpp"

int main(int argc, char** argv) {
  DBSCANClusterHip<pcl::PointXYZI> db;
  db.setSearchMethod(nullptr);
  if (argc < 7) {
    std::printf("compile-only\n");
    return 0;
  }
  FILE* in = std::fopen(argv[1], "rb");
  int n = 0;
  if (!in || std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
  std::vector<float> raw((size_t)n * 4);
  if (std::fread(raw.data(), 16, (size_t)n, in) != (size_t)n) return 2;
  std::fclose(in);
  const double eps = std::atof(argv[3]);
  const int min_pts = std::atoi(argv[4]), min_sz = std::atoi(argv[5]), max_sz = std::atoi(argv[6]);

  pcl::PointCloud<pcl::PointXYZI>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZI>());
  cloud->resize((size_t)n);
  for (int i = 0; i < n; i++) {
    pcl::PointXYZI& p = cloud->points[(size_t)i];
    p.x = raw[4 * i], p.y = raw[4 * i + 1], p.z = raw[4 * i + 2], p.intensity = raw[4 * i + 3];
  }
  db.setInputCloud(cloud);
  db.setClusterTolerance(eps);
  db.setCorePointMinPts(min_pts);
  db.setMinClusterSize(min_sz);
  db.setMaxClusterSize(max_sz);
  std::vector<pcl::PointIndices> ci;
  db.extract(ci);
  const std::vector<int32_t> labels = db.labels();
  const std::vector<apdgicp_dbscan_cluster> table = db.clusters();
  if ((int64_t)labels.size() != n || table.size() != ci.size()) return 3;
  std::vector<int32_t> off(1, 0), idx;
  for (const pcl::PointIndices& c : ci) {
    idx.insert(idx.end(), c.indices.begin(), c.indices.end());
    off.push_back((int32_t)idx.size());
  }

  // the C ABI on the 16-byte rows
  apdgicp_dbscan_params prm;
  apdgicp_dbscan_default_params(&prm);
  prm.eps = eps, prm.min_pts = min_pts, prm.min_cluster_size = min_sz, prm.max_cluster_size = max_sz;
  apdgicp_dbscan* h = nullptr;
  int32_t K = 0;
  int64_t M = 0;
  int same = 0;
  if (apdgicp_dbscan_create(&prm, 0, nullptr, &h) == 0 && apdgicp_dbscan_run(h, raw.data(), n, 16, nullptr, 0, 0, &K) == 0 && K == (int32_t)ci.size()) {
    std::vector<int32_t> l2((size_t)n), o2((size_t)K + 1), i2;
    std::vector<apdgicp_dbscan_cluster> t2((size_t)K);
    if (apdgicp_dbscan_copy_labels(h, l2.data(), n) == 0 && apdgicp_dbscan_members(h, o2.data(), K + 1, nullptr, 0, &M) == 0) {
      i2.resize((size_t)M);
      if (apdgicp_dbscan_members(h, nullptr, 0, i2.data(), M, nullptr) == 0 && apdgicp_dbscan_clusters(h, t2.data(), K) == 0)
        same = l2 == labels && o2 == off && i2 == idx && (K == 0 || !std::memcmp(t2.data(), table.data(), (size_t)K * sizeof(apdgicp_dbscan_cluster)));
    }
  }
  if (h) apdgicp_dbscan_destroy(h);

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int32_t head[2] = {(int32_t)ci.size(), (int32_t)idx.size()};
  std::fwrite(head, 4, 2, o);
  std::fwrite(labels.data(), 4, labels.size(), o);
  std::fwrite(off.data(), 4, off.size(), o);
  std::fwrite(idx.data(), 4, idx.size(), o);
  std::fwrite(table.data(), sizeof(apdgicp_dbscan_cluster), table.size(), o);
  std::fclose(o);
  std::printf("%d %d\n", same, (int)ci.size());
  return 0;
}
