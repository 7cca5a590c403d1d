// radar_graph_slam::ScanIngestHip (riv-slam_amd/cpp/scan_ingest_hip.hpp) against tests/pcl_shim.
//   test_scan_ingest                     compile-and-link check (no GPU needed)
//   test_scan_ingest scan.bin out.bin    in: int32 n, int32 q, double scan_stamp, double scan_period, float power_threshold, float T[16] column-major,
//                                        n x {x, y, z, power, doppler} floats, q x {stamp, wx, wy, wz} doubles.  The class ingests the 20-byte
//                                        records, deskews the rows as 32-byte pcl::PointXYZI points with its IMU queue and transforms them by T;
//                                        the C ABI called directly does the same on the device rows with the message selectImu names.
//                                        out: int32 n_out, int32 imu index, int32 queue size behind the call, rows [n_out x 8], index [n_out],
//                                        deskewed [n_out x 4] of the class; prints 1 when both paths gave the same bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scan_ingest_hip.hpp"

using radar_graph_slam::ScanIngestHip;

int main(int argc, char** argv) {
  ScanIngestHip ing;
  ing.setPowerThreshold(0.f);
  ing.setScanPeriod(0.1);
  if (argc < 3) {
    std::deque<ScanIngestHip::Imu> q;
    q.push_back(ScanIngestHip::Imu{1.0, {0, 0, 0}});
    q.push_back(ScanIngestHip::Imu{2.0, {0, 0, 0}});
    const bool ok = ScanIngestHip::selectImu(q, 1.0).first == 1 && ScanIngestHip::selectImu(q, 2.0).second == 2 && ing.imuQueueSize() == 0;
    std::printf(ok ? "compile-only\n" : "selectImu is wrong\n");
    return ok ? 0 : 1;
  }
  FILE* in = std::fopen(argv[1], "rb");
  int32_t n = 0, q = 0;
  double stamp = 0, period = 0;
  float thr = 0, T[16];
  if (!in || std::fread(&n, 4, 1, in) != 1 || std::fread(&q, 4, 1, in) != 1 || std::fread(&stamp, 8, 1, in) != 1 || std::fread(&period, 8, 1, in) != 1 ||
      std::fread(&thr, 4, 1, in) != 1 || std::fread(T, 4, 16, in) != 16 || n < 0 || q < 0)
    return 2;
  std::vector<float> raw((size_t)n * 5);
  std::vector<double> imu((size_t)q * 4);
  if (std::fread(raw.data(), 20, (size_t)n, in) != (size_t)n || std::fread(imu.data(), 32, (size_t)q, in) != (size_t)q) return 2;
  std::fclose(in);

  // the class
  ing.setPowerThreshold(thr);
  ing.setScanPeriod(period);
  std::deque<ScanIngestHip::Imu> queue;
  for (int k = 0; k < q; k++) {
    ing.pushImu(imu[4 * k], imu[4 * k + 1], imu[4 * k + 2], imu[4 * k + 3]);
    queue.push_back(ScanIngestHip::Imu{imu[4 * k], {imu[4 * k + 1], imu[4 * k + 2], imu[4 * k + 3]}});
  }
  const int64_t n_out = ing.ingest(raw.data(), n, 20, raw.data() + 3, 20, raw.data() + 4, 20);
  std::vector<float> rows;
  std::vector<int32_t> index;
  if (n_out < 0 || !ing.copyRows(rows, index) || (int64_t)index.size() != n_out) return 3;
  ScanIngestHip::Cloud cloud;
  cloud.resize((size_t)n_out);
  for (int64_t i = 0; i < n_out; i++) {
    pcl::PointXYZI& p = cloud.points[(size_t)i];
    p.x = rows[8 * i], p.y = rows[8 * i + 1], p.z = rows[8 * i + 2], p.intensity = rows[8 * i + 3];
  }
  const ScanIngestHip::Cloud::Ptr desk = ing.deskew(cloud, stamp, T);
  if ((int64_t)desk->size() != n_out) return 3;
  std::vector<float> dk((size_t)n_out * 4);
  for (int64_t i = 0; i < n_out; i++) {
    const pcl::PointXYZI& p = desk->points[(size_t)i];
    dk[4 * i] = p.x, dk[4 * i + 1] = p.y, dk[4 * i + 2] = p.z, dk[4 * i + 3] = p.intensity;
  }

  // the C ABI, the deskew on its own device rows
  const std::pair<int, std::size_t> sel = ScanIngestHip::selectImu(queue, stamp);
  apdgicp_scan_ingest_params prm;
  apdgicp_scan_ingest_default_params(&prm);
  prm.power_threshold = thr;
  apdgicp_scan_ingest* h = nullptr;
  int same = 0;
  int64_t n2 = 0, n3 = 0;
  const float* d_rows = nullptr;
  if (apdgicp_scan_ingest_create(&prm, 0, nullptr, &h) == 0 &&
      apdgicp_scan_ingest_run(h, raw.data(), n, 20, raw.data() + 3, 20, raw.data() + 4, 20, 0, nullptr, &n2) == 0 && n2 == n_out) {
    std::vector<float> r2((size_t)n2 * 8), d2((size_t)n2 * 4);
    std::vector<int32_t> i2((size_t)n2);
    if (apdgicp_scan_ingest_copy(h, r2.data(), i2.data(), n2) == 0 && apdgicp_scan_ingest_points(h, &d_rows, nullptr, &n3) == 0 && n3 == n2 &&
        apdgicp_scan_ingest_deskew(h, d_rows, n2, 32, 12, 1, sel.first >= 0 ? queue[(size_t)sel.first].angular_velocity : nullptr, period, T) == 0 &&
        apdgicp_scan_ingest_deskewed_copy(h, d2.data(), n2) == 0)
      same = i2 == index && (n2 == 0 || (!std::memcmp(r2.data(), rows.data(), r2.size() * 4) && !std::memcmp(d2.data(), dk.data(), d2.size() * 4)));
  }
  if (h) apdgicp_scan_ingest_destroy(h);

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int32_t head[3] = {(int32_t)n_out, (int32_t)sel.first, (int32_t)ing.imuQueueSize()};
  std::fwrite(head, 4, 3, o);
  std::fwrite(rows.data(), 4, rows.size(), o);
  std::fwrite(index.data(), 4, index.size(), o);
  std::fwrite(dk.data(), 4, dk.size(), o);
  std::fclose(o);
  std::printf("%d %d\n", same, (int)n_out);
  return 0;
}
