// radar_graph_slam::ScanIngestHip::runPolar / histogramAdd (riv-slam_amd/cpp/scan_ingest_hip.hpp) against tests/pcl_shim.
//   test_polar_ingest                    compile-and-link check (no GPU needed)
//   test_polar_ingest scan.bin out.bin   in: int32 n, n x 19 floats (a RadarTargetExtended[]: range, azimuth, elevation, velocity, snr, 14 more).
//                                        The class ingests the 76-byte targets, copies the rows, adds them as a pcl cloud to the histogram
//                                        twice; the C ABI called directly does the same with the five lanes at their field offsets and the
//                                        histogram from its own device rows.
//                                        out: int32 n_out, rows [n_out x 8], index [n_out], int32 counts[100], int64 distribution[100] of the
//                                        class; prints 1 when both paths gave the same bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scan_ingest_hip.hpp"

using radar_graph_slam::ScanIngestHip;

struct Target {  // the test's own msgs_radar::RadarTargetExtended: 19 floats
  float range, azimuth, elevation, velocity, snr, power, rcs, detectionconfidence;
  float mean_square_error[6], std_dev[5];
};
static_assert(sizeof(Target) == 76, "19 floats");

int main(int argc, char** argv) {
  ScanIngestHip ing;
  if (argc < 3) {
    int64_t (ScanIngestHip::*run)(const Target*, std::size_t, bool) = &ScanIngestHip::runPolar<Target>;
    bool (ScanIngestHip::*add)(const ScanIngestHip::Cloud&) = &ScanIngestHip::histogramAdd;
    std::vector<int32_t> (ScanIngestHip::*last)() = &ScanIngestHip::histogramLast;
    std::vector<int64_t> (ScanIngestHip::*dist)() = &ScanIngestHip::pointDistribution;
    const bool ok = run && add && last && dist && offsetof(Target, snr) == 16 && offsetof(Target, velocity) == 12;
    std::printf(ok ? "compile-only\n" : "the target layout is wrong\n");
    return ok ? 0 : 1;
  }
  FILE* in = std::fopen(argv[1], "rb");
  int32_t n = 0;
  if (!in || std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
  std::vector<Target> targets((size_t)n);
  if (std::fread(targets.data(), sizeof(Target), (size_t)n, in) != (size_t)n) return 2;
  std::fclose(in);

  // the class
  const int64_t n_out = ing.runPolar(targets.data(), targets.size());
  std::vector<float> rows;
  std::vector<int32_t> index;
  if (n_out != n || !ing.copyRows(rows, index) || (int64_t)index.size() != n_out) return 3;
  ScanIngestHip::Cloud cloud;
  cloud.resize((size_t)n_out);
  for (int64_t i = 0; i < n_out; i++) {
    pcl::PointXYZI& p = cloud.points[(size_t)i];
    p.x = rows[8 * i], p.y = rows[8 * i + 1], p.z = rows[8 * i + 2], p.intensity = rows[8 * i + 3];
  }
  if (!ing.histogramAdd(cloud) || !ing.histogramAdd(cloud)) return 3;
  const std::vector<int32_t> counts = ing.histogramLast();
  const std::vector<int64_t> dist = ing.pointDistribution();
  if (counts.size() != 100 || dist.size() != 100) return 3;

  // the C ABI, the histogram from its own device rows
  apdgicp_scan_ingest* h = nullptr;
  int same = 0;
  int64_t n2 = 0, n3 = 0, frames = 0;
  const float* d_rows = nullptr;
  const float* t0 = n ? &targets[0].range : nullptr;
  if (apdgicp_scan_ingest_create(nullptr, 0, nullptr, &h) == 0 &&
      apdgicp_scan_ingest_run_polar(h, t0, 76, t0 + 1, 76, t0 + 2, 76, t0 + 4, 76, t0 + 3, 76, n, 0, &n2) == 0 && n2 == n_out) {
    std::vector<float> r2((size_t)n2 * 8);
    std::vector<int32_t> i2((size_t)n2), c2(100);
    std::vector<int64_t> s2(100);
    if (apdgicp_scan_ingest_copy(h, r2.data(), i2.data(), n2) == 0 && apdgicp_scan_ingest_points(h, &d_rows, nullptr, &n3) == 0 && n3 == n2 &&
        apdgicp_scan_ingest_histogram_add(h, d_rows, n2, 32, 1) == 0 && apdgicp_scan_ingest_histogram_add(h, d_rows, n2, 32, 1) == 0 &&
        apdgicp_scan_ingest_histogram_last(h, c2.data()) == 0 && apdgicp_scan_ingest_histogram_read(h, s2.data(), &frames) == 0 && frames == 2) {
      for (int64_t& v : s2) v /= frames;
      same = i2 == index && c2 == counts && s2 == dist && (n2 == 0 || !std::memcmp(r2.data(), rows.data(), r2.size() * 4));
    }
  }
  if (h) apdgicp_scan_ingest_destroy(h);

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const int32_t head = (int32_t)n_out;
  std::fwrite(&head, 4, 1, o);
  std::fwrite(rows.data(), 4, rows.size(), o);
  std::fwrite(index.data(), 4, index.size(), o);
  std::fwrite(counts.data(), 4, counts.size(), o);
  std::fwrite(dist.data(), 8, dist.size(), o);
  std::fclose(o);
  std::printf("%d %d\n", same, (int)n_out);
  return 0;
}
