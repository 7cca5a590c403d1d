// pcl::PointIndices as DBSCANSimpleCluster::extract fills it (pcl/PointIndices.h of PCL 1.10: a header and std::vector<int> indices).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace pcl {
struct PCLHeader {
  std::uint32_t seq = 0;
  std::uint64_t stamp = 0;
  std::string frame_id;
};
struct PointIndices {
  using Ptr = std::shared_ptr<PointIndices>;
  using ConstPtr = std::shared_ptr<const PointIndices>;
  PCLHeader header;
  std::vector<int> indices;
};
}  // namespace pcl
