// fast_gicp::FastVGICPHip -- drop-in replacement for fast_gicp::FastVGICP (fast_apdgicp/include/fast_gicp/gicp/fast_vgicp.hpp), the
// FAST_VGICP branch of radar_graph_slam's select_registration_method() (registrations.cpp:62-70), on an MI355X: FastAPDGICPHip with
// the handle switched into the voxelized mode (include/apdgicp_hip.h, "voxelized GICP as a mode of the handle", V1 .. V7).
//
// It derives from FastAPDGICPHip, so the device search object behind the base-class getFitnessScore() / getSearchMethodTarget(), the
// pointer-equality caching of setInputSource / setInputTarget and every setter of the factory come along.  The voxel map is cached by
// the HANDLE and dropped by exactly the calls the reference resets voxelmap_ in (fast_vgicp_impl.hpp:46-63: swapSourceAndTarget,
// setInputTarget with another cloud), all of which the base class already forwards -- so neither is overridden here.
#ifndef FAST_GICP_FAST_VGICP_HIP_HPP
#define FAST_GICP_FAST_VGICP_HIP_HPP

#include "fast_apdgicp_hip.hpp"

namespace fast_gicp {

template <typename PointSource, typename PointTarget>
class FastVGICPHip : public FastAPDGICPHip<PointSource, PointTarget> {
 public:
  using Base = FastAPDGICPHip<PointSource, PointTarget>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastVGICPHip<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastVGICPHip<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastVGICPHip<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastVGICPHip<PointSource, PointTarget>>;
#endif

  explicit FastVGICPHip(int device = 0) : Base(device) {
    this->reg_name_ = "FastVGICPHip";
    apdgicp_vgicp_default_params(&vparams_);  // 1.0, DIRECT1, ADDITIVE: fast_vgicp_impl.hpp:22-24
    push_vgicp("FastVGICPHip");
  }

  // ---- the three setters of the reference (fast_vgicp_impl.hpp:30-43)
  void setResolution(double resolution) {
    vparams_.resolution = resolution;
    push_vgicp("setResolution");
  }
  void setNeighborSearchMethod(NeighborSearchMethod method) {
    switch (method) {  // (the C ABI numbers the methods by their size, the reference's enum starts with DIRECT27)
      case NeighborSearchMethod::DIRECT1: vparams_.neighbor_search = APDGICP_VGICP_DIRECT1; break;
      case NeighborSearchMethod::DIRECT7: vparams_.neighbor_search = APDGICP_VGICP_DIRECT7; break;
      case NeighborSearchMethod::DIRECT27: vparams_.neighbor_search = APDGICP_VGICP_DIRECT27; break;
      default: vparams_.neighbor_search = -1; break;  // DIRECT_RADIUS: "supported on only VGICP_CUDA" (gicp_settings.hpp:8); refused below
    }
    push_vgicp("setNeighborSearchMethod");
  }
  void setVoxelAccumulationMode(VoxelAccumulationMode mode) {
    vparams_.voxel_mode = static_cast<int32_t>(mode);  // same numeric values as apdgicp_vgicp_mode
    push_vgicp("setVoxelAccumulationMode");
  }
  const apdgicp_vgicp_params& vgicpParams() const { return vparams_; }
  /// number of voxels of the target's map (builds it when it is not there); -1 on failure
  long voxelCount() {
    int64_t n = -1;
    if (!this->handle() || apdgicp_vgicp_voxel_count(this->handle(), &n) != 0) {
      std::fprintf(stderr, "[FastVGICPHip] voxelCount failed: %s\n", apdgicp_last_error());
      return -1;
    }
    return (long)n;
  }

 private:
  // a refused setting (MULTIPLICATIVE, DIRECT_RADIUS, a resolution <= 0) leaves the handle with the last accepted one and says so on
  // stderr, like every failed call of the base class
  void push_vgicp(const char* what) {
    if (!this->handle()) return;
    if (apdgicp_set_vgicp(this->handle(), &vparams_) != 0) {
      std::fprintf(stderr, "[FastVGICPHip] %s failed: %s\n", what, apdgicp_last_error());
      int on = 0;
      apdgicp_get_vgicp(this->handle(), &vparams_, &on);
    }
  }
  apdgicp_vgicp_params vparams_;
};

}  // namespace fast_gicp
#endif
