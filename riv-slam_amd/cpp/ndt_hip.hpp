// fast_gicp::NDTHip -- the counterpart of fast_gicp::NDTCuda (fast_apdgicp/include/fast_gicp/ndt/ndt_cuda.hpp) on an MI355X, for the NDT
// branch of radar_graph_slam's select_registration_method() (registrations.cpp:101-134): FastAPDGICPHip with the handle switched into
// the NDT mode (include/apdgicp_hip.h, "NDT (P2D / D2D) as a mode of the handle", N1 .. N9).
//
// It derives from FastAPDGICPHip, so the device search object behind the base-class getFitnessScore() / getSearchMethodTarget(), the
// pointer-equality caching of setInputSource / setInputTarget and every setter of the factory come along.  The voxel maps are cached by
// the HANDLE, by identity of the points they were made from; swapSourceAndTarget swaps them with the clouds (ndt_cuda_impl.hpp:90-93),
// which the base class already forwards -- so nothing of that is overridden here.  The k-NN covariances are never computed in this mode.
#ifndef FAST_GICP_NDT_HIP_HPP
#define FAST_GICP_NDT_HIP_HPP

#include "fast_apdgicp_hip.hpp"

namespace fast_gicp {

enum class NDTDistanceMode { P2D, D2D };  // ndt/ndt_settings.hpp

template <typename PointSource, typename PointTarget>
class NDTHip : public FastAPDGICPHip<PointSource, PointTarget> {
 public:
  using Base = FastAPDGICPHip<PointSource, PointTarget>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<NDTHip<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const NDTHip<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<NDTHip<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const NDTHip<PointSource, PointTarget>>;
#endif

  explicit NDTHip(int device = 0) : Base(device) {
    this->reg_name_ = "NDTHip";
    apdgicp_ndt_default_params(&nparams_);  // 1.0, D2D, DIRECT7: ndt_cuda_impl.hpp:15-22
    push_ndt("NDTHip");
  }

  // ---- the three setters of the reference (ndt_cuda_impl.hpp:30-50)
  void setDistanceMode(NDTDistanceMode mode) {
    nparams_.distance_mode = mode == NDTDistanceMode::P2D ? APDGICP_NDT_P2D : APDGICP_NDT_D2D;
    push_ndt("setDistanceMode");
  }
  void setResolution(double resolution) {
    nparams_.resolution = resolution;
    push_ndt("setResolution");
  }
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) {
    (void)radius;  // belongs to DIRECT_RADIUS, which is refused below
    switch (method) {  // (the C ABI numbers the methods by their size, the reference's enum starts with DIRECT27)
      case NeighborSearchMethod::DIRECT1: nparams_.neighbor_search = APDGICP_VGICP_DIRECT1; break;
      case NeighborSearchMethod::DIRECT7: nparams_.neighbor_search = APDGICP_VGICP_DIRECT7; break;
      case NeighborSearchMethod::DIRECT27: nparams_.neighbor_search = APDGICP_VGICP_DIRECT27; break;
      default: nparams_.neighbor_search = APDGICP_NDT_DIRECT_RADIUS; break;
    }
    push_ndt("setNeighborSearchMethod");
  }
  const apdgicp_ndt_params& ndtParams() const { return nparams_; }
  /// number of voxels of the map of APDGICP_SOURCE / APDGICP_TARGET (builds it when it is not there); -1 on failure
  long voxelCount(int which = APDGICP_TARGET) {
    int64_t n = -1;
    if (!this->handle() || apdgicp_ndt_voxel_count(this->handle(), which, &n) != 0) {
      std::fprintf(stderr, "[NDTHip] voxelCount failed: %s\n", apdgicp_last_error());
      return -1;
    }
    return (long)n;
  }
  /// how many voxel maps the handle has built in this mode (what the cache rules are observed by); -1 on failure
  long buildCount() {
    int64_t n = -1;
    if (!this->handle() || apdgicp_ndt_build_count(this->handle(), &n) != 0) return -1;
    return (long)n;
  }

 private:
  // a refused setting (DIRECT_RADIUS, a resolution <= 0) leaves the handle with the last accepted one and says so on stderr, like every
  // failed call of the base class
  void push_ndt(const char* what) {
    if (!this->handle()) return;
    if (apdgicp_set_ndt(this->handle(), &nparams_) != 0) {
      std::fprintf(stderr, "[NDTHip] %s failed: %s\n", what, apdgicp_last_error());
      int on = 0;
      apdgicp_get_ndt(this->handle(), &nparams_, &on);
    }
  }
  apdgicp_ndt_params nparams_;
};

}  // namespace fast_gicp
#endif
