// fast_gicp::FastVGICPCudaHip -- drop-in replacement for fast_gicp::FastVGICPCuda (fast_apdgicp/include/fast_gicp/gicp/fast_vgicp_cuda.hpp),
// the FAST_VGICP_CUDA branch of radar_graph_slam's select_registration_method() (registrations.cpp:51-61), on an MI355X: FastAPDGICPHip
// with the handle switched into that mode (include/apdgicp_hip.h, "FAST_VGICP_CUDA as a mode of the handle", VC1 .. VC10).
//
// It derives from FastAPDGICPHip, so the device search object behind the base-class getFitnessScore() / getSearchMethodTarget(), the
// pointer-equality caching of setInputSource / setInputTarget, swapSourceAndTarget / clearSource / clearTarget and the setters of the
// factory come along.  The prepared clouds and the voxel map are cached by the HANDLE, by identity (VC10).
#ifndef FAST_GICP_FAST_VGICP_CUDA_HIP_HPP
#define FAST_GICP_FAST_VGICP_CUDA_HIP_HPP

#include <cmath>

#include "fast_apdgicp_hip.hpp"

namespace fast_gicp {

#ifndef FAST_GICP_FAST_VGICP_CUDA_HPP  // same enum as gicp/fast_vgicp_cuda.hpp:21 when that header is absent
enum class NearestNeighborMethod { CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL };
#endif

template <typename PointSource, typename PointTarget>
class FastVGICPCudaHip : public FastAPDGICPHip<PointSource, PointTarget> {
 public:
  using Base = FastAPDGICPHip<PointSource, PointTarget>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastVGICPCudaHip<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastVGICPCudaHip<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastVGICPCudaHip<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastVGICPCudaHip<PointSource, PointTarget>>;
#endif

  explicit FastVGICPCudaHip(int device = 0) : Base(device) {
    this->reg_name_ = "FastVGICPCudaHip";
    apdgicp_vgicp_cuda_default_params(&vparams_);  // 1.0, DIRECT1, PLANE, CPU_PARALLEL_KDTREE: fast_vgicp_cuda_impl.hpp:22-32
    push_mode("FastVGICPCudaHip");
  }

  // ---- the setters of the reference (fast_vgicp_cuda_impl.hpp:37-72)
  void setCorrespondenceRandomness(int) {}  // a no-op there too (:38): k is 20
  void setResolution(double resolution) {
    vparams_.resolution = resolution;
    push_mode("setResolution");
  }
  void setKernelWidth(double kernel_width, double max_dist = -1.0) {  // stored; only GPU_RBF_KERNEL would read them
    kernel_width_ = kernel_width;
    kernel_max_dist_ = max_dist <= 0.0 ? kernel_width * 5.0 : max_dist;
  }
  void setRegularizationMethod(RegularizationMethod method) {
    vparams_.regularization = static_cast<int32_t>(method);  // same numeric values as apdgicp_regularization
    push_mode("setRegularizationMethod");
  }
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) {
    switch (method) {  // (the C ABI numbers the methods by their size, the reference's enum starts with DIRECT27)
      case NeighborSearchMethod::DIRECT1: vparams_.neighbor_search = APDGICP_VGICP_DIRECT1; break;
      case NeighborSearchMethod::DIRECT7: vparams_.neighbor_search = APDGICP_VGICP_DIRECT7; break;
      case NeighborSearchMethod::DIRECT27: vparams_.neighbor_search = APDGICP_VGICP_DIRECT27; break;
      default:
        vparams_.neighbor_search = APDGICP_VGICP_CUDA_DIRECT_RADIUS;
        vparams_.search_radius = radius;
        break;
    }
    push_mode("setNeighborSearchMethod");
  }
  void setNearestNeighborSearchMethod(NearestNeighborMethod method) {
    vparams_.nn_method = static_cast<int32_t>(method);  // same numeric values as apdgicp_nn_method
    push_mode("setNearestNeighborSearchMethod");
  }
  const apdgicp_vgicp_cuda_params& vgicpCudaParams() const { return vparams_; }
  double kernelWidth() const { return kernel_width_; }
  double kernelMaxDist() const { return kernel_max_dist_; }
  /// number of kept points of the source (0) or target (1) cloud (prepares it when it is not); -1 on failure
  long keptCount(int which) {
    int64_t n = -1;
    if (!this->handle() || apdgicp_vgicp_cuda_kept(this->handle(), which, &n, nullptr, 0) != 0) {
      std::fprintf(stderr, "[FastVGICPCudaHip] keptCount failed: %s\n", apdgicp_last_error());
      return -1;
    }
    return (long)n;
  }
  /// number of voxels of the prepared target's map (builds it when it is not there); -1 on failure
  long voxelCount() {
    int64_t n = -1;
    if (!this->handle() || apdgicp_vgicp_cuda_voxel_count(this->handle(), &n) != 0) {
      std::fprintf(stderr, "[FastVGICPCudaHip] voxelCount failed: %s\n", apdgicp_last_error());
      return -1;
    }
    return (long)n;
  }

 private:
  // a refused setting (GPU_RBF_KERNEL, NONE, NORMALIZED_MIN_EIG, a radius outside [0, 4], a resolution <= 0) leaves the handle with the
  // last accepted one and says so on stderr, like every failed call of the base class
  void push_mode(const char* what) {
    if (!this->handle()) return;
    if (apdgicp_set_vgicp_cuda(this->handle(), &vparams_) != 0) {
      std::fprintf(stderr, "[FastVGICPCudaHip] %s failed: %s\n", what, apdgicp_last_error());
      int on = 0;
      apdgicp_get_vgicp_cuda(this->handle(), &vparams_, &on);
    }
  }
  apdgicp_vgicp_cuda_params vparams_;
  double kernel_width_ = 0.5, kernel_max_dist_ = 3.0;  // fast_vgicp_cuda_impl.hpp:31
};

}  // namespace fast_gicp
#endif
