// fast_gicp::FastGICPMultiPointsHip -- the counterpart of fast_gicp::FastGICPMultiPoints (fast_apdgicp/include/fast_gicp/gicp/experimental/
// fast_gicp_mp.hpp) on an MI355X: FastAPDGICPHip with the handle switched into the FastGICPMultiPoints mode (include/apdgicp_hip.h,
// "FastGICPMultiPoints as a mode of the handle", MP1 .. MP11).  The reference marks the class experimental; so is this one.
//
// It derives from FastAPDGICPHip, so the device search object behind the base-class getFitnessScore() / getSearchMethodTarget(), the
// pointer-equality caching of setInputSource / setInputTarget and the pcl::Registration setters come along.  The defaults are the
// class's own (fast_gicp_mp_impl.hpp:27-35), not the APD-GICP handle's: k 20, 64 iterations, both epsilons 1e-5, PLANE, radius 0.5.
// setNeighborSearchRadius is the one extension: the reference has no setter for its radius.
#ifndef FAST_GICP_MP_HIP_HPP
#define FAST_GICP_MP_HIP_HPP

#include "fast_apdgicp_hip.hpp"

namespace fast_gicp {

template <typename PointSource, typename PointTarget>
class FastGICPMultiPointsHip : public FastAPDGICPHip<PointSource, PointTarget> {
 public:
  using Base = FastAPDGICPHip<PointSource, PointTarget>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastGICPMultiPointsHip<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastGICPMultiPointsHip<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastGICPMultiPointsHip<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastGICPMultiPointsHip<PointSource, PointTarget>>;
#endif

  explicit FastGICPMultiPointsHip(int device = 0) : Base(device) {
    this->reg_name_ = "FastGICPMultiPointsHip";
    setCorrespondenceRandomness(20);                           // MPI:28
    this->max_iterations_ = 64;                                // MPI:30
    setRotationEpsilon(1e-5);                                  // MPI:31
    this->transformation_epsilon_ = 1e-5;                      // MPI:32
    setRegularizationMethod(RegularizationMethod::PLANE);      // MPI:33
    apdgicp_gicp_mp_default_params(&mparams_);                 // radius 0.5, MPI:35
    push_mp("FastGICPMultiPointsHip");
  }

  // ---- the setters of fast_gicp_mp.hpp:44-50 (setNumThreads is the base class's no-op), remembered for the getters below
  void setRotationEpsilon(double eps) {
    rotation_epsilon_ = eps;
    Base::setRotationEpsilon(eps);
  }
  void setCorrespondenceRandomness(int k) {
    k_correspondences_ = k;
    Base::setCorrespondenceRandomness(k);
  }
  void setRegularizationMethod(RegularizationMethod m) {
    regularization_ = m;
    Base::setRegularizationMethod(m);
  }
  void setNeighborSearchRadius(double radius) {
    mparams_.neighbor_search_radius = radius;
    push_mp("setNeighborSearchRadius");
  }
  const apdgicp_gicp_mp_params& gicpMpParams() const { return mparams_; }
  int correspondenceRandomness() const { return k_correspondences_; }
  int maximumIterations() const { return this->max_iterations_; }
  double rotationEpsilon() const { return rotation_epsilon_; }
  double transformationEpsilon() const { return this->transformation_epsilon_; }
  RegularizationMethod regularizationMethod() const { return regularization_; }
  /// apdgicp_gicp_mp_state_t of the last align; -1 on failure
  int convergenceState() const {
    int32_t s = -1;
    if (!this->handle() || apdgicp_gicp_mp_state(this->handle(), &s) != 0) return -1;
    return (int)s;
  }

 private:
  // a refused setting (a radius that is not finite and positive) leaves the handle with the last accepted one and says so on stderr,
  // like every failed call of the base class
  void push_mp(const char* what) {
    if (!this->handle()) return;
    if (apdgicp_set_gicp_mp(this->handle(), &mparams_) != 0) {
      std::fprintf(stderr, "[FastGICPMultiPointsHip] %s failed: %s\n", what, apdgicp_last_error());
      int on = 0;
      apdgicp_get_gicp_mp(this->handle(), &mparams_, &on);
      mparams_.enable = 1;
    }
  }
  apdgicp_gicp_mp_params mparams_;
  int k_correspondences_ = 20;
  double rotation_epsilon_ = 1e-5;
  RegularizationMethod regularization_ = RegularizationMethod::PLANE;
};

}  // namespace fast_gicp
#endif
