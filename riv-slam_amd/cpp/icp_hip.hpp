// pcl::IterativeClosestPointHip -- the counterpart of pcl::IterativeClosestPoint on an MI355X, for the ICP branch of radar_graph_slam's
// select_registration_method() (registrations.cpp:71-78): FastAPDGICPHip with the handle switched into the point-to-point ICP mode
// (include/apdgicp_hip.h, "point-to-point ICP as a mode of the handle", IC1 .. IC10).
//
// It derives from FastAPDGICPHip, so the device search object behind the base-class getFitnessScore() / getSearchMethodTarget(), the
// pointer-equality caching of setInputSource / setInputTarget and the pcl::Registration setters (setMaximumIterations,
// setTransformationEpsilon, setMaxCorrespondenceDistance) come along.  The defaults are PCL's own, not the APD-GICP handle's: 10
// iterations, transformation epsilon 0, no gate.  The k-NN covariances are never computed in this mode.
#ifndef APDGICP_ICP_HIP_HPP
#define APDGICP_ICP_HIP_HPP

#include <cfloat>
#include <cmath>

#include "fast_apdgicp_hip.hpp"

namespace pcl {

template <typename PointSource, typename PointTarget>
class IterativeClosestPointHip : public fast_gicp::FastAPDGICPHip<PointSource, PointTarget> {
 public:
  using Base = fast_gicp::FastAPDGICPHip<PointSource, PointTarget>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<IterativeClosestPointHip<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const IterativeClosestPointHip<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<IterativeClosestPointHip<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const IterativeClosestPointHip<PointSource, PointTarget>>;
#endif

  explicit IterativeClosestPointHip(int device = 0) : Base(device) {
    this->reg_name_ = "IterativeClosestPointHip";
    this->max_iterations_ = 10;                        // pcl::Registration: max_iterations_(10)
    this->transformation_epsilon_ = 0.0;               // transformation_epsilon_(0.0)
    this->corr_dist_threshold_ = std::sqrt(DBL_MAX);   // corr_dist_threshold_(sqrt(DBL_MAX))
    apdgicp_icp_default_params(&iparams_);
    push_icp("IterativeClosestPointHip");
  }

  // ---- the setters of registrations.cpp:74-77 that pcl::Registration does not already hold, and the two epsilons
  void setUseReciprocalCorrespondences(bool on) {
    iparams_.use_reciprocal_correspondences = on ? 1 : 0;
    push_icp("setUseReciprocalCorrespondences");
  }
  bool getUseReciprocalCorrespondences() const { return iparams_.use_reciprocal_correspondences != 0; }
  void setEuclideanFitnessEpsilon(double eps) {
    iparams_.euclidean_fitness_epsilon = eps;
    push_icp("setEuclideanFitnessEpsilon");
  }
  void setTransformationRotationEpsilon(double eps) {
    iparams_.rotation_epsilon = eps;
    push_icp("setTransformationRotationEpsilon");
  }
  const apdgicp_icp_params& icpParams() const { return iparams_; }
  // what pcl::Registration holds for this mode (its own getters, where the installed PCL has them, say the same)
  int maximumIterations() const { return this->max_iterations_; }
  double transformationEpsilon() const { return this->transformation_epsilon_; }
  double maxCorrespondenceDistance() const { return this->corr_dist_threshold_; }
  /// DefaultConvergenceCriteria::ConvergenceState of the last align (apdgicp_icp_state); -1 on failure
  int convergenceState() const {
    int32_t s = -1;
    if (!this->handle() || apdgicp_icp_convergence_state(this->handle(), &s) != 0) return -1;
    return (int)s;
  }

 private:
  // a refused setting leaves the handle with the last accepted one and says so on stderr, like every failed call of the base class
  void push_icp(const char* what) {
    if (!this->handle()) return;
    if (apdgicp_set_icp(this->handle(), &iparams_) != 0) {
      std::fprintf(stderr, "[IterativeClosestPointHip] %s failed: %s\n", what, apdgicp_last_error());
      int on = 0;
      apdgicp_get_icp(this->handle(), &iparams_, &on);
      iparams_.enable = 1;
    }
  }
  apdgicp_icp_params iparams_;
};

}  // namespace pcl
#endif
