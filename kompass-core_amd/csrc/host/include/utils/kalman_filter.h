// Linear state-space Kalman filter of the kompass_cpp surface (reference:
// utils/kalman_filter.{h,cpp}).  Host-side float arithmetic on a handful of
// states: the tracker runs it once per control step on one box.  Matrices are
// kc_linalg's column-major MatrixXf; S^-1 is a partial-pivot LU inverse, as
// Eigen's MatrixXf::inverse() computes it.
#pragma once

#include <cstddef>
#include <optional>

#include "kc_linalg.h"

namespace Kompass {

class LinearSSKalmanFilter {
 public:
  LinearSSKalmanFilter(const size_t num_states, const size_t num_inputs);

  // A (n x n), B (n x m), Q (n x n), H (n x n), R (n x n); false on a size mismatch
  bool setup(const Eigen::MatrixXf &A, const Eigen::MatrixXf &B, const Eigen::MatrixXf &Q,
             const Eigen::MatrixXf &H, const Eigen::MatrixXf &R);

  void setInitialState(const Eigen::VectorXf &initial_state);

  void setA(const Eigen::MatrixXf &A);

  // predict `numberSteps` steps, then update with the measurement z (n x 1) and inputs u (m x 1)
  void estimate(const Eigen::MatrixXf &z, const Eigen::MatrixXf &u, const int numberSteps = 1);

  // NOTE (reference): forwards to estimate(z, 0) WITHOUT numberSteps, so every update predicts one step
  void estimate(const Eigen::MatrixXf &z, const int numberSteps = 1);

  double getState(const size_t state_index);

  std::optional<Eigen::MatrixXf> getState();

  // the estimate's uncertainty (not in the reference's interface)
  const Eigen::MatrixXf &getCovariance() const { return P; }

 private:
  bool state_initialized = false, system_initialized = false;
  Eigen::MatrixXf state, A, B, H, P, Q, R;
};

// the inverse of a square float matrix by LU with partial (row) pivoting; throws std::runtime_error when a pivot is 0
Eigen::MatrixXf inversePartialPivLU(const Eigen::MatrixXf &M);

}  // namespace Kompass
