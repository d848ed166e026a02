// LinearSSKalmanFilter (reference: utils/kalman_filter.cpp), float throughout.
#include "utils/kalman_filter.h"

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "utils/logger.h"

namespace Kompass {

namespace {

using Eigen::Index;
using Eigen::MatrixXf;

MatrixXf zeros(Index r, Index c) {
  MatrixXf m(r, c);
  m.fill(0.0f);
  return m;
}

MatrixXf identity(Index n) {
  MatrixXf m = zeros(n, n);
  for (Index i = 0; i < n; ++i) m(i, i) = 1.0f;
  return m;
}

MatrixXf mul(const MatrixXf &a, const MatrixXf &b) {
  MatrixXf c(a.rows(), b.cols());
  for (Index i = 0; i < a.rows(); ++i)
    for (Index j = 0; j < b.cols(); ++j) {
      float s = 0.0f;
      for (Index k = 0; k < a.cols(); ++k) s += a(i, k) * b(k, j);
      c(i, j) = s;
    }
  return c;
}

MatrixXf add(const MatrixXf &a, const MatrixXf &b, float sign = 1.0f) {
  MatrixXf c(a.rows(), a.cols());
  for (Index i = 0; i < a.rows(); ++i)
    for (Index j = 0; j < a.cols(); ++j) c(i, j) = sign > 0.0f ? a(i, j) + b(i, j) : a(i, j) - b(i, j);
  return c;
}

MatrixXf transpose(const MatrixXf &a) {
  MatrixXf t(a.cols(), a.rows());
  for (Index i = 0; i < a.rows(); ++i)
    for (Index j = 0; j < a.cols(); ++j) t(j, i) = a(i, j);
  return t;
}

}  // namespace

MatrixXf inversePartialPivLU(const MatrixXf &M) {
  const Index n = M.rows();
  if (M.cols() != n) throw std::invalid_argument("inverse of a non-square matrix");
  MatrixXf lu = M;
  std::vector<Index> perm(static_cast<size_t>(n));
  for (Index i = 0; i < n; ++i) perm[static_cast<size_t>(i)] = i;
  for (Index k = 0; k < n; ++k) {
    Index p = k;
    float best = std::fabs(lu(k, k));
    for (Index i = k + 1; i < n; ++i)
      if (std::fabs(lu(i, k)) > best) {
        best = std::fabs(lu(i, k));
        p = i;
      }
    if (best == 0.0f) throw std::runtime_error("Kalman filter: singular innovation matrix");
    if (p != k) {
      for (Index j = 0; j < n; ++j) std::swap(lu(k, j), lu(p, j));
      std::swap(perm[static_cast<size_t>(k)], perm[static_cast<size_t>(p)]);
    }
    for (Index i = k + 1; i < n; ++i) {
      lu(i, k) /= lu(k, k);
      for (Index j = k + 1; j < n; ++j) lu(i, j) -= lu(i, k) * lu(k, j);
    }
  }
  // solve L U X = P I, column by column
  MatrixXf inv(n, n);
  std::vector<float> y(static_cast<size_t>(n));
  for (Index c = 0; c < n; ++c) {
    for (Index i = 0; i < n; ++i) {
      float s = perm[static_cast<size_t>(i)] == c ? 1.0f : 0.0f;
      for (Index k = 0; k < i; ++k) s -= lu(i, k) * y[static_cast<size_t>(k)];
      y[static_cast<size_t>(i)] = s;
    }
    for (Index i = n - 1; i >= 0; --i) {
      float s = y[static_cast<size_t>(i)];
      for (Index k = i + 1; k < n; ++k) s -= lu(i, k) * inv(k, c);
      inv(i, c) = s / lu(i, i);
    }
  }
  return inv;
}

LinearSSKalmanFilter::LinearSSKalmanFilter(const size_t num_states, const size_t num_inputs) {
  const Index n = static_cast<Index>(num_states), m = static_cast<Index>(num_inputs);
  state = zeros(n, 1);
  A = zeros(n, n);
  B = zeros(n, m);
  Q = zeros(n, n);
  H = zeros(n, n);
  R = zeros(n, n);
  P = identity(n);
}

bool LinearSSKalmanFilter::setup(const MatrixXf &A_, const MatrixXf &B_, const MatrixXf &Q_, const MatrixXf &H_,
                                 const MatrixXf &R_) {
  if (A_.size() != A.size() || B_.size() != B.size() || Q_.size() != Q.size() || H_.size() != H.size() ||
      R_.size() != R.size()) {
    LOG_ERROR("Cannot setup the KalmanFilter. Matrix size error. Expected the following sized: A=", A.size(),
              ", B=", B.size(), ", H=", H.size(), ", Q=", Q.size(), ", R=", R.size());
    return false;
  }
  A = A_;
  B = B_;
  H = H_;
  R = R_;
  Q = Q_;
  system_initialized = true;
  return true;
}

void LinearSSKalmanFilter::setInitialState(const Eigen::VectorXf &initial_state) {
  if (initial_state.size() != state.rows()) {
    LOG_ERROR("Cannot set initial state. Expected the following sized: ", state.rows());
    throw std::length_error("Error Setting Initial State");
  }
  for (Index i = 0; i < state.rows(); ++i) state(i, 0) = initial_state(i);
  state_initialized = true;
}

void LinearSSKalmanFilter::setA(const MatrixXf &A_) { A = A_; }

void LinearSSKalmanFilter::estimate(const MatrixXf &measurements, const MatrixXf &inputs, const int numberSteps) {
  const MatrixXf A_t = transpose(A);
  const MatrixXf B_u = mul(B, inputs);
  MatrixXf predicted = state;
  for (int i = 0; i < numberSteps; ++i) {
    predicted = add(mul(A, predicted), B_u);
    P = add(mul(mul(A, P), A_t), Q);  // covariance extrapolation
  }
  const MatrixXf H_t = transpose(H);
  const MatrixXf S = add(R, mul(mul(H, P), H_t));          // innovation
  const MatrixXf K = mul(mul(P, H_t), inversePartialPivLU(S));  // gain
  state = add(predicted, mul(K, add(measurements, mul(H, predicted), -1.0f)));
  P = mul(add(identity(P.rows()), mul(K, H), -1.0f), P);
}

void LinearSSKalmanFilter::estimate(const MatrixXf &measurements, const int numberSteps) {
  estimate(measurements, zeros(B.cols(), 1));  // (numberSteps is dropped, as in the reference)
}

double LinearSSKalmanFilter::getState(const size_t state_index) {
  return state_initialized ? state(static_cast<Index>(state_index), 0) : 0.0;
}

std::optional<Eigen::MatrixXf> LinearSSKalmanFilter::getState() {
  if (state_initialized && system_initialized) return state;
  return std::nullopt;
}

}  // namespace Kompass
