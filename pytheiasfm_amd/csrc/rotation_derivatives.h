// rotation_derivatives.h -- ceres::AngleAxisToRotationMatrix and ceres::RotationMatrixToAngleAxis with the closed-form
// derivatives of the branch each call took (what Ceres' Jets give), one thread per call.  Shared by the two Levenberg-Marquardt
// loops whose residual is the logarithm of a product of rotations: nonlinear_rotations.hip (PairwiseRotationError; DESIGN.md
// 3.6i has the derivation) and alignment.hip (RotationAlignmentError of AlignRotations).  Pinned against 50-digit arithmetic
// through theia_hip_selftest_pairwise_rotation_error.  The including file must be compiled without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace thip {

// ceres::AngleAxisToRotationMatrix, row-major, and what its derivative needs
struct AaCtx {
  double u[3], theta, c, s;
  bool big;
};

__device__ __forceinline__ void aa_rot(const double* w, AaCtx& a, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  a.big = t2 > DBL_EPSILON;
  if (a.big) {
    a.theta = sqrt(t2);
    const double wx = w[0] / a.theta, wy = w[1] / a.theta, wz = w[2] / a.theta;
    const double c = cos(a.theta), s = sin(a.theta);
    a.u[0] = wx; a.u[1] = wy; a.u[2] = wz; a.c = c; a.s = s;
    R[0] = c + wx * wx * (1.0 - c);      R[3] = wz * s + wx * wy * (1.0 - c);  R[6] = -wy * s + wx * wz * (1.0 - c);
    R[1] = wx * wy * (1.0 - c) - wz * s; R[4] = c + wy * wy * (1.0 - c);       R[7] = wx * s + wy * wz * (1.0 - c);
    R[2] = wy * s + wx * wz * (1.0 - c); R[5] = -wx * s + wy * wz * (1.0 - c); R[8] = c + wz * wz * (1.0 - c);
  } else {
    a.u[0] = a.u[1] = a.u[2] = 0.0; a.theta = 0.0; a.c = 1.0; a.s = 0.0;
    R[0] = 1.0; R[3] = w[2]; R[6] = -w[1];
    R[1] = -w[2]; R[4] = 1.0; R[7] = w[0];
    R[2] = w[1]; R[5] = -w[0]; R[8] = 1.0;
  }
}

// dR / dw_K of the branch aa_rot took
template <int K>
__device__ __forceinline__ void aa_rot_d(const AaCtx& a, double* D) {
  double v[3];   // the derivative of s u, the vector of the skew part
  if (a.big) {
    double du[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) du[i] = ((i == K ? 1.0 : 0.0) - a.u[i] * a.u[K]) / a.theta;
    const double dc = -a.s * a.u[K], ds = a.c * a.u[K], omc = 1.0 - a.c;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        D[3 * r + q] = ((r == q ? dc : 0.0) - dc * (a.u[r] * a.u[q])) + omc * (du[r] * a.u[q] + a.u[r] * du[q]);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = ds * a.u[i] + a.s * du[i];
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) D[q] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = i == K ? 1.0 : 0.0;
  }
  D[1] -= v[2]; D[2] += v[1]; D[3] += v[2]; D[5] -= v[0]; D[6] -= v[1]; D[7] += v[0];
}

// ceres::RotationMatrixToAngleAxis (RotationMatrixToQuaternion, then QuaternionToAngleAxis) and what its derivative needs
struct LogCtx {
  int branch;   // 0: trace >= 0; 1 + i: the largest diagonal entry is i
  bool has_sin;
  double t, h, q[4], st, kf;
};

template <int I>
__device__ __forceinline__ void quat_diag(const double* E, LogCtx& L) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  L.t = sqrt(E[I * 3 + I] - E[J * 3 + J] - E[K * 3 + K] + 1.0);
  L.q[I + 1] = 0.5 * L.t;
  L.h = 0.5 / L.t;
  L.q[0] = (E[K * 3 + J] - E[J * 3 + K]) * L.h;
  L.q[J + 1] = (E[J * 3 + I] + E[I * 3 + J]) * L.h;
  L.q[K + 1] = (E[K * 3 + I] + E[I * 3 + K]) * L.h;
}
template <int I>
__device__ __forceinline__ void quat_diag_d(const double* E, const double* dE, const LogCtx& L, double* dq) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  const double dt = (dE[I * 3 + I] - dE[J * 3 + J] - dE[K * 3 + K]) / (2.0 * L.t);
  const double dh = -0.5 * dt / (L.t * L.t);
  dq[I + 1] = 0.5 * dt;
  dq[0] = (dE[K * 3 + J] - dE[J * 3 + K]) * L.h + (E[K * 3 + J] - E[J * 3 + K]) * dh;
  dq[J + 1] = (dE[J * 3 + I] + dE[I * 3 + J]) * L.h + (E[J * 3 + I] + E[I * 3 + J]) * dh;
  dq[K + 1] = (dE[K * 3 + I] + dE[I * 3 + K]) * L.h + (E[K * 3 + I] + E[I * 3 + K]) * dh;
}

__device__ __forceinline__ void log_rot(const double* E, LogCtx& L, double* r) {
  const double trace = E[0] + E[4] + E[8];
  if (trace >= 0.0) {
    L.branch = 0;
    L.t = sqrt(trace + 1.0);
    L.q[0] = 0.5 * L.t;
    L.h = 0.5 / L.t;
    L.q[1] = (E[7] - E[5]) * L.h; L.q[2] = (E[2] - E[6]) * L.h; L.q[3] = (E[3] - E[1]) * L.h;
  } else if (E[0] >= E[4] && E[0] >= E[8]) {   // i = 0 unless E11 > E00, then i = 2 if E22 > E[i][i]
    L.branch = 1; quat_diag<0>(E, L);
  } else if (E[4] > E[0] && E[4] >= E[8]) {
    L.branch = 2; quat_diag<1>(E, L);
  } else {
    L.branch = 3; quat_diag<2>(E, L);
  }
  const double s2 = L.q[1] * L.q[1] + L.q[2] * L.q[2] + L.q[3] * L.q[3];
  L.has_sin = s2 > 0.0;
  if (L.has_sin) {
    L.st = sqrt(s2);
    const double ct = L.q[0];
    const double two_theta = 2.0 * ((ct < 0.0) ? atan2(-L.st, -ct) : atan2(L.st, ct));
    L.kf = two_theta / L.st;
  } else {
    L.st = 0.0;
    L.kf = 2.0;
  }
  r[0] = L.q[1] * L.kf; r[1] = L.q[2] * L.kf; r[2] = L.q[3] * L.kf;
}

// dr for the matrix derivative dE, through the branches log_rot took
__device__ __forceinline__ void log_rot_d(const double* E, const double* dE, const LogCtx& L, double* dr) {
  double dq[4];
  if (L.branch == 0) {
    const double dt = ((dE[0] + dE[4]) + dE[8]) / (2.0 * L.t);
    const double dh = -0.5 * dt / (L.t * L.t);
    dq[0] = 0.5 * dt;
    dq[1] = (dE[7] - dE[5]) * L.h + (E[7] - E[5]) * dh;
    dq[2] = (dE[2] - dE[6]) * L.h + (E[2] - E[6]) * dh;
    dq[3] = (dE[3] - dE[1]) * L.h + (E[3] - E[1]) * dh;
  } else if (L.branch == 1) {
    quat_diag_d<0>(E, dE, L, dq);
  } else if (L.branch == 2) {
    quat_diag_d<1>(E, dE, L, dq);
  } else {
    quat_diag_d<2>(E, dE, L, dq);
  }
  if (L.has_sin) {
    const double ct = L.q[0];
    const double dst = ((L.q[1] * dq[1] + L.q[2] * dq[2]) + L.q[3] * dq[3]) / L.st;
    const double dtt = 2.0 * (ct * dst - L.st * dq[0]) / (L.st * L.st + ct * ct);
    const double dk = (dtt - L.kf * dst) / L.st;
    dr[0] = dq[1] * L.kf + L.q[1] * dk; dr[1] = dq[2] * L.kf + L.q[2] * dk; dr[2] = dq[3] * L.kf + L.q[3] * dk;
  } else {
    dr[0] = 2.0 * dq[1]; dr[1] = 2.0 * dq[2]; dr[2] = 2.0 * dq[3];
  }
}

}  // namespace thip
