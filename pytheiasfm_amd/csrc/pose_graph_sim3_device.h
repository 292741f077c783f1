// pose_graph_sim3_device.h -- the per-edge and per-node arithmetic of the Sim(3) pose graph (csrc/pose_graph_sim3.hip, DESIGN.md
// 3.6x), host and device, over sim3_device.h: Sim3ReconAlignErrorTerm (sfm/transformation/pose_graph_sim3_error.h:46-103) and
// Sim3Manifold::Plus (align_reconstructions_pose_graph_optim.cc:39-56).  Compile without FMA contraction.
//
// THE TERM, as the reference writes it.  Edge (i, j) with the measurement Sji:  r = log(Sji exp(x_i) exp(x_j)^-1), 7 rows in
// Sophus' order upsilon | omega | sigma.  With Jr0 the 7 x 7 matrix whose blocks are (0,0) = hat(omega_r) + sigma_r I,
// (0,3) = hat(upsilon_r), (0,6) = -upsilon_r, (3,3) = hat(omega_r) -- built from the UNWEIGHTED r --,
//   J_i = sqrt_information (I + Jr0 / 2 + Jr0^2 / 12) Adj(exp(x_j)),   J_j = -J_i,   residual = sqrt_information r.
// This is the derivative along Sim3Manifold::Plus (a right perturbation) as a truncated series, not the derivative in the
// ambient 7-vector; it is restated, not improved.  The series is evaluated by its blocks (the structural zeros of Jr0 are not
// multiplied out): the same numbers as the 7 x 7 products for finite entries.
//
// A group element is kept as (scale, R, t), x -> scale R x + t, taken from a tangent by sim3_to_rts (the unit quaternion's
// matrix and the quaternion's squared norm, as Sophus' rotationMatrix() and scale()); products and the inverse are formed on
// these, where Sophus multiplies quaternions: rounding level.
#pragma once
#include "sim3_device.h"

namespace thip {
namespace sim3 {

struct Sim3T { double s, R[9], t[3]; };

S3D void group_from_tangent(const double* a, Sim3T& S) { sim3_to_rts(a, S.R, S.t, &S.s); }

S3D void compose(const Sim3T& A, const Sim3T& B, Sim3T& C) {   // C = A B
  C.s = A.s * B.s;
  mul33(A.R, B.R, C.R);
  double v[3];
  mul3v(A.R, B.t, v);
  for (int r = 0; r < 3; ++r) C.t[r] = A.s * v[r] + A.t[r];
}
S3D void invert(const Sim3T& A, Sim3T& B) {   // Sim3::inverse(): (rxso3^-1, -(rxso3^-1 t))
  B.s = 1.0 / A.s;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) B.R[3 * r + c] = A.R[3 * c + r];
  double v[3];
  mul3v(B.R, A.t, v);
  for (int r = 0; r < 3; ++r) B.t[r] = -(B.s * v[r]);
}

// r = log(Sji exp(x_i) exp(x_j)^-1), z = log(Sji); Sj = exp(x_j) for the adjoint.  false where Sophus' log would abort (r is
// then NaN).
S3D bool pose_graph_residual(const double* xi, const double* xj, const double* z, double* r, Sim3T& Sj) {
  Sim3T Z, Si, Sjinv, A, E;
  group_from_tangent(z, Z);
  group_from_tangent(xi, Si);
  group_from_tangent(xj, Sj);
  invert(Sj, Sjinv);
  compose(Si, Sjinv, A);
  compose(Z, A, E);
  const bool ok = sim3_log(E.s, E.R, E.t, r);
  if (!ok)
    for (int k = 0; k < 7; ++k) r[k] = NAN;
  return ok;
}

// M = I + Jr0 / 2 + Jr0^2 / 12 of the unweighted residual r, row-major 7 x 7.  With A = hat(omega) + sigma I, U = hat(upsilon),
// O = hat(omega):  Jr0 = [A U -u; 0 O 0; 0 0 0],  Jr0^2 = [A^2  AU + UO  -Au; 0 O^2 0; 0 0 0].
S3D void pose_graph_series(const double* r, double* M) {
  const double* u = r;
  const double* w = r + 3;
  const double sigma = r[6];
  double A[9], U[9], O[9], A2[9], AU[9], UO[9], O2[9], Au[3];
  hat(w, O);
  hat(u, U);
  for (int k = 0; k < 9; ++k) A[k] = O[k];
  A[0] += sigma; A[4] += sigma; A[8] += sigma;
  mul33(A, A, A2);
  mul33(A, U, AU);
  mul33(U, O, UO);
  mul33(O, O, O2);
  mul3v(A, u, Au);
  for (int k = 0; k < 49; ++k) M[k] = 0.0;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      const double id = a == b ? 1.0 : 0.0;
      M[7 * a + b] = (id + 0.5 * A[3 * a + b]) + (1.0 / 12.0) * A2[3 * a + b];
      M[7 * a + 3 + b] = 0.5 * U[3 * a + b] + (1.0 / 12.0) * (AU[3 * a + b] + UO[3 * a + b]);
      M[7 * (3 + a) + 3 + b] = (id + 0.5 * O[3 * a + b]) + (1.0 / 12.0) * O2[3 * a + b];
    }
    M[7 * a + 6] = 0.5 * (-u[a]) + (1.0 / 12.0) * (-Au[a]);
  }
  M[48] = 1.0;
}

// Sophus' Sim3::Adj() (sim3.hpp): [sR  hat(t) R  -t; 0 R 0; 0 0 1], row-major 7 x 7
S3D void sim3_adjoint(const Sim3T& S, double* Adj) {
  double T[9], TR[9];
  hat(S.t, T);
  mul33(T, S.R, TR);
  for (int k = 0; k < 49; ++k) Adj[k] = 0.0;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      Adj[7 * a + b] = S.s * S.R[3 * a + b];
      Adj[7 * a + 3 + b] = TR[3 * a + b];
      Adj[7 * (3 + a) + 3 + b] = S.R[3 * a + b];
    }
    Adj[7 * a + 6] = -S.t[a];
  }
  Adj[48] = 1.0;
}

// The term of one edge: res [7] = W r, Ji [49] row-major = (W M) Adj(exp(x_j)); W [49] row-major or null = identity.  Ji may
// be null (the candidate's cost).  Returns false where the logarithm is not defined (res is NaN, Ji untouched).
S3D bool pose_graph_term(const double* xi, const double* xj, const double* z, const double* W, double* res, double* Ji) {
  double r[7];
  Sim3T Sj;
  const bool ok = pose_graph_residual(xi, xj, z, r, Sj);
  for (int a = 0; a < 7; ++a) {
    if (W) {
      double s = 0.0;
      for (int k = 0; k < 7; ++k) s += W[7 * a + k] * r[k];
      res[a] = s;
    } else {
      res[a] = r[a];
    }
  }
  if (!ok || !Ji) return ok;
  double M[49], Adj[49];
  pose_graph_series(r, M);
  sim3_adjoint(Sj, Adj);
  for (int a = 0; a < 7; ++a) {
    double row[7];
    for (int c = 0; c < 7; ++c) {
      if (W) {
        double s = 0.0;
        for (int k = 0; k < 7; ++k) s += W[7 * a + k] * M[7 * k + c];
        row[c] = s;
      } else {
        row[c] = M[7 * a + c];
      }
    }
    for (int c = 0; c < 7; ++c) {
      double s = 0.0;
      for (int k = 0; k < 7; ++k) s += row[k] * Adj[7 * k + c];
      Ji[7 * a + c] = s;
    }
  }
  return true;
}

// Sim3Manifold::Plus: log(exp(x) exp(d')), d' = d with d'[6] = max(d[6], -20).  false where the logarithm is not defined.
S3D bool pose_graph_plus(const double* x, const double* d, double* out) {
  double dd[7];
  for (int k = 0; k < 7; ++k) dd[k] = d[k];
  dd[6] = dd[6] < -20.0 ? -20.0 : dd[6];   // std::max(d[6], -20.)
  Sim3T X, D, P;
  group_from_tangent(x, X);
  group_from_tangent(dd, D);
  compose(X, D, P);
  return sim3_log(P.s, P.R, P.t, out);
}

}  // namespace sim3
}  // namespace thip
