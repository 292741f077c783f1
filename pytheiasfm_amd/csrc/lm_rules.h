// lm_rules.h -- the step rules of Ceres 2.2's TrustRegionMinimizer with LevenbergMarquardtStrategy
// (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc), once, for every Levenberg-Marquardt loop of the library:
// ba_solver.hip (lm_control_body), ba_invdepth.hip (host loop), ba_batch.hip (k_view_lm, k_track_lm), twoview_lm.hip
// (three kernels), twoview_ba.hip, ba_inner.hip (TeamLm, pt_block_lm), graph_lm.h (k_post, k_decide), alignment.hip
// (k_align_rotations), sim3_alignment.hip (sim3_advance) and pose_graph_sim3.hip (k_pg_post, k_pg_decide).
// Rules only: no loop, no linearisation, no manifold, no reduction -- each loop keeps its own body and control flow, its
// trace, counters and masks.  DESIGN.md 3.3 has the rules in words.
//
// The state is any struct with the members  double radius, decrease_factor;  <integer> invalid_steps, step_successful
// -- TrustRegion below for the loops that hold it in registers; LmState (ba_handle.h), NlState (graph_lm.h) and TeamLm
// (ba_inner.hip) carry those members among their own, in layouts the host reads back.  k_track_lm, k_fundamental_lm and
// pt_block_lm fill the register file and came out larger with their state in a TrustRegion: they keep the state and its
// updates written out (the text of shrink / invalid_step / accept / converged_before_step) and take the other rules here.
// The fast-math files ba_kernels.hip, ba_fused.hip and ba_fused_intr.hip keep their own LM diagonal and Jacobi scale.
// Every expression here is the one the loops had: same operations, same order (the files are built without FMA
// contraction and compared with the oracle bit for bit).
#pragma once
#include <cmath>

// host and device: the loop of ba_invdepth.hip runs on the host.  Defined here only.
#ifndef LMR
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LMR __host__ __device__ __forceinline__
#else
#define LMR inline
#endif
#endif

namespace thip {
namespace lm {

struct TrustRegion {
  double radius = 1e4, decrease_factor = 2.0;
  int invalid_steps = 0;          // in a row
  bool step_successful = true;    // the last step was accepted (the gradient rule applies after successful steps only)
};
// the start of a solve, for the states that are not a TrustRegion
template <class S>
LMR void start(S& s) { s.radius = 1e4; s.decrease_factor = 2.0; s.invalid_steps = 0; s.step_successful = 1; }

// LevenbergMarquardtStrategy: D = clamp(diag(J'J), 1e-6, 1e32) / radius
LMR double lm_diagonal(double h, double radius) { return fmin(fmax(h, 1e-6), 1e32) / radius; }
// Jacobi scaling of a column with squared norm colsq
LMR double jacobi_scale(double colsq) { return 1.0 / (1.0 + sqrt(colsq)); }

// Model cost change of the step -y on the packed lower triangle H (entry (a, b), a >= b, at tri(a, b)), H without the LM
// diagonal:  y'g - y'Hy / 2
LMR constexpr int tri(int a, int b) { return a * (a + 1) / 2 + b; }
template <int N>
LMR double model_cost_change(const double* H, const double* g, const double* y) {
  double yg = 0.0, yHy = 0.0;
  for (int a = 0; a < N; ++a) {
    yg += y[a] * g[a];
    double row = 0.0;
    for (int b = 0; b < N; ++b) row += H[a >= b ? tri(a, b) : tri(b, a)] * y[b];
    yHy += y[a] * row;
  }
  return yg - 0.5 * yHy;
}

// Between two iterations: the gradient tolerance (after a successful step only) and the radius floor
template <class S>
LMR bool gradient_rule(const S& s, double gmax, double gradient_tolerance) { return s.step_successful && gmax <= gradient_tolerance; }
template <class S>
LMR bool radius_floor(const S& s) { return s.radius <= 1e-32; }
template <class S>
LMR bool converged_before_step(const S& s, double gmax, double gradient_tolerance) {
  return gradient_rule(s, gmax, gradient_tolerance) || radius_floor(s);
}

// A valid step ends the run of invalid ones
template <class S>
LMR void valid_step(S& s) { s.invalid_steps = 0; }
// A rejected step (StepRejected)
template <class S>
LMR void shrink(S& s) { s.radius /= s.decrease_factor; s.decrease_factor *= 2.0; s.step_successful = 0; }
// An invalid step (the solve failed, a non-finite step, a model cost change that is not positive): false on the fifth in
// a row -- the solve has failed and the state stays --, otherwise a rejected step
template <class S>
LMR bool invalid_step(S& s) {
  if (++s.invalid_steps >= 5) return false;
  shrink(s);
  return true;
}

// The candidate's rules, in Ceres' order
LMR bool parameter_rule(double step_norm, double x_norm, double tol) { return step_norm <= tol * (x_norm + tol); }
LMR bool function_rule(double x_cost, double cand_cost, double tol) { return fabs(x_cost - cand_cost) <= tol * x_cost; }
LMR bool step_accepted(double rho) { return rho > 1e-3; }
// An accepted step (StepAccepted): radius = min(max_radius, radius / max(1/3, 1 - (2 rho - 1)^3)).
// Two forms of the cube: Ceres and the CPU oracle call pow(t, 3), and the two loops that are compared with the oracle
// step by step, trace included (ba_solver.hip, ba_invdepth.hip), keep that call (kPow); the others multiply, which the
// device's pown is not guaranteed to equal to the bit.
template <bool kPow = false, class S>
LMR void accept(S& s, double rho, double max_radius) {
  const double t = 2.0 * rho - 1.0;
  double cube;
  if constexpr (kPow) cube = pow(t, 3);
  else cube = t * t * t;
  s.radius = fmin(max_radius, s.radius / fmax(1.0 / 3.0, 1.0 - cube));
  s.decrease_factor = 2.0; s.step_successful = 1;
}

}  // namespace lm
}  // namespace thip
