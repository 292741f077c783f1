// ransac_solvers.hip -- the minimal solvers bound directly (pytheia's sfm module): five-point, P4Pf, P4Pfr, P3P, SQPnP and
// DLS-PnP on rows of whole problems.  Host code only: the kernels are the RANSAC stages of ransac.hip, dls_kernels.hip and
// p4pfr_kernels.hip behind their launch_* functions; every call enqueues on the shared solver stream (SolverCall).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ransac_internal.h"

using namespace thip;

namespace {

// P4Pf / P4Pfr rows as RANSAC problems: one problem of four data per call row, one hypothesis each with the identity
// sample, so that the RANSAC stages run as they are.  mm = models per hypothesis of the estimator.
struct FourPointProblems {
  size_t n = 0;
  int mm = 0;
  DBuf<double> dc, dmod; DBuf<int> dn, dsamp, dact, ddense, dtags, dbase; DBuf<int64_t> doff;
  std::vector<int64_t> off; std::vector<int> samp, act; std::vector<double> hm;   // sources / destination of asynchronous copies
  int upload(int num, int max_models, const double* corr2d3d, hipStream_t st) {
    n = (size_t)num; mm = max_models;
    int rc;
    if ((rc = dc.ensure(n * 20)) || (rc = dmod.ensure(n * mm * kStride)) || (rc = dn.ensure(n)) || (rc = dsamp.ensure(n * 4)) ||
        (rc = dact.ensure(n)) || (rc = ddense.ensure(n)) || (rc = dtags.ensure(n * mm)) || (rc = dbase.ensure(n)) || (rc = doff.ensure(n + 1)))
      return rc;
    off.resize(n + 1); samp.resize(n * 4); act.assign(n, 1);
    for (size_t i = 0; i <= n; ++i) off[i] = (int64_t)(4 * i);
    for (size_t i = 0; i < n * 4; ++i) samp[i] = (int)(i % 4);
    HIP_TRYR(hipMemcpyAsync(dc.p, corr2d3d, sizeof(double) * n * 20, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemcpyAsync(dsamp.p, samp.data(), sizeof(int) * n * 4, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemcpyAsync(dact.p, act.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemsetAsync(ddense.p, 0, sizeof(int) * n, st));
    HIP_TRYR(hipMemsetAsync(dmod.p, 0, sizeof(double) * n * mm * kStride, st));
    return 0;
  }
  // waits for the call; models: [n][mm][width], the first `width` doubles of every model row, zero past a row's solutions
  int download(SolverCall& call, int width, double* models, int32_t* num_solutions) {
    hm.resize(n * mm * kStride);
    HIP_TRYR(hipMemcpyAsync(hm.data(), dmod.p, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, call.st));
    HIP_TRYR(hipMemcpyAsync(num_solutions, dn.p, sizeof(int) * n, hipMemcpyDeviceToHost, call.st));
    HIP_TRYR(hipGetLastError());
    HIP_TRYR(call.wait());
    for (size_t i = 0; i < n; ++i)
      for (int j = 0; j < mm; ++j)
        for (int k = 0; k < width; ++k) models[(i * mm + j) * width + k] = j < num_solutions[i] ? hm[(i * mm + j) * kStride + k] : 0.0;
    return 0;
  }
};

}  // namespace

extern "C" {

int theia_hip_five_point_relative_pose(int32_t num, const double* corr, double* essential_matrices, int32_t* num_solutions) {
  if (num < 0 || (num > 0 && (!corr || !essential_matrices || !num_solutions))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (num == 0) return 0;
  SolverCall call;
  int rc = call.open();
  if (rc) return rc;
  hipStream_t st = call.st;
  DBuf<double> dc, de; DBuf<int> dn;
  if ((rc = dc.ensure((size_t)num * 20)) || (rc = de.ensure((size_t)num * 90)) || (rc = dn.ensure(num))) return rc;
  HIP_TRYR(hipMemcpyAsync(dc.p, corr, sizeof(double) * num * 20, hipMemcpyHostToDevice, st));
  launch_five_point(num, dc.p, de.p, dn.p, st);
  HIP_TRYR(hipMemcpyAsync(essential_matrices, de.p, sizeof(double) * num * 90, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(num_solutions, dn.p, sizeof(int) * num, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(call.wait());
  return 0;
}

int theia_hip_four_point_pose_and_focal_length(int32_t num, const double* corr2d3d, double* projection_matrices, int32_t* num_solutions) {
  if (num < 0 || (num > 0 && (!corr2d3d || !projection_matrices || !num_solutions))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (num == 0) return 0;
  SolverCall call;
  int rc = call.open();
  if (rc) return rc;
  FourPointProblems prob;
  DBuf<double> dws, dsol; DBuf<int> dok, dmask;
  const size_t n = (size_t)num;
  if ((rc = dws.ensure(n * (size_t)p4pf_workspace_doubles())) || (rc = dsol.ensure(n * 50)) || (rc = dok.ensure(n)) || (rc = dmask.ensure(n)) ||
      (rc = prob.upload(num, 10, corr2d3d, call.st)))
    return rc;
  if ((rc = launch_p4pf_fit(num, 1, prob.doff.p, prob.dc.p, prob.dsamp.p, prob.dact.p, dws.p, dsol.p, dok.p, dmask.p, prob.dmod.p, prob.dn.p,
                            prob.ddense.p, prob.dtags.p, prob.dbase.p, call.st)))
    return rc;
  return prob.download(call, 12, projection_matrices, num_solutions);
}

int theia_hip_four_point_focal_length_radial_distortion(int32_t num, const double* corr2d3d, const double* limits, const double* rotation_draws,
                                                        double* models, int32_t* num_solutions) {
  // (the six-argument form of rounds 1 - 4 keeps its symbol and its ABI; the solver's pre-filter count is the _ex form's)
  return theia_hip_four_point_focal_length_radial_distortion_ex(num, corr2d3d, limits, rotation_draws, models, num_solutions, nullptr);
}

int theia_hip_four_point_focal_length_radial_distortion_ex(int32_t num, const double* corr2d3d, const double* limits, const double* rotation_draws,
                                                           double* models, int32_t* num_solutions, int32_t* num_solver_solutions) {
  if (num < 0 || !limits || (num > 0 && (!corr2d3d || !models || !num_solutions))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = p4pfr_check_limits(limits);
  if (rc || num == 0) return rc;
  SolverCall call;
  if ((rc = call.open()) || (rc = p4pfr_ensure_tables())) return rc;
  hipStream_t st = call.st;
  constexpr int kMm = 13, kMd = 14;
  FourPointProblems prob;
  DBuf<double> dws, drot; DBuf<int> dsolver;
  const size_t n = (size_t)num;
  if ((rc = dsolver.ensure(n)) || (rc = dws.ensure(n * (size_t)p4pfr_workspace_doubles())) || (rc = drot.ensure(n * 9))) return rc;
  std::vector<double> rot(n * 9);
  Mt19937 g;
  g.seed(42);   // rotation_draws == NULL: the calls of a fresh process, in order (the solver's static RandomNumberGenerator(42))
  for (size_t i = 0; i < n; ++i) {
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = rotation_draws ? rotation_draws[3 * i + k] : g.rand_double(-0.5, 0.5);
    p4pfr_rotation_from_draws(v, rot.data() + 9 * i);
  }
  if ((rc = prob.upload(num, kMm, corr2d3d, st))) return rc;
  HIP_TRYR(hipMemcpyAsync(drot.p, rot.data(), sizeof(double) * n * 9, hipMemcpyHostToDevice, st));
  launch_p4pfr_fit(num, 1, prob.doff.p, prob.dc.p, prob.dsamp.p, prob.dact.p, drot.p, limits, dws.p, prob.dmod.p, prob.dn.p, prob.ddense.p,
                   prob.dtags.p, prob.dbase.p, st, dsolver.p);
  if (num_solver_solutions) HIP_TRYR(hipMemcpyAsync(num_solver_solutions, dsolver.p, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  return prob.download(call, kMd, models, num_solutions);
}

int theia_hip_pose_from_three_points(int32_t num, const double* corr2d3d, double* rotations, double* translations, int32_t* num_solutions) {
  if (num < 0 || (num > 0 && (!corr2d3d || !rotations || !translations || !num_solutions))) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (num == 0) return 0;
  SolverCall call;
  int rc = call.open();
  if (rc) return rc;
  hipStream_t st = call.st;
  DBuf<double> dc, dr, dt; DBuf<int> dn;
  if ((rc = dc.ensure((size_t)num * 15)) || (rc = dr.ensure((size_t)num * 36)) || (rc = dt.ensure((size_t)num * 12)) || (rc = dn.ensure(num))) return rc;
  HIP_TRYR(hipMemcpyAsync(dc.p, corr2d3d, sizeof(double) * num * 15, hipMemcpyHostToDevice, st));
  launch_p3p(num, dc.p, dr.p, dt.p, dn.p, st);
  HIP_TRYR(hipMemcpyAsync(rotations, dr.p, sizeof(double) * num * 36, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(translations, dt.p, sizeof(double) * num * 12, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(num_solutions, dn.p, sizeof(int) * num, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(call.wait());
  return 0;
}

int theia_hip_sqpnp(int32_t num, const int64_t* offsets, const double* features, const double* world_points,
                    double* quaternions, double* translations, int32_t* num_solutions) {
  if (num < 0 || (num > 0 && (!offsets || !features || !world_points || !quaternions || !translations || !num_solutions)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (num == 0) return 0;
  SolverCall call;
  int rc = call.open();
  if (rc) return rc;
  hipStream_t st = call.st;
  for (int i = 0; i < num; ++i)
    if (offsets[i + 1] < offsets[i]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing");
  const int64_t total = offsets[num] - offsets[0];
  if (offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  DBuf<double> df, dw, dq, dt; DBuf<int> dn; DBuf<int64_t> dof;
  if ((rc = df.ensure((size_t)std::max<int64_t>(1, total) * 2)) || (rc = dw.ensure((size_t)std::max<int64_t>(1, total) * 3)) ||
      (rc = dq.ensure((size_t)num * 72)) || (rc = dt.ensure((size_t)num * 54)) || (rc = dn.ensure(num)) || (rc = dof.ensure(num + 1)))
    return rc;
  if (total) {
    HIP_TRYR(hipMemcpyAsync(df.p, features, sizeof(double) * total * 2, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemcpyAsync(dw.p, world_points, sizeof(double) * total * 3, hipMemcpyHostToDevice, st));
  }
  HIP_TRYR(hipMemcpyAsync(dof.p, offsets, sizeof(int64_t) * (num + 1), hipMemcpyHostToDevice, st));
  launch_sqpnp(num, dof.p, df.p, dw.p, dq.p, dt.p, dn.p, st);
  HIP_TRYR(hipMemcpyAsync(quaternions, dq.p, sizeof(double) * num * 72, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(translations, dt.p, sizeof(double) * num * 54, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(num_solutions, dn.p, sizeof(int) * num, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(call.wait());
  return 0;
}

void theia_hip_dls_macaulay_terms(int64_t first_call, int64_t num_calls, double* out) {
  if (first_call < 0 || num_calls <= 0 || !out) return;
  std::vector<double> u; dls::GlibcRand gen;
  dls::dls_terms(u, gen, (size_t)(first_call + num_calls));
  std::memcpy(out, u.data() + 4 * first_call, sizeof(double) * 4 * num_calls);
}

int theia_hip_dls_pnp(int32_t num, const int64_t* offsets, const double* features, const double* world_points,
                      const int64_t* call_index, double* quaternions, double* translations, int32_t* num_solutions) {
  if (num < 0 || (num > 0 && (!offsets || !features || !world_points || !quaternions || !translations || !num_solutions)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (num == 0) return 0;
  SolverCall call;
  int rc = call.open();
  if (rc || (rc = dls_ensure_tables())) return rc;
  hipStream_t st = call.st;
  if (offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  int64_t max_call = num - 1;
  for (int i = 0; i < num; ++i) {
    if (offsets[i + 1] < offsets[i]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing");
    if (call_index) {
      if (call_index[i] < 0 || call_index[i] > (1 << 26)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "call_index out of range");
      max_call = std::max(max_call, call_index[i]);
    }
  }
  const int64_t total = offsets[num];
  std::vector<double> uall, u((size_t)num * 4); dls::GlibcRand gen;
  dls::dls_terms(uall, gen, (size_t)max_call + 1);
  for (int i = 0; i < num; ++i) std::memcpy(&u[(size_t)4 * i], &uall[(size_t)4 * (call_index ? call_index[i] : i)], 4 * sizeof(double));
  constexpr int NS = dlsdev::kMaxSolutions;
  DBuf<double> df, dw, dq, dt, du, da, dtf; DBuf<int> dn, dok; DBuf<int64_t> dof;
  if ((rc = df.ensure((size_t)std::max<int64_t>(1, total) * 2)) || (rc = dw.ensure((size_t)std::max<int64_t>(1, total) * 3)) ||
      (rc = dq.ensure((size_t)num * 4 * NS)) || (rc = dt.ensure((size_t)num * 3 * NS)) || (rc = dn.ensure(num)) || (rc = dof.ensure(num + 1)) ||
      (rc = du.ensure((size_t)num * 4)) || (rc = da.ensure((size_t)num * 729)) || (rc = dtf.ensure((size_t)num * 27)) || (rc = dok.ensure(num)))
    return rc;
  if (total) {
    HIP_TRYR(hipMemcpyAsync(df.p, features, sizeof(double) * total * 2, hipMemcpyHostToDevice, st));
    HIP_TRYR(hipMemcpyAsync(dw.p, world_points, sizeof(double) * total * 3, hipMemcpyHostToDevice, st));
  }
  HIP_TRYR(hipMemcpyAsync(dof.p, offsets, sizeof(int64_t) * (num + 1), hipMemcpyHostToDevice, st));
  HIP_TRYR(hipMemcpyAsync(du.p, u.data(), sizeof(double) * num * 4, hipMemcpyHostToDevice, st));
  launch_dls_solve_a(num, dof.p, df.p, dw.p, du.p, da.p, dtf.p, dok.p, st);
  launch_dls_solve_b(num, dof.p, dw.p, da.p, dtf.p, dok.p, dq.p, dt.p, dn.p, st);
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(hipMemcpyAsync(quaternions, dq.p, sizeof(double) * num * 4 * NS, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(translations, dt.p, sizeof(double) * num * 3 * NS, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipMemcpyAsync(num_solutions, dn.p, sizeof(int) * num, hipMemcpyDeviceToHost, st));
  HIP_TRYR(hipGetLastError());
  HIP_TRYR(call.wait());
  return 0;
}

void theia_hip_release_scratch(void) { dev_pool().release(); host_pool().release(); }

}  // extern "C"
