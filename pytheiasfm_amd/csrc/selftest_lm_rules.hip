// selftest_lm_rules.hip -- test-only entry point for the trust-region step rules every Levenberg-Marquardt loop of the
// library takes from lm_rules.h: a script of step outcomes the caller chooses is played through the header twice, by one
// device thread and on the host, and the state after every record comes back from both.  Nothing here runs on the
// estimation path.
#include "lm_rules.h"
#include "device_util.h"

#include <cfloat>

namespace thip {
namespace {

constexpr int kMaxRecords = 16;
constexpr int kIn = 4;    // per record: op | a | b | c
constexpr int kOut = 7;   // radius | decrease_factor | invalid_steps | step_successful | decision | value | radius floor reached
enum { OP_INVALID = 1, OP_EVALUATED = 2, OP_BEFORE_STEP = 3, OP_PARAMETER = 4, OP_FUNCTION = 5, OP_DIAGONAL = 6, OP_JACOBI = 7,
       OP_MODEL3 = 8, OP_MODEL6 = 9 };

// H[k] = a + k over the packed triangle, g[i] = b + i, y[i] = c - i
template <int N>
LMR double model_of(double a, double b, double c) {
  double H[N * (N + 1) / 2], g[N], y[N];
  for (int k = 0; k < N * (N + 1) / 2; ++k) H[k] = a + k;
  for (int i = 0; i < N; ++i) { g[i] = b + i; y[i] = c - i; }
  return lm::model_cost_change<N>(H, g, y);
}

LMR void play(int count, const double* rec, double* out) {
  lm::TrustRegion tr;
  for (int k = 0; k < count; ++k) {
    const double a = rec[kIn * k + 1], b = rec[kIn * k + 2], c = rec[kIn * k + 3];
    double decision = 0.0, value = 0.0;
    switch ((int)rec[kIn * k]) {
      case OP_INVALID: decision = lm::invalid_step(tr); break;                       // 0: the fifth in a row
      case OP_EVALUATED: {                                                            // a = rho, b = max_radius
        lm::valid_step(tr);
        lm::TrustRegion with_pow = tr;
        decision = lm::step_accepted(a);
        if (decision != 0.0) { lm::accept(tr, a, b); lm::accept<true>(with_pow, a, b); }
        else { lm::shrink(tr); lm::shrink(with_pow); }
        value = with_pow.radius;                                                      // the radius of the pow form
        break;
      }
      case OP_BEFORE_STEP: decision = lm::converged_before_step(tr, a, b); break;     // a = gmax, b = gradient_tolerance
      case OP_PARAMETER: decision = lm::parameter_rule(a, b, c); break;               // step_norm, x_norm, tolerance
      case OP_FUNCTION: decision = lm::function_rule(a, b, c); break;                 // x_cost, cand_cost, tolerance
      case OP_DIAGONAL: value = lm::lm_diagonal(a, b); break;                         // h, radius
      case OP_JACOBI: value = lm::jacobi_scale(a); break;
      case OP_MODEL3: value = model_of<3>(a, b, c); break;
      case OP_MODEL6: value = model_of<6>(a, b, c); break;
      default: decision = -1.0;
    }
    double* o = out + kOut * k;
    o[0] = tr.radius; o[1] = tr.decrease_factor; o[2] = tr.invalid_steps; o[3] = tr.step_successful; o[4] = decision; o[5] = value;
    o[6] = lm::converged_before_step(tr, DBL_MAX, 0.0);
  }
}

__global__ __launch_bounds__(64) void k_selftest_lm_rules(int count, const double* __restrict__ rec, double* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) play(count, rec, out);
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_selftest_lm_rules(int32_t count, const double* records, double* device_out, double* host_out) {
  if (count < 1 || count > kMaxRecords) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!records || !device_out || !host_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<double> d_rec, d_out;
  if ((rc = d_rec.up(records, kIn * (size_t)count)) || (rc = d_out.alloc(kOut * (size_t)count))) return rc;
  k_selftest_lm_rules<<<1, 64, 0, nullptr>>>(count, d_rec.p, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(device_out, d_out.p, sizeof(double) * kOut * (size_t)count, hipMemcpyDeviceToHost));
  play(count, records, host_out);
  return 0;
}
