// selftest_rotation_maps.hip -- test-only entry point for the rotation maps every global-pose stage starts and ends with
// (rotation_maps.h: angle_axis_to_rot, rot_to_angle_axis, eigen_rot_to_rotvec, multiply_rotations) on
// angle-axis vectors the caller chooses.  The kernel keeps the production launch shape of the stages that call them:
// 256-thread workgroups, one lane per case.  Nothing here runs on the estimation path.
#include "rotation_maps.h"
#include "device_util.h"

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kRecord = 18;   // per case: R(a) [9] row-major | rot_to_angle_axis(R) [3] | multiply_rotations(a, b) [3] | eigen_rot_to_rotvec(R) [3]

__global__ __launch_bounds__(kThreads) void k_selftest_rotation_maps(int count, const double* __restrict__ a,
                                                                     const double* __restrict__ b, double* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  double wa[3], wb[3], R[9], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { wa[k] = a[3 * (size_t)i + k]; wb[k] = b[3 * (size_t)i + k]; }
  double* o = out + kRecord * (size_t)i;
  rsc::angle_axis_to_rot(wa, R);
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  rsc::rot_to_angle_axis(R, v);
  o[9] = v[0]; o[10] = v[1]; o[11] = v[2];
  multiply_rotations(wa, wb, v);
  o[12] = v[0]; o[13] = v[1]; o[14] = v[2];
  rsc::eigen_rot_to_rotvec(R, v);
  o[15] = v[0]; o[16] = v[1]; o[17] = v[2];
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_selftest_rotation_maps(int32_t count, const double* a, const double* b, double* out) {
  if (count < 1 || count > (1 << 20)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "count = %d", count);
  if (!a || !b || !out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<double> d_a, d_b, d_out;
  const size_t rec = kRecord * (size_t)count;
  if ((rc = d_a.up(a, 3 * (size_t)count)) || (rc = d_b.up(b, 3 * (size_t)count)) || (rc = d_out.alloc(rec))) return rc;
  k_selftest_rotation_maps<<<grid_of(count, kThreads), kThreads, 0, nullptr>>>(count, d_a.p, d_b.p, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out.p, sizeof(double) * rec, hipMemcpyDeviceToHost));
  return 0;
}
