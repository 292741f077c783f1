// rotation_compose.h -- MultiplyRotations (math/rotation.cc:56-66) on the device, shared by the rotation stage's residual
// (rotation_averaging.hip) and the orientation filter (view_pair_filters.hip).
#ifndef THEIA_HIP_ROTATION_COMPOSE_H_
#define THEIA_HIP_ROTATION_COMPOSE_H_
#include "ransac_device.h"

namespace thip {

// MultiplyRotations(a, b): angle-axis -> matrices, product, matrix -> angle-axis (row-major matrices throughout)
__device__ __forceinline__ void multiply_rotations(const double* a, const double* b, double* out) {
  double Ra[9], Rb[9], R[9];
  rsc::angle_axis_to_rot(a, Ra);
  rsc::angle_axis_to_rot(b, Rb);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (Ra[3 * r] * Rb[c] + Ra[3 * r + 1] * Rb[3 + c]) + Ra[3 * r + 2] * Rb[6 + c];
  rsc::rot_to_angle_axis(R, out);
}

}  // namespace thip
#endif
