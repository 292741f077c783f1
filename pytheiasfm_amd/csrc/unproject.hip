// unproject.hip -- theia_hip_unproject: pixels -> camera points, normalised features and world rays for all eight camera
// models (Camera::PixelToNormalizedCoordinates, Camera::PixelToUnitDepthRay, camera.cc:218-230, over
// CameraIntrinsicsModel::ImageToCameraCoordinates, camera_intrinsics_model.cc:150-167).  The per-pixel function is
// unproject_device.h; this file must be compiled without FMA contraction (build.sh's default).
//
// k_unproject<MODELS>   one lane per observation, 256 per workgroup.  The lane reads its pixel (one 16 B load), its camera's
//                       intrinsics group and runs pixel_to_camera(): a per-lane switch over the model and, in the four iterative
//                       models, a per-lane loop whose lanes leave by their own break and then hold their value in registers
//                       while the wave's other lanes go on -- no cross-lane operation touches a result, so an observation's
//                       bytes do not depend on what shares its wave.  MODELS is the set of models the call's observations use:
//                       a call with one model (the usual data set) runs that model's instance, whose waves carry no other
//                       model's code or registers; a mixed call runs the instance with all eight.  Same source, same IEEE
//                       operations: the instances give the same bytes.
//                       world_ray = R' p with the angle-axis -> matrix routine of the BA kernels (rotation_terms, the
//                       small-angle branch of ceres::AngleAxisToRotationMatrix included), evaluated per observation.
//                       The summary's three counters are one wave reduction each and one integer atomic per wave.
#include "unproject_device.h"
#include "wave_reduce.h"
#include "device_util.h"

namespace thip {
namespace {

constexpr int kThreads = 256;

struct Counters { unsigned long long invalid, not_converged; unsigned max_trips; unsigned pad; };

template <unsigned MODELS>
__global__ __launch_bounds__(kThreads) void k_unproject(long long n, const double2* __restrict__ obs_uv,
                                                        const int* __restrict__ obs_cam, const int* __restrict__ cam_group,
                                                        const double* __restrict__ cam_ext, const double* __restrict__ intrinsics,
                                                        const int* __restrict__ group_model, double* __restrict__ camera_point,
                                                        double* __restrict__ normalized, double* __restrict__ world_ray,
                                                        double* __restrict__ world_ray_unit, uint8_t* __restrict__ status,
                                                        uint8_t* __restrict__ iterations, Counters* __restrict__ counters) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;
  int bad = 0, stuck = 0;
  unsigned trips = 0;
  if (live) {
    const double2 uv = obs_uv[i];
    const int c = obs_cam ? obs_cam[i] : 0;
    const int g = cam_group[c];
    Unprojected o;
    pixel_to_camera<MODELS>(group_model[g], intrinsics + (size_t)g * THEIA_MAX_INTRINSICS, uv.x, uv.y, o);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!o.valid) { o.p[0] = nan; o.p[1] = nan; o.p[2] = nan; }   // stated deviation: the reference returns an uninitialised vector
    bad = !o.valid;
    stuck = !o.converged;
    trips = (unsigned)o.trips;
    if (camera_point) {
      camera_point[3 * i] = o.p[0]; camera_point[3 * i + 1] = o.p[1]; camera_point[3 * i + 2] = o.p[2];
    }
    if (normalized) {   // .hnormalized()
      normalized[2 * i] = o.p[0] / o.p[2];
      normalized[2 * i + 1] = o.p[1] / o.p[2];
    }
    if (world_ray || world_ray_unit) {
      RotTerms t;
      rotation_terms(cam_ext + (size_t)c * 6 + 3, t);
      double w[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) w[j] = t.R[j] * o.p[0] + t.R[3 + j] * o.p[1] + t.R[6 + j] * o.p[2];   // R' p
      if (world_ray) { world_ray[3 * i] = w[0]; world_ray[3 * i + 1] = w[1]; world_ray[3 * i + 2] = w[2]; }
      if (world_ray_unit) {
        const double len = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        world_ray_unit[3 * i] = w[0] / len; world_ray_unit[3 * i + 1] = w[1] / len; world_ray_unit[3 * i + 2] = w[2] / len;
      }
    }
    if (status) status[i] = (uint8_t)((o.valid ? 1 : 0) | (o.converged ? 2 : 0));
    if (iterations) iterations[i] = (uint8_t)o.trips;
  }
  if (counters) {   // every lane of the wave takes part, the dead ones with zeros
    bad = wave_sum_butterfly(bad);
    stuck = wave_sum_butterfly(stuck);
    trips = wave_max_u32(trips);
    if ((threadIdx.x & 63) == 0) {
      if (bad) atomicAdd(&counters->invalid, (unsigned long long)bad);
      if (stuck) atomicAdd(&counters->not_converged, (unsigned long long)stuck);
      if (trips) atomicMax(&counters->max_trips, trips);
    }
  }
}

template <unsigned MODELS, class... Args>
void launch(long long n, Args... args) {
  k_unproject<MODELS><<<grid_of((size_t)n, kThreads), kThreads>>>(n, args...);
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_unproject(int64_t num_obs, const double* obs_uv, const int32_t* obs_cam, int32_t num_cameras,
                                   const int32_t* cam_group, const double* cam_ext, int32_t num_groups, const double* intrinsics,
                                   const int32_t* group_model, double* camera_point, double* normalized, double* world_ray,
                                   double* world_ray_unit, uint8_t* status, uint8_t* iterations,
                                   theia_unproject_summary* summary) {
  const auto t_call = std::chrono::steady_clock::now();
  if (num_obs < 0 || num_cameras < 0 || num_groups < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if ((num_obs > 0 && !obs_uv) || (num_cameras > 0 && !cam_group) || (num_groups > 0 && (!intrinsics || !group_model)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if ((world_ray || world_ray_unit) && num_obs > 0 && !cam_ext)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a world ray needs cam_ext");
  for (int g = 0; g < num_groups; ++g)
    if (group_model[g] < THEIA_CAM_PINHOLE || group_model[g] > THEIA_CAM_ORTHOGRAPHIC)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "group %d: camera model %d", g, (int)group_model[g]);
  for (int c = 0; c < num_cameras; ++c)
    if (cam_group[c] < 0 || cam_group[c] >= num_groups)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "camera %d: group %d out of range", c, (int)cam_group[c]);
  unsigned models = 0;   // the models the observations use
  if (obs_cam) {
    for (int64_t k = 0; k < num_obs; ++k) {
      if (obs_cam[k] < 0 || obs_cam[k] >= num_cameras)
        return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld: camera %d out of range", (long long)k, (int)obs_cam[k]);
      models |= 1u << group_model[cam_group[obs_cam[k]]];
    }
  } else if (num_obs > 0) {
    if (num_cameras < 1) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "obs_cam is NULL and there is no camera 0");
    models = 1u << group_model[cam_group[0]];
  }
  if (summary) *summary = theia_unproject_summary{};
  if (num_obs == 0) return 0;

  int rc = ensure_device();
  if (rc) return rc;
  const size_t n = (size_t)num_obs;
  DevBuf<double2> d_uv;
  DevBuf<int> d_cam, d_group, d_model;
  DevBuf<double> d_ext, d_intr, d_point, d_norm, d_ray, d_unit;
  DevBuf<uint8_t> d_status, d_iter;
  DevBuf<Counters> d_cnt;
  if ((rc = d_uv.up(obs_uv, n)) || (obs_cam && (rc = d_cam.up(obs_cam, n))) || (rc = d_group.up(cam_group, num_cameras)) ||
      (cam_ext && (rc = d_ext.up(cam_ext, (size_t)num_cameras * 6))) ||
      (rc = d_intr.up(intrinsics, (size_t)num_groups * THEIA_MAX_INTRINSICS)) || (rc = d_model.up(group_model, num_groups)) ||
      (camera_point && (rc = d_point.alloc(3 * n))) || (normalized && (rc = d_norm.alloc(2 * n))) ||
      (world_ray && (rc = d_ray.alloc(3 * n))) || (world_ray_unit && (rc = d_unit.alloc(3 * n))) ||
      (status && (rc = d_status.alloc(n))) || (iterations && (rc = d_iter.alloc(n))) || (summary && (rc = d_cnt.alloc(1))))
    return rc;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (summary) {
    HIP_TRY(hipMemset(d_cnt.p, 0, sizeof(Counters)));
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventRecord(ev0, nullptr));
  }
#define THIP_UNPROJECT_ARGS                                                                                             \
  (long long)num_obs, d_uv.p, d_cam.p, d_group.p, d_ext.p, d_intr.p, d_model.p, d_point.p, d_norm.p, d_ray.p, d_unit.p, \
      d_status.p, d_iter.p, d_cnt.p
  switch (models) {   // one model: its own instance
    case 1u << THEIA_CAM_PINHOLE: launch<1u << THEIA_CAM_PINHOLE>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL: launch<1u << THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_FISHEYE: launch<1u << THEIA_CAM_FISHEYE>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_FOV: launch<1u << THEIA_CAM_FOV>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_DIVISION_UNDISTORTION: launch<1u << THEIA_CAM_DIVISION_UNDISTORTION>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_DOUBLE_SPHERE: launch<1u << THEIA_CAM_DOUBLE_SPHERE>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_EXTENDED_UNIFIED: launch<1u << THEIA_CAM_EXTENDED_UNIFIED>(THIP_UNPROJECT_ARGS); break;
    case 1u << THEIA_CAM_ORTHOGRAPHIC: launch<1u << THEIA_CAM_ORTHOGRAPHIC>(THIP_UNPROJECT_ARGS); break;
    default: launch<kModelsAll>(THIP_UNPROJECT_ARGS); break;
  }
#undef THIP_UNPROJECT_ARGS
  hipError_t launched = hipGetLastError();
  float kernel_ms = 0.f;
  if (summary) {
    if (launched == hipSuccess) launched = hipEventRecord(ev1, nullptr);
    if (launched == hipSuccess) launched = hipEventSynchronize(ev1);
    if (launched == hipSuccess) launched = hipEventElapsedTime(&kernel_ms, ev0, ev1);
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
  }
  HIP_TRY(launched);
  if (camera_point) HIP_TRY(hipMemcpy(camera_point, d_point.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
  if (normalized) HIP_TRY(hipMemcpy(normalized, d_norm.p, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
  if (world_ray) HIP_TRY(hipMemcpy(world_ray, d_ray.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
  if (world_ray_unit) HIP_TRY(hipMemcpy(world_ray_unit, d_unit.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, d_status.p, n, hipMemcpyDeviceToHost));
  if (iterations) HIP_TRY(hipMemcpy(iterations, d_iter.p, n, hipMemcpyDeviceToHost));
  if (summary) {
    Counters h{};
    HIP_TRY(hipMemcpy(&h, d_cnt.p, sizeof(Counters), hipMemcpyDeviceToHost));
    summary->num_invalid = (int64_t)h.invalid;
    summary->num_not_converged = (int64_t)h.not_converged;
    summary->max_iterations = (int32_t)h.max_trips;
    summary->kernel_ms = kernel_ms;
    summary->call_ms = ms_since(t_call);
  }
  return 0;
}
