// ransac_internal.h -- what the RANSAC translation units share: ransac.hip (kernels, batch driver), ransac_streams.hip
// (streams entry point, theia_hip_rng_*) and ransac_solvers.hip (the directly bound minimal solvers).
#pragma once
#include <hip/hip_runtime.h>

#include <optional>

#include "dls_device.h"      // dlsdev::kMaxSolutions, dls::GlibcRand
#include "radial_homography_device.h"   // rsc::kRadHomDatum
#include "theia_hip.h"
#include "device_util.h"
#include "pools.h"
#include "ransac_rng.h"

namespace thip {

// ---- estimator tables
// models per sample an estimator can return = slot stride of the per-hypothesis arrays
__host__ __device__ inline int max_models(int est) {
  if (est == THEIA_EST_RADIAL_HOMOGRAPHY) return 2;
  if (est == THEIA_EST_SIMILARITY_2D3D) return dlsdev::kMaxSolutions;
  if (est == THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE) return 10;
  if (est == THEIA_EST_RIGID_TRANSFORMATION_2D3D) return 8;
  if (est == THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE) return 13;
  if (est == THEIA_EST_CAMERA_ALIGNMENT) return 1;   // EstimateModel always returns its one (possibly identity) model
  if (est >= THEIA_EST_FUNDAMENTAL_MATRIX) return 1;
  if (est == THEIA_EST_ABSOLUTE_POSE_DLS) return dlsdev::kMaxSolutions;
  return est == THEIA_EST_ABSOLUTE_POSE_SQPNP ? 18 : (est == THEIA_EST_ABSOLUTE_POSE_KNEIP ? 4 : 10);
}
constexpr int kStride = THEIA_RANSAC_MODEL_STRIDE;

__host__ __device__ inline int sample_size(int est) {
  switch (est) {
    case THEIA_EST_RELATIVE_POSE: case THEIA_EST_ESSENTIAL_MATRIX: return 5;
    case THEIA_EST_FUNDAMENTAL_MATRIX: case THEIA_EST_UNCALIBRATED_RELATIVE_POSE: return 8;
    case THEIA_EST_HOMOGRAPHY: case THEIA_EST_SIMILARITY_2D3D: case THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE:
    case THEIA_EST_RIGID_TRANSFORMATION_2D3D: case THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE:
    case THEIA_EST_CAMERA_ALIGNMENT: return 4;
    case THEIA_EST_RADIAL_HOMOGRAPHY: return 6;
    case THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION: case THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION:
    case THEIA_EST_TRIANGULATION: return 2;
    default: return 3;
  }
}
// meaningful doubles of a model row (layouts in theia_hip.h)
inline int model_doubles(int est) {
  switch (est) {
    case THEIA_EST_RELATIVE_POSE: return 21;
    case THEIA_EST_UNCALIBRATED_RELATIVE_POSE: return 23;
    case THEIA_EST_ABSOLUTE_POSE_KNEIP: case THEIA_EST_ABSOLUTE_POSE_DLS: case THEIA_EST_ABSOLUTE_POSE_SQPNP: return 12;
    case THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE: return 12;   // projection matrix, row-major 3 x 4
    case THEIA_EST_RIGID_TRANSFORMATION_2D3D: return 12;    // rotation | translation
    case THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE: return 14;   // rotation | translation | focal length | radial distortion
    case THEIA_EST_DOMINANT_PLANE: return 6;
    case THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION: case THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION: return 3;
    case THEIA_EST_TRIANGULATION: return 4;
    case THEIA_EST_RADIAL_HOMOGRAPHY: return 20;   // H | l1 | l2 | H^-1
    case THEIA_EST_SIMILARITY_2D3D: case THEIA_EST_CAMERA_ALIGNMENT: return 13;     // rotation | translation | scale
    default: return 9;   // essential / fundamental matrix, homography
  }
}
constexpr int kTriDatum = 33;   // PointObservation row of THEIA_EST_TRIANGULATION (theia_hip.h)
constexpr int kAlignDatum = 6;  // CameraCorrespondence row of THEIA_EST_CAMERA_ALIGNMENT: camera1 (3) | camera2 (3)
constexpr int kSimDatum = 26;   // CameraAndFeatureCorrespondence2D3D row of THEIA_EST_SIMILARITY_2D3D: dir (3) | point (4) | pixel (2) | extrinsics (6) | model | intrinsics (10)
__host__ __device__ inline int datum_size(int est) {
  switch (est) {
    case THEIA_EST_ABSOLUTE_POSE_KNEIP: case THEIA_EST_ABSOLUTE_POSE_DLS: case THEIA_EST_ABSOLUTE_POSE_SQPNP:
    case THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION: case THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE:
    case THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE: return 5;
    case THEIA_EST_DOMINANT_PLANE: return 3;
    case THEIA_EST_CAMERA_ALIGNMENT: return kAlignDatum;
    case THEIA_EST_TRIANGULATION: return kTriDatum;
    case THEIA_EST_RADIAL_HOMOGRAPHY: return rsc::kRadHomDatum;
    case THEIA_EST_SIMILARITY_2D3D: case THEIA_EST_RIGID_TRANSFORMATION_2D3D: return kSimDatum;
    default: return 4;
  }
}

// ---- the shared stream and a call's place on it (ransac.hip)
// The minimal-solver kernels need up to ~12 KB of scratch per lane; the runtime sizes a hardware queue's
// scratch arena for a full chip of such waves, and two queues asking for it at the same time end in
// HSA_STATUS_ERROR_OUT_OF_RESOURCES (queue abort).  Every RANSAC kernel of the process therefore goes to ONE stream
// (= one hardware queue, one arena), whichever host thread enqueues it: calls from a thread pool interleave their
// launches on it (each call owns its buffers, the stream keeps each call's own order) and wait for their OWN work
// through an event -- no host-side lock, nobody waits for another caller's synchronisation.
hipStream_t solver_stream();
// transfers that may run beside the solver stream's kernels (no kernel ever goes here: no scratch arena)
hipStream_t copy_stream();
struct CallSync {   // "my work on the shared stream is done"
  hipEvent_t e = nullptr;
  CallSync() { (void)hipEventCreateWithFlags(&e, hipEventDisableTiming); }
  ~CallSync() { if (e) (void)hipEventDestroy(e); }
  hipError_t wait(hipStream_t st) {
    hipError_t r = hipEventRecord(e, st);
    return r != hipSuccess ? r : hipEventSynchronize(e);
  }
};
// The prologue of every entry point that enqueues on the solver stream: device ready, the stream, the pool scope on it and
// the call's event.  Declared ahead of the call's buffers, so that they go back to the caches while the scope stands.
struct SolverCall {
  hipStream_t st = nullptr;
  std::optional<PoolStreamScope> pool_scope;   // blocks this call hands back to the caches are tagged with an event on this stream (pools.h)
  std::optional<CallSync> mine;
  int open() {
    const int rc = ensure_device();
    if (rc) return rc;
    st = solver_stream();
    pool_scope.emplace(st);
    if (!st) return set_error(THEIA_HIP_ERR_NO_DEVICE, "could not create the solver stream");
    mine.emplace();
    return 0;
  }
  hipError_t wait() { return mine->wait(st); }
};

// ---- the batch driver (ransac.hip)
// theia_hip_ransac_estimate_streams: the problems of one driver call are the head problems of their streams, one per stream
// (every problem starts where its stream stands).  gen[stream[p]] is the generator problem p starts from; the driver
// overwrites it with the generator after exactly num_iterations samples.  Per stream the P4Pfr first-call flag and (DLS /
// gDLS) the rand() stream positioned at the problem's first call.
struct StreamInit {
  Mt19937* gen;
  const int* stream;
  const uint8_t* p4pfr_first;
  const dls::GlibcRand* dls_start;   // NULL unless the estimator is DLS / gDLS
};
// the host driver of both entry points: si == NULL is the seeded batch (problem i: RandomNumberGenerator(seed + i))
int ransac_run(const theia_ransac_batch* batch, const theia_ransac_params* params, theia_ransac_result* result,
               const StreamInit* si);

inline int check_result_arrays(int nprob, const theia_ransac_result* result) {
  if (nprob > 0 && (!result->success || !result->models || !result->num_inliers || !result->inlier_mask ||
                    !result->num_iterations || !result->confidence))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null result array");
  return 0;
}
inline void reset_counters(theia_ransac_result* result) {
  result->hypotheses_evaluated = 0; result->models_scored = 0; result->time_fit_score_seconds = 0.0;
  result->time_fit_seconds = 0.0; result->time_score_seconds = 0.0;
}
// limits = {max focal length, min focal length, max distortion, min distortion}; the reference CHECKs these
// (four_point_focal_length_radial_distortion.cc:82-90)
inline int p4pfr_check_limits(const double* limits) {
  if (!(limits[1] >= 0.0 && limits[0] >= 0.0 && limits[0] >= limits[1] && limits[2] <= 0.0 && limits[3] <= 0.0 && limits[2] <= limits[3]))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "P4Pfr: needs 0 <= min focal length <= max focal length and max distortion <= min distortion <= 0");
  return 0;
}

// ---- launchers of kernels of ransac.hip that ransac_solvers.hip needs too
// P4Pf for B hypotheses of nprob problems: polynomial system -> eigen stage of the five-point solver -> projection
// matrices.  ws: [nprob * B][p4pf_workspace_doubles()], sol: [nprob * B][50], ok / mask: [nprob * B]
int p4pf_workspace_doubles();
int launch_p4pf_fit(int nprob, int B, const int64_t* offsets, const double* data, const int* samples, const int* active_iters,
                    double* ws, double* sol, int* ok, int* mask, double* models, int* counts, int* dense_count, int* tags,
                    int* hyp_base, hipStream_t st);
// the minimal solvers on whole problems, one thread each
void launch_five_point(int num, const double* corr, double* E, int* nsol, hipStream_t st);
void launch_p3p(int num, const double* corr, double* R, double* t, int* nsol, hipStream_t st);
void launch_sqpnp(int num, const int64_t* offsets, const double* feat, const double* world, double* quat, double* trans, int* nsol,
                  hipStream_t st);
void launch_dls_solve_b(int num, const int64_t* offsets, const double* world, const double* action, const double* tfac, const int* ok,
                        double* quat, double* trans, int* nsol, hipStream_t st);

}  // namespace thip
