/*
 * theia_hip.h -- C-ABI of the MI355X (gfx950) bundle-adjustment + RANSAC engine.
 *
 * This is the drop-in boundary: plain C structs of pointers and sizes, no
 * Eigen / STL / torch types.  Every entry point names the reference interface
 * (pyTheiaSfM, paths relative to the reference root) that it replaces.  The
 * reference-side shim (flatten Reconstruction -> call -> scatter back) is shown
 * in INTEGRATION.md.
 *
 * All floating point data is IEEE FP64.  All index data is int32 unless noted.
 * Return value of every function: 0 = THEIA_HIP_OK, negative = error code;
 * the library never throws and never aborts.  theia_hip_last_error() returns a
 * thread-local human-readable message for the last failing call.
 */
#ifndef THEIA_HIP_H_
#define THEIA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
enum {
  THEIA_HIP_OK = 0,
  THEIA_HIP_ERR_INVALID_ARGUMENT = -1, /* reference: glog CHECK -> abort        */
  THEIA_HIP_ERR_NO_DEVICE = -2,        /* no gfx950 device / HIP runtime error  */
  THEIA_HIP_ERR_UNSUPPORTED = -3,      /* option combination not built yet      */
  THEIA_HIP_ERR_OUT_OF_MEMORY = -4,
  THEIA_HIP_ERR_INTERNAL = -5
};

int theia_hip_init(int device_ordinal);
int theia_hip_shutdown(void);
int theia_hip_device_count(int* count);
const char* theia_hip_last_error(void);
const char* theia_hip_version(void);

/* ------------------------------------------------------- camera model enums */
/* src/theia/sfm/camera/camera_intrinsics_model_type.h:46-56 */
enum {
  THEIA_CAM_PINHOLE = 0,
  THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL = 1,
  THEIA_CAM_FISHEYE = 2,
  THEIA_CAM_FOV = 3,
  THEIA_CAM_DIVISION_UNDISTORTION = 4,
  THEIA_CAM_DOUBLE_SPHERE = 5,
  THEIA_CAM_EXTENDED_UNIFIED = 6,
  THEIA_CAM_ORTHOGRAPHIC = 7
};
#define THEIA_MAX_INTRINSICS 10 /* largest kIntrinsicsSize (radial-tangential) */

/* src/theia/sfm/bundle_adjustment/create_loss_function.h:52-60 */
enum {
  THEIA_LOSS_TRIVIAL = 0,
  THEIA_LOSS_HUBER = 1,
  THEIA_LOSS_SOFTLONE = 2,
  THEIA_LOSS_CAUCHY = 3,
  THEIA_LOSS_ARCTAN = 4,
  THEIA_LOSS_TUKEY = 5,
  THEIA_LOSS_TRUNCATED = 6
};

/* src/theia/sfm/bundle_adjustment/bundle_adjustment.h:71-85 (bitmask) */
enum {
  THEIA_INTR_NONE = 0x00,
  THEIA_INTR_FOCAL_LENGTH = 0x01,
  THEIA_INTR_ASPECT_RATIO = 0x02,
  THEIA_INTR_SKEW = 0x04,
  THEIA_INTR_PRINCIPAL_POINTS = 0x08,
  THEIA_INTR_RADIAL_DISTORTION = 0x10,
  THEIA_INTR_TANGENTIAL_DISTORTION = 0x20,
  THEIA_INTR_ALL = 0x3f
};

/* per-camera constant mask bits (what BundleAdjuster freezes):
 *   bundle_adjuster.cc:477-518 SetCameraExtrinsicsConstant / PositionConstant /
 *   OrientationConstant / SetTzConstant. */
enum {
  THEIA_CAM_CONST_POSITION = 0x1,
  THEIA_CAM_CONST_ORIENTATION = 0x2,
  THEIA_CAM_CONST_ALL = 0x3,
  THEIA_CAM_CONST_TZ = 0x4
};

/* ------------------------------------------------------------ BA problem IR */
/*
 * Flattened form of what BundleAdjuster::AddView/AddTrack build inside Ceres
 * (bundle_adjuster.cc:116-221): one 2-residual block per (estimated view,
 * estimated track) observation; raw parameter blocks
 *   camera extrinsics  [position(3) | angle-axis(3)]   camera.h:202-204,251
 *   shared intrinsics  [K doubles per intrinsics group] camera_intrinsics_model.h
 *   homogeneous point  [x y z w]                        track.h:66,110
 * Parameters are updated IN PLACE (as Ceres writes through the borrowed
 * double* of the Reconstruction, bundle_adjuster.cc:585-591).
 * Caller owns every buffer; nothing is retained after a call returns unless a
 * handle was created, and a handle owns device copies only.
 */
/* problem flags: a track shard of a multi-GPU solve keeps every non-constant
 * camera in the reduced system (also those it does not observe) so that all
 * ranks index the reduced camera system identically. */
enum { THEIA_BA_FLAG_KEEP_UNOBSERVED_CAMERAS = 0x1, THEIA_BA_FLAG_INVERSE_DEPTH = 0x2 };

typedef struct theia_ba_problem {
  int32_t num_cameras;
  int32_t num_groups;
  int32_t num_points;
  int32_t flags;               /* THEIA_BA_FLAG_* */
  int64_t num_obs;

  double* cam_ext;             /* [num_cameras][6]  in/out */
  double* intrinsics;          /* [num_groups][THEIA_MAX_INTRINSICS] in/out */
  const int32_t* group_model;  /* [num_groups] THEIA_CAM_*                 */
  const int32_t* cam_group;    /* [num_cameras] intrinsics group of camera */
  const uint8_t* cam_const;    /* [num_cameras] THEIA_CAM_CONST_* bits, or NULL */
  const uint8_t* group_const;  /* [num_groups] 1 = whole block constant, or NULL
                                  (bundle_adjuster.cc:444-459)             */
  double* points;              /* [num_points][4]  in/out */
  const uint8_t* point_const;  /* [num_points] 1 = SetTrackConstant, or NULL */

  const double* obs_uv;        /* [num_obs][2] Feature::point_             */
  const double* obs_sqrt_info; /* [num_obs][2] 1/sqrt(cov_xx), 1/sqrt(cov_yy)
                                  (reprojection_error.h:94-99) or NULL = 1 */
  const int32_t* obs_cam;      /* [num_obs] camera index                   */
  const int32_t* obs_pt;       /* [num_obs] point index                    */
  /* Camera priors (View::{Position,Gravity,Orientation}Prior added by AddView / AddViewPriors,
   * bundle_adjuster.cc:159-172,291-313; functors position_error.h, gravity_error.h,
   * orientation_error.h: 3 residuals each, no loss).  All optional (NULL); a prior is used when its
   * bit is set both in cam_prior_mask[c] and in options->prior_mask.  Sharded solves: pass the
   * priors on exactly ONE rank (cameras are replicated). */
  const uint8_t* cam_prior_mask;                 /* [num_cameras] THEIA_PRIOR_* bits           */
  const double* cam_position_prior;              /* [num_cameras][3]                           */
  const double* cam_position_prior_sqrt_info;    /* [num_cameras][3][3] row-major              */
  const double* cam_gravity_prior;               /* [num_cameras][3] gravity in the camera frame */
  const double* cam_gravity_prior_sqrt_info;     /* [num_cameras][3][3]                        */
  const double* cam_orientation_prior;           /* [num_cameras][3] angle-axis                */
  const double* cam_orientation_prior_sqrt_info; /* [num_cameras][3][3]                        */
  /* Depth priors (BundleAdjuster::AddDepthPriorErrorResidual, bundle_adjuster.cc:154-156,643-650;
   * DepthPriorError, depth_prior_error.h): every feature with depth_prior != 0 of a solve with
   * use_depth_priors contributes ONE more residual block on (extrinsics, point),
   *   d = (R (X - w C))_z - depth_prior,  weighted by 1 / sqrt(depth_prior_variance),
   * under its own loss (options.robust_loss_width_depth_prior).  Here such a block is one more
   * OBSERVATION ROW of kind THEIA_OBS_DEPTH_PRIOR on the same camera and point:
   *   obs_uv = (depth_prior, 0), obs_sqrt_info = (1 / sqrt(variance), any) (obs_sqrt_info then required).
   * NULL = every row is a reprojection error. */
  const uint8_t* obs_kind;                       /* [num_obs] THEIA_OBS_* or NULL              */
  /* Inverse-depth parametrisation (BundleAdjustmentOptions::use_inverse_depth_parametrization; BundleAdjuster::AddInvTrack,
   * bundle_adjuster.cc:223-289; functors camera/reprojection_error.h:173-286): with THEIA_BA_FLAG_INVERSE_DEPTH the
   * variable of track t is point_inverse_depth[t] = Track::InverseDepth() along point_ref_bearing[t] =
   * Track::ReferenceBearingVector() in the frame of view point_ref_cam[t] = Track::ReferenceViewId(); `points` is not
   * read (the caller's UpdateHomogeneousPoint rebuilds it afterwards, bundle_adjustment.cc:47-65).  Every residual block
   * touches the reference camera, the observing camera, the intrinsics group of the observing camera
   * (bundle_adjuster.cc:594-622; optimised on the subset of options.intrinsics_to_optimize unless group_const) and the
   * inverse depth; the camera priors enter as AddViewPriors adds them (bundle_adjuster.cc:289-313: the views that observe
   * a track or are the reference view of one).  Through theia_hip_ba_solve and the handle API (create / reset_parameters /
   * set_options / run / download; covariance, evaluation and sharding: THEIA_HIP_ERR_UNSUPPORTED); no depth rows / inner
   * iterations in this mode; a track may be observed through at most 8 variable intrinsics groups (ERR_UNSUPPORTED beyond).
   * REFERENCE PARITY: the reference's BundleAdjust*Reconstruction entry points never optimise intrinsics in this mode
   * (only AddInvTrack runs, no view enters optimized_camera_intrinsics_groups_: bundle_adjuster.cc:441-459), so a caller
   * that mirrors them passes options.intrinsics_to_optimize = 0 (the Python mirror does). */
  const int32_t* point_ref_cam;                  /* [num_points] camera index of the reference view */
  const double* point_ref_bearing;               /* [num_points][3]                                 */
  double* point_inverse_depth;                   /* [num_points] in/out, > 0                        */
} theia_ba_problem;
enum { THEIA_PRIOR_POSITION = 1, THEIA_PRIOR_GRAVITY = 2, THEIA_PRIOR_ORIENTATION = 4 };
enum { THEIA_OBS_REPROJECTION = 0, THEIA_OBS_DEPTH_PRIOR = 1 };

/* Mirrors BundleAdjustmentOptions (bundle_adjustment.h:87-167), the fields the
 * HIP backend honours.  The linear-algebra selector fields of the reference
 * struct have no counterpart: this backend IS the linear solver. */
typedef struct theia_ba_options {
  int32_t loss_function_type;    /* THEIA_LOSS_*                  (:90) */
  int32_t intrinsics_to_optimize;/* THEIA_INTR_* bitmask          (:135) */
  int32_t max_num_iterations;    /*                               (:138) */
  int32_t use_homogeneous_point_parametrization; /* SphereManifold<4> (:127) */
  int32_t constant_camera_orientation;           /* (:122) */
  int32_t constant_camera_position;              /* (:123) */
  int32_t orthographic_camera;                   /* (:163) tz constant */
  int32_t use_inner_iterations;  /* (:144) accepted, see DESIGN.md deviation */
  int32_t verbose;               /* (:118) per-iteration table on stderr */
  int32_t prior_mask;            /* THEIA_PRIOR_* bits: use_position_priors (:154), use_gravity_priors (:166),
                                    use_orientation_priors (:157) */
  double robust_loss_width;      /* (:91) */
  double function_tolerance;     /* (:148) */
  double gradient_tolerance;     /* (:149) */
  double parameter_tolerance;    /* (:150) */
  double max_trust_region_radius;/* (:151) */
  double max_solver_time_in_seconds; /* (:141) */
  double robust_loss_width_depth_prior; /* (:94) width of the loss on THEIA_OBS_DEPTH_PRIOR rows */
} theia_ba_options;

void theia_ba_options_default(theia_ba_options* o);

/* termination_type values (ceres::TerminationType order) */
enum {
  THEIA_TERM_CONVERGENCE = 0,
  THEIA_TERM_NO_CONVERGENCE = 1,
  THEIA_TERM_FAILURE = 2
};

/* Mirrors BundleAdjustmentSummary (bundle_adjustment.h:170-178) plus the
 * per-iteration trace used for parity checking against the oracle. */
typedef struct theia_ba_summary {
  int32_t success;               /* IsSolutionUsable() (bundle_adjuster.cc:352) */
  int32_t termination_type;
  int32_t num_iterations;        /* LM iterations run (successful + rejected)   */
  int32_t num_successful_steps;
  double initial_cost;
  double final_cost;
  double setup_time_in_seconds;
  double solve_time_in_seconds;
  /* optional trace, caller-allocated arrays of trace_capacity entries each
   * (entry 0 = iteration 0), NULL to skip */
  int32_t trace_capacity;
  int32_t trace_size;
  double* trace_cost;
  double* trace_gradient_max_norm;
  double* trace_step_norm;
  double* trace_radius;
  int32_t* trace_accepted;
  /* time spent per phase (seconds, device-side events): linearize+Schur,
   * reduced solve, back-substitution+trial cost */
  double time_linearize;
  double time_solve_reduced;
  double time_backsub;
  /* the dominant kernel alone (ba_linearize_schur), HIP events on its stream */
  double time_kernel_linearize;
  int32_t num_linearize_launches;
  int32_t reserved1;
} theia_ba_summary;

/* One-shot solve: replaces BundleAdjuster::Optimize -> ceres::Solve
 * (bundle_adjuster.cc:315-355) for the problem built by
 * BundleAdjustReconstruction / BundleAdjustPartialReconstruction /
 * BundleAdjustPartialViewsConstant (bundle_adjustment.cc:111-217). */
int theia_hip_ba_solve(const theia_ba_problem* problem,
                       const theia_ba_options* options,
                       theia_ba_summary* summary);

/* A batch of INDEPENDENT single-view adjustments: problem i optimises the 6
 * extrinsics cam_ext[i] against its observations [offsets[i], offsets[i+1]) of
 * CONSTANT homogeneous world points, i.e. N calls of
 * BundleAdjustView(options, view_id, reconstruction) (bundle_adjustment.cc:220-237;
 * camera localisation, and RefineModel of the absolute-pose estimator,
 * estimate_calibrated_absolute_pose.cc:120-153) as one launch: one whole LM solve
 * per wavefront, no host round trips.  Honoured options: loss type / width,
 * max_num_iterations, the three tolerances, max_trust_region_radius,
 * constant_camera_{orientation,position}, orthographic_camera.  summaries[i]
 * receives success / termination / iterations / initial / final cost (no trace). */
typedef struct theia_ba_view_batch {
  int32_t num_problems;
  const int64_t* offsets;        /* [num_problems+1] observation offsets, offsets[0] = 0 */
  const double* obs_uv;          /* [total][2] pixels                          */
  const double* obs_sqrt_info;   /* [total][2] or NULL (= 1, 1)                */
  const double* points;          /* [total][4] homogeneous world point of each observation */
  double* cam_ext;               /* [num_problems][6] in/out                   */
  const double* intrinsics;      /* [num_problems][THEIA_MAX_INTRINSICS]       */
  const int32_t* model;          /* [num_problems] THEIA_CAM_*                 */
  const uint8_t* cam_const;      /* [num_problems] THEIA_CAM_CONST_* bits or NULL */
} theia_ba_view_batch;
int theia_hip_ba_views_batch(const theia_ba_view_batch* batch,
                             const theia_ba_options* options,
                             theia_ba_summary* summaries);

/* A batch of INDEPENDENT two-view bundle adjustments: N calls of BundleAdjustTwoViews(options, correspondences,
 * &camera1, &camera2, &points) (bundle_adjust_two_views.cc:110-185; the refinement step of
 * TwoViewMatchGeometricVerification::VerifyMatches, two_view_match_geometric_verification.cc:259-289) as one launch, one
 * LM solve per wavefront.  Camera 1 is held constant, camera 2 moves, the focal length of a camera moves unless
 * const_intrinsics says otherwise (lower bound 1), the points move as XYZW vectors without a manifold; reprojection
 * residuals in both views, trivial loss, Ceres' solver defaults as that function sets them (no inner iterations; pass
 * max_trust_region_radius = 1e16).  Honoured options: max_num_iterations, the three tolerances,
 * max_trust_region_radius.  The same arithmetic as theia_hip_ba_solve on the same flat problem. */
typedef struct theia_ba_two_view_full_batch {
  int32_t num_problems;
  const int64_t* offsets;          /* [num_problems+1] correspondence offsets, offsets[0] = 0            */
  const double* correspondences;   /* [total][4] = (x1, y1, x2, y2) pixels                                */
  double* cam_ext;                 /* [num_problems][2][6]: camera 1 (constant), camera 2 (in/out)       */
  double* intrinsics;              /* [num_problems][2][THEIA_MAX_INTRINSICS]; the focal lengths in/out  */
  const int32_t* model;            /* [num_problems][2] THEIA_CAM_*                                      */
  const uint8_t* const_intrinsics; /* [num_problems][2] 1 = the camera's focal length is held constant   */
  double* points;                  /* [total][4] XYZW of every correspondence, in/out                    */
} theia_ba_two_view_full_batch;
int theia_hip_ba_two_views_batch(const theia_ba_two_view_full_batch* batch, const theia_ba_options* options,
                                 theia_ba_summary* summaries);

/* A batch of INDEPENDENT two-view angular adjustments: problem i refines the relative
 * rotation (angle-axis) and the unit position of view 2 against the angular epipolar
 * error of its correspondences [offsets[i], offsets[i+1]), i.e. N calls of
 * BundleAdjustTwoViewsAngular(options, correspondences, &info)
 * (bundle_adjust_two_views.cc:189-246, residual angular_epipolar_error.h:54-91, bound at
 * src/pytheia/sfm/sfm.cc:1620) -- also RefineModel of the relative-pose estimator
 * (estimate_relative_pose.cc:111-138).  The position moves on SphereManifold<3>; the
 * linear solver is selected by linear_solver: EXACT = the solution of the 5 x 5 normal
 * equations (any direct BundleAdjustmentOptions::linear_solver_type, the default), CGNR =
 * conjugate gradients with the JACOBI preconditioner and Ceres' q-tolerance rule, an
 * inexact step (what the relative-pose RefineModel selects).
 * Honoured options: loss type / width, max_num_iterations, the three tolerances,
 * max_trust_region_radius.  Normalised image coordinates. */
enum { THEIA_TWO_VIEW_EXACT = 0, THEIA_TWO_VIEW_CGNR = 1 };
typedef struct theia_ba_two_view_batch {
  int32_t num_problems;
  int32_t linear_solver;           /* THEIA_TWO_VIEW_*                                       */
  const int64_t* offsets;          /* [num_problems+1], offsets[0] = 0                      */
  const double* correspondences;   /* [total][4] = (x1, y1, x2, y2)                          */
  double* rotation_position;       /* [num_problems][6] in/out: TwoViewInfo::rotation_2 | position_2 */
} theia_ba_two_view_batch;
int theia_hip_ba_two_views_angular_batch(const theia_ba_two_view_batch* batch,
                                         const theia_ba_options* options,
                                         theia_ba_summary* summaries);

/* A batch of INDEPENDENT homography refinements = N calls of OptimizeHomography(options,
 * correspondences, &homography) (bundle_adjust_two_views.cc:298-358; RefineModel of the homography
 * estimator, estimate_homography.cc:89-104): the nine entries of H against the symmetric geometric
 * distance (homography_error.h:45-95: H x1 - x2 and H^-1 x2 - x1, four residuals under one loss),
 * direct linear solver, result divided by H(2,2).  homographies [num_problems][9] row-major in/out;
 * correspondences [total][4] = (x1, y1, x2, y2).  Honoured options as for the two-view batch. */
int theia_hip_optimize_homography_batch(int32_t num_problems, const int64_t* offsets,
                                        const double* correspondences, double* homographies,
                                        const theia_ba_options* options,
                                        theia_ba_summary* summaries);

/* N calls of OptimizeRelativePositionWithKnownRotation(correspondences, rotation1, rotation2, &relative_position)
 * (bundle_adjustment/optimize_relative_position_with_known_rotation.cc:116-191; pybind sfm.cc:1621-1622; called once per
 * view pair from a thread pool by RefineRelativeTranslationsWithKnownRotations, reconstruction_estimator_utils.cc:263-291):
 * the IRLS null-vector solve on the epipolar constraints with both rotations known, at most 100 iterations, sign by the
 * cheirality majority.  One pair per wavefront (csrc/relpos_irls.hip).  correspondences [total][4] = normalised
 * (x1, y1, x2, y2); rotations [num_problems][6] = rotation1 | rotation2 as angle-axis (world -> camera, as
 * Camera::GetOrientationAsAngleAxis); relative_positions [num_problems][3] out (unit vectors; the reference returns true
 * always); num_iterations [num_problems] optional out.  An empty pair yields (0, 0, -1) like the reference's arithmetic. */
int theia_hip_optimize_relative_position_batch(int32_t num_problems, const int64_t* offsets,
                                               const double* correspondences, const double* rotations,
                                               double* relative_positions, int32_t* num_iterations);

/* N calls of OptimizeFundamentalMatrix(options, correspondences, &F) (bundle_adjust_two_views.cc:248-296;
 * RefineModel of the fundamental-matrix estimator, estimate_fundamental_matrix.cc:53-90): F moves on the
 * 7-dof manifold of fundamental_matrix_parameterization.h:15-75 (Plus through the SVD of the current F:
 * every accepted step re-normalises F to singular values (1, sigma, 0)) against one squared-Sampson
 * residual per correspondence (sampson_error.h:21-33); no loss function (options->loss_function_type
 * must be TRIVIAL), direct solver.  fundamental_matrices [num_problems][9] row-major in/out.
 * A problem with no correspondences has a parameter block and no residual block: like Ceres (which drops the
 * unused block: "no non-constant parameter blocks"; Ceres 2.2's rule as recalled, its source is not part of this
 * tree) it ends at once with CONVERGENCE, success = 1, 0 iterations,
 * both costs 0 and F untouched (not renormalised), as the angular and homography entries do. */
int theia_hip_optimize_fundamental_matrix_batch(int32_t num_problems, const int64_t* offsets,
                                                const double* correspondences, double* fundamental_matrices,
                                                const theia_ba_options* options,
                                                theia_ba_summary* summaries);

/* Every point of `problem` as its OWN problem with all cameras constant: N calls of
 * BundleAdjustTrack(options, track_id, reconstruction) (bundle_adjustment.cc:262-285; the
 * per-track refinement after triangulation, estimate_track.cc:289) in one launch, one thread
 * per track running its whole LM.  problem->points is updated in place; points flagged in
 * point_const (or without observations) are left alone.  summaries[num_points]. */
int theia_hip_ba_tracks_batch(const theia_ba_problem* problem,
                              const theia_ba_options* options,
                              theia_ba_summary* summaries);

/* Per-track reprojection sweep = the loop body of SetOutlierTracksToUnestimated
 * (set_outlier_tracks_to_unestimated.cc:64-139; the same residual as the BA, without Jacobians): for
 * every point of `problem` over its observations: the mean squared (unweighted) reprojection error, the
 * number of views that see it at negative depth (Camera::ProjectPoint), and the smallest cosine between
 * two of its viewing rays (SufficientTriangulationAngle, triangulation.cc:236-250: a track passes when
 * that cosine is below cos(min_angle); 2.0 when it has fewer than two views).  One thread per track. */
int theia_hip_track_statistics(const theia_ba_problem* problem,
                               double* mean_sq_reprojection_error,
                               int32_t* num_behind_camera,
                               double* min_ray_cosine);

/* TrackEstimator::EstimateTrack (estimate_track.cc:206-319) for every point of `problem` that is
 * not flagged in point_const.  With triangulation_method = MIDPOINT (the default, estimate_track.h:82):
 *   1. fewer than two observations, or no pair of viewing rays further apart than
 *      min_triangulation_angle_degrees (SufficientTriangulationAngle, triangulation.cc:236-250) -> bad angle;
 *   2. TriangulateMidpoint (triangulation.cc:130-157): sum (I - d d^T) X = sum (I - d d^T) o, Cholesky;
 *      not positive definite -> failed triangulation; the point becomes (X, 1);
 *      SVD / L2_MINIMIZATION: TriangulateNViewSVD / TriangulateNView (triangulation.cc:178-214) on the pixels and
 *      Camera::GetProjectionMatrix of every observation (computed here from the extrinsics and the model's focal length,
 *      aspect ratio, skew and principal point); the homogeneous point is defined up to sign, as in the reference;
 *   3. bundle_adjustment: BundleAdjustTrack on that point (= theia_hip_ba_tracks_batch), !success -> rejected;
 *   4. AcceptableReprojectionError (estimate_track.cc:93-117): any view with Camera::ProjectPoint < 0, or a mean
 *      squared reprojection error >= max_acceptable_reprojection_error_pixels^2 -> bad reprojection.
 * One thread per track for every stage.  obs_ray_dir[num_obs][3] = Camera::PixelToUnitDepthRay(feature).normalized()
 * of each observation (the caller's camera classes undistort; estimate_track.cc:76-77), origins are the camera
 * positions.  problem->points is written for every track that reached stage 2 (as the reference writes
 * track->MutablePoint() before it knows the outcome).  estimated[num_points]: 1 = SetEstimated(true).
 * counters: {bad angles, failed triangulations, bad reprojections, rejected by the track BA}. */
typedef struct theia_track_estimate_options {
  double min_triangulation_angle_degrees;           /* estimate_track.h:69, default 3.0 */
  double max_acceptable_reprojection_error_pixels;  /* :64, default 5.0 */
  int32_t bundle_adjustment;                        /* :73, default 1 */
  int32_t triangulation_method;                     /* :82, TriangulationMethodType: 0 MIDPOINT (default), 1 SVD, 2 L2_MINIMIZATION */
} theia_track_estimate_options;
int theia_hip_estimate_tracks(const theia_ba_problem* problem, const double* obs_ray_dir,
                              const theia_ba_options* ba_options,
                              const theia_track_estimate_options* options,
                              uint8_t* estimated, int32_t counters[4]);

/* Handle API: problem resident in HBM across calls (bench, repeated solves).  Problems with THEIA_BA_FLAG_INVERSE_DEPTH
 * support create / reset_parameters / set_options / run / download / destroy (the other calls return ERR_UNSUPPORTED). */
typedef struct theia_ba_handle_s* theia_ba_handle;
int theia_hip_ba_create(const theia_ba_problem* problem,
                        const theia_ba_options* options, theia_ba_handle* out);
int theia_hip_ba_reset_parameters(theia_ba_handle h,
                                  const theia_ba_problem* problem);
/* Device-resident copy of the handle's current parameters (cameras, points,
 * intrinsics), and the way back: repeated solves from the same start without a
 * host round trip (bench.py: the timed region starts with its inputs in HBM). */
/* Optional, sharded solves: this rank's index and the number of ranks of the
 * all-reduce group.  With it the MAX-reduced scalar (gradient max-norm) rides in
 * the SUM all-reduce of the reduced camera system (one slot per rank), saving one
 * collective per LM iteration; without it a separate MAX all-reduce is issued. */
int theia_hip_ba_set_shard(theia_ba_handle h, int32_t rank, int32_t world_size);
int theia_hip_ba_snapshot_parameters(theia_ba_handle h);
int theia_hip_ba_restore_parameters(theia_ba_handle h);
/* Replace the solver-control options of a handle (iteration cap, tolerances,
 * loss, radius cap, verbosity).  Options that shape the problem
 * (parametrisation, constant-camera switches, intrinsics mask) must equal the
 * ones given to create(), else THEIA_HIP_ERR_INVALID_ARGUMENT. */
int theia_hip_ba_set_options(theia_ba_handle h, const theia_ba_options* options);
int theia_hip_ba_run(theia_ba_handle h, theia_ba_summary* summary);
int theia_hip_ba_download(theia_ba_handle h, theia_ba_problem* problem);
int theia_hip_ba_destroy(theia_ba_handle h);

/* Shape of the device plan of a handle, for roofline accounting (bench.py): reduced system size, elimination-tree
 * levels and FP64 flops of one reduced-camera solve (K3), workgroups ("runs") of the fused linearise + Schur kernel
 * (0 = the gather kernels are in use), tracks on the per-observation slow path.  Any pointer may be NULL. */
int theia_hip_ba_plan_info(theia_ba_handle h, int32_t* n, int32_t* k3_levels, double* k3_flops, int32_t* fused_runs,
                           int32_t* slow_path_tracks);

/* Which kernel instances a run() of the handle dispatches to, for the tests: one line of text per kernel family, for
 * example "k_lin_schur pd=3 models=all lossk=2 first=0" or "k_lin_schur_i pd=4 models=notrig lossk=0 bw=13 kmask=0",
 * NUL-terminated in buf[cap].  The values come from the host functions the launch sites themselves branch on.
 * THEIA_HIP_ERR_INVALID_ARGUMENT when cap is too small. */
int theia_hip_ba_kernel_instances(theia_ba_handle h, char* buf, int32_t cap);

/* DIAGNOSTIC, for the tests only (like theia_hip_ba_kernel_instances; no caller needs it to solve anything).
 * Which launches a run() of the handle takes between the large kernels of an LM iteration: *folded = 1 when
 * its bodies after the first take the folded chain (k_schur_sum finishes the reduced system, k_cam_update and the control
 * kernel clear it), 0 when every body keeps the separate launches.  The value is the one run() branches on,
 * from the handle, its options and the environment (THEIA_HIP_LM_GLUE_KERNELS=1 keeps the separate launches).
 * Note: a handle CREATED with use_inner_iterations != 0 carries the inner-iteration lists and keeps the separate launches
 * even after theia_hip_ba_set_options switched the inner iterations off (its per-camera blocks are rebuilt every
 * iteration); create the handle with use_inner_iterations = 0 to get the folded chain. */
int theia_hip_ba_lm_chain(theia_ba_handle h, int32_t* folded);


/* Covariance blocks at the handle's current state for the two block-diagonal problems behind the
 * *WithCov entry points (bundle_adjustment.cc:288-386,420-499; GetCovarianceFor{Track,Tracks,View,Views},
 * bundle_adjuster.cc:660-773 = ceres::Covariance (J'J)^-1 in tangent space, loss applied):
 *   point_cov[num_points][d][d], d = 3 (homogeneous manifold) or 4: needs every camera constant;
 *   cam_cov[num_cameras][6][6]: needs every point constant and no partially constant camera.  With optimised intrinsics
 *   the cameras of a group are coupled through the group's columns: the extrinsics blocks of the dense inverse of J'J are
 *   returned (reduced systems up to 2048 columns: a *WithCov call covers a handful of views).
 * Either pointer may be NULL.  Entries of constant / unobserved blocks are zero.  NOT yet multiplied
 * by the empirical variance factor 2 * final_cost / redundancy (the caller's bookkeeping). */
int theia_hip_ba_covariance(theia_ba_handle h, double* point_cov, double* cam_cov);

/* Covariance blocks of a problem in which cameras and points are BOTH free: what BundleAdjuster::GetCovarianceForTrack(s)
 * and GetCovarianceForView(s) (bundle_adjuster.cc:660-773) return when ceres::Covariance is handed the coupled problem of
 * BundleAdjustReconstruction / BundleAdjustPartialReconstruction.  The result is the camera (6 x 6) and point (d x d)
 * diagonal blocks of (J'J)^-1 at the handle's current state, with EVERY variable block in J -- camera extrinsics, the free
 * intrinsics of variable groups, points -- J being the loss-corrected, unscaled Jacobian in tangent space with the
 * camera-prior and depth-prior rows included.  With H = J'J = [U W; W' V] and S = U - W V^-1 W':
 *   cam_cov[c]   = [S^-1]_cc,
 *   point_cov[p] = V_p^-1 + V_p^-1 (sum over the observations a, b of p: W_ap' [S^-1]_ab W_bp) V_p^-1.
 * view_sel / track_sel: camera / point indices whose blocks are wanted, NULL = all of them; only the columns of S^-1 these
 * need are solved for, at most max_rhs_columns unit vectors at a time (0 = chosen by the library).
 * cam_cov [num_cameras][6][6], point_cov [num_points][d][d], either may be NULL.  Blocks that are not selected, constant
 * or unobserved are zero.  NOT multiplied by the empirical variance factor.
 * Deviations from the reference, and limits:
 *  - a partially constant camera (cam_const 1 or 2) comes back as the ambient 6 x 6 with zero rows and columns at its
 *    frozen parameters; Ceres returns the (6 - k)-sized tangent block, which the reference writes into a Matrix6d unpadded;
 *  - a pivot that is not positive, in a point block or in S, returns THEIA_HIP_ERR_INTERNAL ("rank deficient
 *    (ceres::Covariance::Compute fails)").  A point block's pivot below 1e-13 of its diagonal entry counts as not positive
 *    (a track with one observation, an un-parametrised homogeneous point: the exact value is zero).  No other rank test is
 *    made: on a gauge-free problem the pivots of S are rounding noise of either sign and the result is the caller's
 *    business, as with Ceres;
 *  - the covariance of the intrinsics blocks themselves and cross-covariances between blocks are not returned;
 *  - inverse-depth handles and sharded handles: THEIA_HIP_ERR_UNSUPPORTED; a workspace that does not fit (the factored
 *    copy of S, X [needed columns][n], the per-observation Jacobians): THEIA_HIP_ERR_OUT_OF_MEMORY.
 * The handle stays usable: the next run() starts from the same state. */
int theia_hip_ba_covariance_full(theia_ba_handle h, int32_t num_view_sel, const int32_t* view_sel, int32_t num_track_sel,
                                 const int32_t* track_sel, int32_t max_rhs_columns, double* cam_cov, double* point_cov);
/* Device time of the phases of the last theia_hip_ba_covariance_full call of this process, in milliseconds:
 * {linearisation + Jacobians + copy, factorisation, column solves, block kernels}. */
int theia_hip_ba_covariance_full_timing(double* phase_ms);
/* Tangent dimensions of the handle's variable blocks: 6 minus the frozen parameters per variable camera, the free
 * intrinsics of every variable group, d per variable point -- the "free parameters" of the variance factor
 * 2 * final_cost / (number of residuals - free parameters) of a coupled problem. */
int theia_hip_ba_free_parameter_count(theia_ba_handle h, int64_t* count);


/* Introspection used by parity tests (device results copied to host):
 *  - per-observation residual r[2] and Jacobian blocks J_cam[2][6],
 *    J_pt[2][pt_dof] (tangent space, loss-corrected, NOT Jacobi-scaled) of
 *    ReprojectionError<Model> (reprojection_error.h:54-110); valid[i] = functor
 *    return value.
 *  - the dense reduced camera system  S (n x n, row-major, both triangles) and
 *    rhs (n) for trust-region radius `radius`,
 *    n = 10 * (#variable intrinsics groups) + 6 * (#variable cameras) with the
 *    intrinsics slots first, in Jacobi-scaled space exactly as handed to the
 *    Cholesky kernel. */
int theia_hip_ba_evaluate(theia_ba_handle h, double* cost, double* residuals,
                          double* jac_cam, double* jac_pt, uint8_t* valid);
/* as theia_hip_ba_evaluate plus J_intr[2][THEIA_MAX_INTRINSICS] per observation
 * (zero for constant groups / frozen parameters). */
int theia_hip_ba_evaluate_ex(theia_ba_handle h, double* cost, double* residuals,
                             double* jac_cam, double* jac_pt, double* jac_intr,
                             uint8_t* valid);
int theia_hip_ba_reduced_system(theia_ba_handle h, double radius, int32_t* n,
                                double* S, double* rhs, int64_t capacity);

/* K3 alone (introspection for the parity tests): solve the dense SPD system
 * A x = b with the reduced-camera Cholesky kernels.  A: n x n row-major, only
 * the lower triangle is read; x: n.  Returns THEIA_HIP_ERR_INTERNAL when a
 * pivot is not positive (what makes an LM step "invalid"). */
int theia_hip_dense_spd_solve(int32_t n, const double* A, const double* b, double* x);

/* The same kernels factored once and solved many times (the ADMM solves of theia_hip_robust_rotation_averaging):
 * factor the n x n SPD matrix A (row-major, lower triangle read) once, then solve A X = B for the k right-hand sides
 * B [k][n] into X [k][n] against the stored factor.  THEIA_HIP_ERR_INTERNAL when a pivot is not positive. */
int theia_hip_dense_spd_solve_multi(int32_t n, const double* A, int32_t k, const double* B, double* X);

/* K3 on a tile structure the caller chooses (introspection for the K3 tests): the level-scheduled tile-sparse Cholesky
 * (chol_plan_create / chol_plan_solve) the BA runs, built for the given 64 x 64 tile co-visibility.
 * A: n x n SPD, row-major with leading dimension lda >= n.  Of the buffer only the factor's structure tiles (the declared
 * ones plus fill) at their physical lower position are read, and of a diagonal tile only its lower triangle: the strict
 * upper triangle is never read, so the assembly does not have to write it.
 * tile_adj [nt][nt] (nt = ceil(n / 64)), symmetric (the diagonal is ignored), or NULL = dense.
 * mode 0: A uploaded verbatim, the rhs as row n, the solution in place (the BA's layout when lda == n).
 * mode 1: as mode 0, but the solution goes to a separate buffer (the non-in-place back-substitution).
 * mode 2: a device buffer filled with NaN, chol_plan_clear, then A's lower structure tiles (tile_adj + the diagonal
 *         tiles) and the rhs ADDED on the device: the BA's clear-then-accumulate order.
 * info (optional): the path the plan took.  tile_order / tile_level [nt] (optional): the plan's elimination order
 * (the tile at each position) and the level of each position (identity / 0 .. nt-1 on the dense path).
 * THEIA_HIP_ERR_INTERNAL when a pivot is not positive; THEIA_HIP_ERR_INVALID_ARGUMENT for a bad n / lda / mode or an
 * asymmetric tile_adj (checked before the device is touched). */
typedef struct theia_k3_info {
  int32_t dense;             /* 1 = the plan fell back to the dense panel chain */
  int32_t levels, num_symm_tiles, num_deferred_targets, num_deferred_partials, split_level, num_shared_tiles;
  double flops;
} theia_k3_info;
int theia_hip_tile_sparse_spd_solve(int32_t n, int32_t lda, const uint8_t* tile_adj, int32_t mode, const double* A,
                                    const double* b, double* x, theia_k3_info* info, int32_t* tile_order,
                                    int32_t* tile_level);
/* The sharded plan (chol_plan_create_sharded) of num_ranks ranks, emulated in one process on one device.  Rank r holds
 * its partial system A [r] (n x n, lda = n) and b [r]; tile_class [r][nt]: 0 shared, 1 this rank's, 2 another rank's.
 * Per rank: the plan, phase 0 on its own partial sums; then the tiles of chol_plan_shared_tiles and the whole rhs row
 * summed over the ranks (in rank order, the same sum on every rank); then phase 1.  x [r]: rank r's raw solution (its
 * own private columns and the shared ones are meaningful).  THEIA_HIP_ERR_INVALID_ARGUMENT for tile classes that are
 * inconsistent across the ranks, THEIA_HIP_ERR_INTERNAL when the ranks' shared-tile lists differ or a pivot is not
 * positive, THEIA_HIP_ERR_UNSUPPORTED when a rank's structure has no level schedule. */
int theia_hip_tile_sparse_spd_solve_sharded(int32_t n, int32_t num_ranks, const uint8_t* tile_adj_union,
                                            const uint8_t* tile_class, const double* A, const double* b, double* x,
                                            theia_k3_info* info);

/* RobustRotationEstimator::EstimateRotations (global_pose_estimation/robust_rotation_estimator.cc:66-110; pybind
 * sfm.cc:1749-1780, the ROBUST_L1L2 global rotation estimator of the global pipeline): L1 ADMM regression on the view
 * graph (math/l1_solver.h), then IRLS with the weight sigma / (|e|^2 + sigma^2)^2 per edge, through one N x N Laplacian
 * factorisation per solve (csrc/rotation_averaging.hip).  orientations [num_views][3] angle-axis, in/out; fixed
 * [num_views] non-zero = held constant, or NULL (no view flagged: view 0 is fixed -- the reference fixes the first key
 * of its unordered_map); edges [num_edges][2] = (i, j) with relative_rotations [num_edges][3] = r_ij, R_j ~ R_ij R_i.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (the reference's CHECK failures; orientations untouched): no edge, an edge naming a
 * view out of range, a connected component of the view graph without a fixed view.  THEIA_HIP_ERR_INTERNAL: a
 * factorisation failed (the reference's `return false`); orientations hold the state reached so far.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (N + 3)^2 array of doubles (N = free views) does not fit on the device. */
typedef struct theia_rotation_options {
  int32_t max_num_l1_iterations, max_num_irls_iterations;
  double l1_step_convergence_threshold, irls_step_convergence_threshold, irls_loss_parameter_sigma;
} theia_rotation_options;
typedef struct theia_rotation_summary {
  int32_t l1_iterations, admm_iterations, irls_iterations, reserved;
  double final_squared_residual, setup_ms, l1_ms, irls_ms;
} theia_rotation_summary;
int theia_hip_robust_rotation_averaging(int32_t num_views, double* orientations, const uint8_t* fixed, int32_t num_edges,
                                        const int32_t* edges, const double* relative_rotations,
                                        const theia_rotation_options* options, theia_rotation_summary* summary);

/* LinearRotationEstimator::EstimateRotations (global_pose_estimation/linear_rotation_estimator.cc:76-204, Martinec &
 * Pajdla; the LINEAR global rotation estimator of the global pipeline, global_reconstruction_estimator.cc:349-353):
 * orientations from the pairs' relative rotations alone, without an initial guess (csrc/linear_rotations.hip).  Per pair
 * e = (i, j) with R_e = AngleAxisToRotationMatrix(relative_rotations[e]), R_j = R_e R_i, the symmetric 3n x 3n matrix M
 * over the n views that have an edge gets +I on the diagonal blocks (i, i) and (j, j), -R_e' at block (i, j) and -R_e at
 * block (j, i) (:90-150); repeated pairs add up.  The eigenvectors of its three smallest eigenvalues, X [3n][3], hold
 * X_i = R_i Q / sqrt(n) for one common orthogonal Q, and view i's orientation is ProjectToRotationMatrix(X_i)
 * (sfm/pose/util.cc:117-129: U V' of the Jacobi SVD, negated when its determinant is negative) as angle-axis (:170-201).
 * Where the reference runs Spectra's shift-invert Lanczos (3 of 6 vectors, shift 0, 1000 iterations, 1e-4) over a sparse
 * Cholesky of M, this runs a block inverse iteration over one dense Cholesky of M + mu I, mu = 3n eps max diag M (the three
 * eigenvalues are rounding errors of either sign on noise-free input; the shift moves no eigenvector): from a fixed
 * pseudo-random start block, Y = (M + mu I)^-1 X, Q = Y orthonormalised (modified Gram-Schmidt, two passes), until
 * |Q - X (X' Q)|_F <= subspace_convergence_threshold.  The result is defined up to Q: the reference fixes no view and
 * neither does this; Q differs from the reference's and is the same in every run (no floating-point atomics, every sum
 * in a fixed order: two runs are bit-identical).
 * edges [num_edges][2] = (i, j); orientations_out [num_views][3] angle-axis and estimated_out [num_views]: a view with an
 * edge gets its orientation and 1; a view without one gets 0 and its orientations_out row is left untouched (the
 * reference gives it no entry).
 * THEIA_HIP_ERR_INVALID_ARGUMENT (checked before the device is touched; outputs untouched, summary zeroed): no edge (the
 * reference's CHECK_GT, :158); an edge naming a view out of range; an edge from a view to itself (the reference would
 * write -R into a diagonal block); the views that have edges do not form one connected graph (the reference does not
 * check: the null space then has three dimensions per component and its result is meaningless);
 * max_num_iterations <= 0; a threshold that is not positive and finite.
 * THEIA_HIP_ERR_INTERNAL: a pivot of the factorisation was not positive (outputs untouched, summary holds the shift), or
 * the iteration did not converge within max_num_iterations (outputs hold the state reached).
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3n + 1)^2 array of doubles does not fit on the device. */
typedef struct theia_linear_rotation_options {
  int32_t max_num_iterations;      /* 1000, the reference's Spectra limit */
  int32_t reserved;
  double subspace_convergence_threshold;   /* 1e-10 */
} theia_linear_rotation_options;
typedef struct theia_linear_rotation_summary {
  int32_t iterations, num_views_in_system;
  double eigenvalues[3];           /* ascending, shift subtracted: 1 / theta - mu for the eigenvalues theta of X' Y */
  double subspace_change;          /* |Q - X (X' Q)|_F of the last step */
  double shift;                    /* mu */
  double setup_ms, factor_ms, iterate_ms;   /* set-up = checks, plan, uploads, assembly, start block */
} theia_linear_rotation_summary;
int theia_hip_linear_rotations(int32_t num_views, int32_t num_edges, const int32_t* edges,
                               const double* relative_rotations, const theia_linear_rotation_options* options /*NULL = defaults*/,
                               double* orientations_out, uint8_t* estimated_out, theia_linear_rotation_summary* summary);

/* LagrangeDualRotationEstimator::EstimateRotations (global_pose_estimation/lagrange_dual_rotation_estimator.cc:51-197;
 * pybind sfm.cc:1797-1801; the LAGRANGE_DUAL global rotation estimator of the global pipeline,
 * global_reconstruction_estimator.cc:354-360, and the first half of HYBRID, hybrid_rotation_estimator.cc:69-109): global
 * orientations from the pairs' relative rotations alone, without an initial guess, by the rank-restricted SDP relaxation
 * of rotation averaging with its certificate of global optimality (csrc/lagrange_dual_rotations.hip).
 * Per pair e = (i, j) with R_e = AngleAxisToRotationMatrix(relative_rotations[e]), R_j ~ R_e R_i, the symmetric 3n x 3n
 * matrix R over the n views that have an edge, indexed in ascending view order, has R_e' at block (i, j) and R_e at block
 * (j, i) (:167-197); Q = -R.  The unknown is Y [r][3n], r = min_rank at first, all zero unless y_init is given.
 *   BCM (math/rank_restricted_sdp_solver.cc:58-129): per sweep, for every view in the sweep order, G_i = sum over its
 *     neighbours j of Y_j Q_ji and Y_i = U V' of the thin SVD of -G_i ([I_3; 0] for a zero block, as Eigen's JacobiSVD
 *     gives).  f = tr(Y Q Y').  Before each sweep err = |f_prev - f| / max(|f_prev|, 1) with f_prev = DBL_MAX at first
 *     (math/bcm_sdp_solver.h:64-72); the BCM stops when err <= tolerance or after max_iterations sweeps;
 *     total_iterations_num = sweeps + 1 (:127).
 *   Staircase (math/riemannian_staircase.cc:57-111), for r = min_rank .. max_rank: the BCM; Lambda = SymBlockDiag(Q Y' Y);
 *     lambda_min(Q - Lambda) > -min_eigenvalue_nonnegativity_tolerance: certified, stop.  Otherwise a zero row is added to
 *     Y, Ydot = that row set to v', v a unit direction of negative curvature, and alpha is backtracked from
 *     max(16e-6, 10 gradient_tolerance / |lambda_min|) by halving down to 1e-6 (:215-309): the first trial
 *     Y+ = per-view polar factor of Y + alpha Ydot with f(Y+) < f(Y), Riemannian gradient norm > gradient_tolerance and
 *     > preconditioned_gradient_tolerance (no preconditioner) is taken, else the trial of least f when that is below
 *     f(Y), else the staircase stops (the added zero row stays, as in the reference).  After an uncertified level at
 *     max_rank the escape still runs, so final_rank is at most max_rank + 1.
 *   Solution (:311-319, :148-165): X_i = Y_0' Y_i, projected by ProjectToSOd (math/rotation.cc:105-120) when the rank left
 *     behind is above min_rank; view i's orientation is X_i', negated when its determinant is negative, as angle-axis.
 *     The gauge view, whose orientation is the identity, is the lowest view that has an edge (the reference: its view of
 *     index 0, which may have no edge).
 * Stated deviations.  (1) G_i is gathered from the neighbours at every update, where the reference keeps G incrementally:
 * the same sums in another order.  (2) The sweep is scheduled in levels of views that share no edge; sweep_order INDEX is
 * the reference's order, COLOURED the order by (greedy colour in index order, index), which is the reference's sweep on a
 * relabelled graph (its SetViewIdToIndex allows it) and needs as many launches per sweep as there are colours.  (3) The
 * certificate is a dense FP64 Cholesky of Q - Lambda + sigma I: no failed pivot at sigma = the tolerance is the
 * reference's test.  (4) Where the reference's Lanczos starts from a random vector, v comes from a shift bracketed to 5 %
 * between a failing and a succeeding factorisation and inverse iteration from a fixed start; it is admitted only when
 * v'(Q - Lambda)v <= 0.9 lambda_min is proven by the bracket.  The staircase's path after an escape depends on v within
 * the arithmetic of the BCM's tolerance.  No atomics: two runs on one input are bit-identical.
 * The polar factor is defined where sigma_min(G_i) >= 1e-3 sigma_max(G_i) (|Y_i' Y_i - I| <= 1e-14); a non-zero block with
 * a zero singular value makes f non-finite and the call returns THEIA_HIP_ERR_INTERNAL.
 * solver_type THEIA_SDP_RANK_DEFICIENT_BCM runs one BCM at rank 3 (or rank_init) with no certificate, as the reference
 * uses RankRestrictedSDPSolver; ComputeErrorBound (:86-145) is not part of EstimateRotations and is not built.
 * edges [num_edges][2] = (i, j); y_init: NULL, or [rank_init][3n] with rank_init in 3 .. 10 (inside min_rank .. max_rank
 * for the staircase) whose blocks have orthonormal columns; orientations_out [num_views][3] and estimated_out
 * [num_views] as theia_hip_linear_rotations: a view without an edge gets 0 and its row is left untouched; y_out: NULL, or
 * room for [max_rank + 1][3n], of which [final_rank][3n] is written; level_log_out: NULL, or [level_log_rows][8], one row
 * per BCM: rank, sweeps, f after the level, certified, the lambda_min estimate (NaN where certified, which needs none),
 * v'(Q - Lambda)v of the escape direction, the accepted alpha (0: none), 1 when the least-f fallback was used;
 * summary->num_levels counts the rows there would be.
 * Returns 0 whatever the staircase's end, as the reference returns true; summary->end_state says which it was.
 * THEIA_HIP_ERR_UNSUPPORTED: solver_type THEIA_SDP_RBR_BCM (no caller's default; its dense 3n x 3n iterate is another
 * design).  THEIA_HIP_ERR_INVALID_ARGUMENT (checked before the device is touched; outputs untouched, summary zeroed): no
 * edge (the reference's CHECK_GT, :91); a view out of range; a pair naming one view twice; an unordered pair given twice
 * (the reference's map cannot hold one, and its adjacency list would count it inconsistently); the views that have edges
 * do not form one connected graph; min_rank or max_rank outside 3 .. 10 or min_rank > max_rank; rank_init out of range; a
 * tolerance that is negative or not finite; max_iterations <= 0; an unknown solver_type or sweep_order.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3n + 1)^2 array of doubles of the certificate does not fit on the device (only
 * the staircase allocates it).  THEIA_HIP_ERR_INTERNAL: f not finite; no admissible v (outputs untouched). */
enum { THEIA_SDP_RBR_BCM = 0, THEIA_SDP_RANK_DEFICIENT_BCM = 1, THEIA_SDP_RIEMANNIAN_STAIRCASE = 2 };   /* math/solver_options.h:43-49 */
enum { THEIA_SWEEP_ORDER_INDEX = 0, THEIA_SWEEP_ORDER_COLOURED = 1 };
enum {
  THEIA_LAGRANGE_DUAL_END_BCM = 0,            /* RANK_DEFICIENT_BCM: no certificate asked for */
  THEIA_LAGRANGE_DUAL_END_CERTIFIED = 1,
  THEIA_LAGRANGE_DUAL_END_MAX_RANK = 2,       /* the level at max_rank was not certified */
  THEIA_LAGRANGE_DUAL_END_ESCAPE_FAILED = 3   /* no trial step lowered f */
};
typedef struct theia_lagrange_dual_options {
  int32_t solver_type;             /* THEIA_SDP_RIEMANNIAN_STAIRCASE */
  int32_t max_iterations;          /* 500 sweeps per BCM */
  int32_t min_rank, max_rank;      /* 3, 10 */
  int32_t sweep_order;             /* THEIA_SWEEP_ORDER_INDEX */
  int32_t reserved;
  double tolerance;                /* 1e-8 */
  double min_eigenvalue_nonnegativity_tolerance;   /* 1e-5 */
  double gradient_tolerance, preconditioned_gradient_tolerance;   /* 1e-2, 1e-4 */
} theia_lagrange_dual_options;
typedef struct theia_lagrange_dual_summary {
  int32_t total_iterations_num;    /* of the last BCM, as the reference's Summary: sweeps + 1 */
  int32_t sweeps, total_sweeps;    /* of the last BCM; of all of them */
  int32_t final_rank, end_state, num_levels, num_views_in_system, gauge_view;
  int32_t schedule_levels, schedule_launches;   /* levels of the sweep order; launches per sweep */
  int32_t factorisations, reserved;
  double f;                        /* tr(Y Q Y') of the Y left behind */
  double lambda_min;               /* the estimate of the last uncertified level; NaN when the last level was certified */
  double setup_ms, sweep_ms, certificate_ms, escape_ms, total_ms;
} theia_lagrange_dual_summary;
int theia_hip_lagrange_dual_rotations(int32_t num_views, int32_t num_edges, const int32_t* edges,
                                      const double* relative_rotations, const theia_lagrange_dual_options* options /*NULL = defaults*/,
                                      int32_t rank_init, const double* y_init /* optional */, double* orientations_out,
                                      uint8_t* estimated_out, double* y_out /* optional */, theia_lagrange_dual_summary* summary,
                                      double* level_log_out /* optional */, int32_t level_log_rows);

/* NonlinearRotationEstimator::EstimateRotations (global_pose_estimation/nonlinear_rotation_estimator.cc:49-98 with
 * pairwise_rotation_error.h:65-96; pybind sfm.cc:1782-1787; the NONLINEAR global rotation estimator of the global
 * pipeline): Ceres' Levenberg-Marquardt solve over one PairwiseRotationError block per pair, weight 1, under
 * SoftLOneLoss(robust_loss_width), restated on the device in FP64 (csrc/nonlinear_rotations.hip).  Per
 * pair e = (i, j) the residual is the angle-axis vector of R(w_j) R(w_i)' R(rel_e)' (ceres::AngleAxisToRotationMatrix,
 * ceres::RotationMatrixToAngleAxis, small-angle branches included); the Jacobians are closed forms of the branch taken.
 * The solver is ceres::Solver::Options at its defaults with max_num_iterations = 200 (:90-92): TrustRegionMinimizer +
 * LevenbergMarquardtStrategy of Ceres 2.2 on the dense normal equations of order 3m, m = the views that take part.
 * orientations [num_views][3] angle-axis, in/out; fixed [num_views] non-zero = held constant (no columns, not in |x|,
 * bits unchanged), or NULL: no view is held, the reference's problem -- the gauge (a common rotation on the right) is
 * then free, only the LM diagonal makes the system definite, and a factorisation that meets a pivot that is not positive
 * is an invalid step, not an error.  A view without an edge is not in the problem and is left untouched; a pair between
 * two held views is not in the problem either.  edges [num_edges][2] = (i, j) with relative_rotations [num_edges][3] =
 * TwoViewInfo::rotation_2, R_j ~ R_ij R_i; repeated and reversed pairs add up.
 * trace_out (optional) [trace_capacity][5]: (cost, gradient max norm, step norm, radius, accepted) per row, row 0 the
 * start, then one row per iteration, in theia_ba_summary's convention; summary->trace_size rows are written.
 * Returns 0 whatever the termination, as the reference returns true: after THEIA_ROTATION_TERM_FAILURE (five invalid
 * steps in a row) the orientations are as passed in, after the cap they hold the last accepted iterate.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (checked before the device is touched; orientations untouched, summary zeroed): no edge;
 * an edge naming a view out of range; an edge from a view to itself (Ceres refuses a residual block that names one
 * parameter block twice); max_num_iterations < 0; a width or a maximum radius that is not positive and finite; a
 * tolerance that is negative or not finite (zero switches a rule off, as in Ceres).
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3m + 1)^2 array of doubles does not fit on the device. */
enum {
  THEIA_ROTATION_TERM_NONE = 0,                 /* nothing to solve: every view of every edge is held */
  THEIA_ROTATION_TERM_GRADIENT_TOLERANCE = 1,
  THEIA_ROTATION_TERM_FUNCTION_TOLERANCE = 2,
  THEIA_ROTATION_TERM_PARAMETER_TOLERANCE = 3,
  THEIA_ROTATION_TERM_MAX_ITERATIONS = 4,
  THEIA_ROTATION_TERM_FAILURE = 5,
  THEIA_ROTATION_TERM_MIN_RADIUS = 6            /* the radius fell to 1e-32 */
};
typedef struct theia_nonlinear_rotation_options {
  int32_t max_num_iterations;      /* 200 */
  int32_t reserved;
  double robust_loss_width;        /* 0.1 */
  double function_tolerance;       /* 1e-6 */
  double gradient_tolerance;       /* 1e-10 */
  double parameter_tolerance;      /* 1e-8 */
  double max_trust_region_radius;  /* 1e16, Ceres' default (the BA's options carry 1e12) */
} theia_nonlinear_rotation_options;
typedef struct theia_nonlinear_rotation_summary {
  int32_t iterations;              /* passes of the loop; a pass that ends on the parameter or function tolerance is in none of the three counts below */
  int32_t num_successful_steps, num_unsuccessful_steps, num_invalid_steps;
  int32_t termination;             /* THEIA_ROTATION_TERM_* */
  int32_t num_views_in_problem;    /* m */
  int32_t trace_size, reserved;
  double initial_cost, final_cost, final_radius, final_gradient_max_norm, seconds;
} theia_nonlinear_rotation_summary;
int theia_hip_nonlinear_rotations(int32_t num_views, double* orientations /* [n][3], in/out */,
                                  const uint8_t* fixed /* [n] or NULL */, int32_t num_edges, const int32_t* edges,
                                  const double* relative_rotations,
                                  const theia_nonlinear_rotation_options* options /*NULL = defaults*/,
                                  theia_nonlinear_rotation_summary* summary, double* trace_out /* optional */,
                                  int32_t trace_capacity);

/* NonlinearPositionEstimator::EstimatePositions (global_pose_estimation/nonlinear_position_estimator.cc:136-206 with
 * pairwise_translation_error.h:65-100; the NONLINEAR global position estimator, the default of
 * ReconstructionEstimatorOptions, global_reconstruction_estimator.cc:431): Ceres' Levenberg-Marquardt solve over one
 * PairwiseTranslationError block per pair and one per observation of a selected track, under
 * HuberLoss(robust_loss_width), restated on the device in FP64 (csrc/nonlinear_positions.hip).  The
 * unknowns are 3-vectors: the positions [num_views][3] and the points [num_points][3], both in/out.
 *   camera-to-camera (:226-259): edges [num_edges][2] = (i, j) with relative_translations [num_edges][3] =
 *     TwoViewInfo::position_2; direction t = R(orientations[i])' position_2 (ceres::AngleAxisToRotationMatrix), weight 1,
 *     scale = scale_estimates[e] (TwoViewInfo::scale_estimate), NULL = all -1; repeated and reversed pairs add up
 *   point-to-camera (:382-412): track t = observations track_offsets[t] .. track_offsets[t + 1] - 1 of obs_view [N] /
 *     obs_feature [N][2] (normalised), one edge each from the view to the point; direction
 *     normalize(R(w_ray)' [x, y, 1]) with w_ray = ray_orientations[view], NULL = orientations (the reference rotates the
 *     ray by the camera's own stored orientation, :68-75); weight point_to_camera_weight, scale -1
 *   residual with d = x_second - x_first: scale > 0: w (d - scale t); otherwise w (d / |d| - t), and with |d| < 1e-12 the
 *     norm is the constant 1.  The Jacobians are closed forms of the branch taken.
 * The solver is that of theia_hip_nonlinear_rotations: TrustRegionMinimizer + LevenbergMarquardtStrategy of Ceres 2.2 on
 * the dense normal equations of order 3 (free views + points); the points are not Schur-eliminated (DESIGN.md 3.6l on
 * the reference's choice of linear solver).  fixed [num_views] non-zero = held constant (no columns, not in |x|, bits
 * unchanged), or NULL; a view without an edge is left untouched; a pair between two held views is not in the problem;
 * points are never held.  The gauge (a translation, and a scale too where no edge carries a scale estimate) is free
 * unless views are held: only the LM diagonal makes the system definite then.
 * trace_out and the return value as theia_hip_nonlinear_rotations; summary->termination takes the THEIA_ROTATION_TERM_*
 * values above, which name the rules of the loop the two stages share.  After THEIA_ROTATION_TERM_FAILURE positions and
 * points are as passed in, otherwise they hold the last accepted iterate; with nothing free the call returns 0 with
 * THEIA_ROTATION_TERM_NONE.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (checked before the device is touched; arrays untouched, summary zeroed): no views; no
 * edges of either kind; an index out of range; an edge from a view to itself; a non-finite input; a width, a weight or a
 * maximum radius that is not positive and finite; a tolerance that is negative or not finite; max_num_iterations < 0;
 * num_points > 0 with a null array; track_offsets that do not start at 0 and increase strictly; an observation naming a
 * view twice in one track.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3m + 1)^2 array of doubles does not fit on the device. */
typedef struct theia_nonlinear_position_options {
  int32_t max_num_iterations;      /* 400 */
  int32_t reserved;
  double robust_loss_width;        /* 0.1 */
  double function_tolerance;       /* 1e-6 */
  double gradient_tolerance;       /* 1e-10 */
  double parameter_tolerance;      /* 1e-8 */
  double max_trust_region_radius;  /* 1e16 */
} theia_nonlinear_position_options;
typedef struct theia_nonlinear_position_summary {
  int32_t iterations;              /* as theia_nonlinear_rotation_summary */
  int32_t num_successful_steps, num_unsuccessful_steps, num_invalid_steps;
  int32_t termination;             /* THEIA_ROTATION_TERM_* */
  int32_t num_views_in_problem;    /* the views that take columns */
  int32_t trace_size;
  int32_t num_points_in_problem;
  int32_t num_camera_edges_in_problem;   /* pairs with a free end */
  int32_t num_point_edges_in_problem;
  double initial_cost, final_cost, final_radius, final_gradient_max_norm, seconds;
} theia_nonlinear_position_summary;
int theia_hip_nonlinear_positions(int32_t num_views, const double* orientations /* [n][3] */,
                                  double* positions /* [n][3], in/out */, const uint8_t* fixed /* [n] or NULL */,
                                  int32_t num_edges, const int32_t* edges, const double* relative_translations,
                                  const double* scale_estimates /* [E] or NULL */, int32_t num_points,
                                  double* points /* [T][3], in/out, or NULL */, const int32_t* track_offsets /* [T + 1] */,
                                  const int32_t* obs_view, const double* obs_feature,
                                  const double* ray_orientations /* [n][3] or NULL */, double point_to_camera_weight,
                                  const theia_nonlinear_position_options* options /*NULL = defaults*/,
                                  theia_nonlinear_position_summary* summary, double* trace_out /* optional */,
                                  int32_t trace_capacity);

/* LeastUnsquaredDeviationPositionEstimator::EstimatePositions (global_pose_estimation/
 * least_unsquared_deviation_position_estimator.cc:75-213; pybind sfm.cc:1196-1204, 1707-1726, the default
 * LEAST_UNSQUARED_DEVIATION position stage of the global pipeline): per pair e = (i, j) the rows c_j - c_i - s_e d_e with
 * d_e = R_i' relative_translation_e and the bound s_e >= 1, solved by ConstrainedL1Solver's ADMM
 * (math/constrained_l1_solver.cc:49-187) with the scales eliminated: one dense 3m x 3m Cholesky of the Schur complement
 * (m = free views), factored once, then up to max_num_iterations x-updates against it; the stopping test runs on the
 * device (csrc/lud_positions.hip).  orientations [num_views][3] angle-axis (world -> camera); fixed [num_views] non-zero =
 * held at the origin, or NULL (view 0 is held -- the reference holds the first view its unordered_set yields); edges
 * [num_edges][2] = (i, j) with relative_translations [num_edges][3] = TwoViewInfo::position_2; positions_out [num_views][3].
 * THEIA_HIP_ERR_INVALID_ARGUMENT (the reference's CHECK failures; nothing launched, outputs untouched): no edge, an edge
 * naming a view out of range, a connected component of the view graph without a held view (a view without edges counts),
 * max_num_iterations <= 0, rho <= 0 or a non-finite option.  THEIA_HIP_ERR_INTERNAL: the factorisation failed (positions
 * untouched).  THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3m + 1)^2 array of doubles does not fit on the device
 * (5 000 free views take 1.8 GB, 20 000 take 29 GB). */
typedef struct theia_lud_options {   /* ConstrainedL1Solver::Options (constrained_l1_solver.h:64-74) */
  int32_t max_num_iterations, reserved;                 /* 1000 */
  double rho, alpha, absolute_tolerance, relative_tolerance;   /* 10, 1.2, 1e-4, 1e-2 */
} theia_lud_options;
typedef struct theia_lud_summary {
  int32_t admm_iterations, converged;   /* converged: the stopping test passed within max_num_iterations */
  double r_norm, s_norm, primal_eps, dual_eps;   /* of the last iteration */
  double setup_ms, factor_ms, admm_ms;
} theia_lud_summary;
int theia_hip_lud_positions(int32_t num_views, const double* orientations, const uint8_t* fixed, int32_t num_edges,
                            const int32_t* edges, const double* relative_translations, const theia_lud_options* options,
                            double* positions_out, theia_lud_summary* summary);

/* LiGTPositionEstimator::EstimatePositions (global_pose_estimation/LiGT_position_estimator.cc:160-470, options
 * LiGT_position_estimator.h:70-82; pybind sfm.cc:1728-1747, the LIGT position stage of the global pipeline, which skips the pairwise
 * translation optimisation and the 1DSfM filter for it, global_reconstruction_estimator.cc:190-208): positions from the
 * global orientations and the tracks' normalised features (csrc/ligt_positions.hip).  Per track of >= 3 observations the
 * base pair maximises theta^2_ij = |[f_j]x R_j R_i' f_i|^2 (:227-255), every other observation gives one 3-row constraint
 * B c_v1 + C c_v2 + D c_v3 = 0 (:257-289, :307-351), the normal equations H = sum [B C D]' [B C D] are summed on the 3 x 3
 * blocks of the views (:94-121, :356-401) without the held view, and the positions are the unit eigenvector of H's
 * smallest eigenvalue: one dense Cholesky of H + mu I, mu = n eps max diag H (the shift moves no eigenvector), then inverse
 * iteration from x = 1 / sqrt(n) until |x_new - sign(x_new . x) x|_2 <= eigensolver_threshold or max_power_iterations
 * (the reference declares both options and reads neither: it takes BDCSVD or Spectra's shift-invert, :190-207).  The sign
 * is voted by the view pairs (:432-470): +1 when (R_first (c_second - c_first) / |.|) . relative_translation > 0, else -1,
 * over the pairs whose two views are in the system; a negative total flips every position.  num_edges = 0: no vote.
 * orientations [num_views][3] angle-axis (world -> camera); track t holds the observations track_offsets[t] ..
 * track_offsets[t + 1] - 1 of obs_view / obs_feature ((x, y) of hnormalized(PixelToNormalizedCoordinates(pixel))).
 * Where the reference depends on the order of its hash maps or threads, the rule here is: tracks in the caller's order
 * and observations in the caller's order within a track; the base pair is the first maximal pair in lexicographic (i, j)
 * order (strict >, from 0); a track with fewer than 3 observations, or whose best theta^2 is not positive (0 or NaN; the
 * reference reads a default-constructed pair there), is skipped and enters no view into the system; the held view (index
 * -1, at the origin) is v1 of the first track used; the other views are indexed in the order of the reference's
 * insertions, v1, v2, v3 per constraint, constraints in (track, observation) order; every entry of H is summed in (track,
 * observation) order by one owner, B'B, B'D and D'D within their track first, without floating-point atomics: two runs are
 * bit-identical.  theta^2 of the pair search is evaluated as |R_i' f_i x R_j' f_j|^2, equal for orthonormal R; the
 * observation of v3 itself, whose B = C = D vanish, is counted as a constraint and adds nothing.
 * positions_out [num_views][3] and estimated_out [num_views]: a view of the system gets its position (the held view
 * zeros) and 1; a view outside it gets 0 and its positions_out row is left untouched.  Optional outputs: base_pairs_out
 * [num_tracks][2] observation indices within the track (-1 -1: skipped); system_out [3 (m - 1)]^2 row-major, H before
 * the shift, both triangles (m = summary->num_views_in_system; size it for num_views); system_index_out [num_views]: the
 * view's block in H, -1 held, -2 not in the system.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing launched, outputs untouched; checked before the device is touched): a view index
 * out of range, decreasing track_offsets, a track naming one view twice, a view pair out of range,
 * max_power_iterations <= 0, a non-positive or non-finite eigensolver_threshold, no track with 3 observations; the same
 * code, outputs untouched, after the pair search when every track was skipped for its theta^2.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (3 (m - 1) + 1)^2 array of doubles (twice with system_out), or the 72 bytes per
 * 3 x 3 item (three per used track and three per constraint), do not fit on the device.  THEIA_HIP_ERR_INTERNAL: the
 * factorisation failed even with the shift (outputs untouched, summary holds the shift). */
typedef struct theia_ligt_options {   /* LiGTPositionEstimator::Options (LiGT_position_estimator.h:70-82) */
  int32_t max_power_iterations, reserved;   /* 1000 */
  double eigensolver_threshold;             /* 1e-8 */
} theia_ligt_options;
typedef struct theia_ligt_summary {
  int32_t num_views_in_system;   /* m: the held view and the 3 (m - 1) unknowns' views */
  int32_t tracks_used, tracks_skipped;
  int32_t num_constraints;       /* len - 1 per used track, as the reference counts its triplets */
  int32_t iterations, converged; /* converged: the step test passed within max_power_iterations */
  int32_t sign_votes, flipped;   /* the total of the +1 / -1 votes; 1 = every position was negated */
  double eigenvalue;             /* the last iterate's Rayleigh quotient minus the shift */
  double shift;                  /* mu */
  double setup_ms, assemble_ms, factor_ms, eig_ms;   /* set-up = checks, uploads, pair search, plan */
} theia_ligt_summary;
int theia_hip_ligt_positions(
    int32_t num_views, const double* orientations /*[num_views][3] angle-axis, world -> camera*/,
    int32_t num_tracks, const int32_t* track_offsets /*[num_tracks+1]*/,
    const int32_t* obs_view /*[num_obs]*/, const double* obs_feature /*[num_obs][2], normalised*/,
    int32_t num_edges, const int32_t* edges /*[num_edges][2]*/,
    const double* relative_translations /*[num_edges][3]; 0 edges = no sign vote*/,
    const theia_ligt_options* options /*NULL = defaults*/,
    double* positions_out /*[num_views][3]*/, uint8_t* estimated_out /*[num_views]*/,
    int32_t* base_pairs_out /*optional [num_tracks][2]*/,
    double* system_out /*optional*/, int32_t* system_index_out /*optional [num_views]*/,
    theia_ligt_summary* summary);

/* LinearPositionEstimator::EstimatePositions (global_pose_estimation/linear_position_estimator.cc:151-473, options
 * linear_position_estimator.h; compute_triplet_baseline_ratios.cc:52-157; math/graph/triplet_extractor.h;
 * triangulation.cc:130-157, 236-250; the LINEAR_TRIPLET position stage of the global pipeline; Jiang, Cui, Tan, ICCV 2013):
 * positions from the global orientations, the view pairs' relative poses and the tracks' normalised features
 * (csrc/linear_positions.hip).
 *  1. Every triangle (a < b < c) of the view pairs (triplet_extractor.h FindTriplets).
 *  2. Per triangle and per track seen by all three views the unit rays f = (x, y, 1) / |.|; each of the pairs (a, b),
 *     (a, c), (b, c) is triangulated in its first view's frame from the origins 0 and position_2 and the directions f_first
 *     and R_2' f_second (compute_triplet_baseline_ratios.cc:52-88): the rays must satisfy d0 . d1 < cos(2 deg)
 *     (triangulation.cc:236-250), TriangulateMidpoint solves sum (I - d d') p = sum (I - d d') o by LLT (:130-157), the depths
 *     are |p| and |p - position_2|.  baseline = (1, median(depth1_12 / depth1_13), median(depth2_12 / depth2_23)) (:92-157).
 *  3. Per view the number of triangles it is in; the views indexed in the order a, b, c over the triangles, the first held at
 *     the origin (index -1) (linear_position_estimator.cc:222-243); w = 1 / sqrt(min of the three counts) (:374-380).
 *  4. Per triangle t01 = -R_a' p2(a, b), t02 = -R_a' p2(a, c), t12 = -R_b' p2(b, c), r012 = FromTwoVectors(t12, -t01),
 *     r201 = FromTwoVectors(t01, t02), r120 = FromTwoVectors(-t02, -t12) (:335-364), s012 = b0 / b2, s201 = b1 / b0,
 *     s120 = b2 / b1, the three constraint rows of :396-422, and H += Ci' Cj on the views' 3 x 3 blocks without the held
 *     view's rows and columns (:87-134).
 *  5. The positions are the unit eigenvector of H's smallest eigenvalue (the reference: Spectra shift-invert, :189-196).
 *     Here: one dense Cholesky of H + mu I, mu = n eps max diag H (the shift moves no eigenvector; on noise-free data the
 *     eigenvalue is a rounding error of either sign), then inverse iteration from x = 1 / sqrt(n) until
 *     |x_new - sign(x_new . x) x|_2 <= eigensolver_threshold or max_power_iterations.
 *  6. The sign is voted by the view pairs (:435-473): +1 when (R_first (c_second - c_first) / |.|) . position_2 > 0, else
 *     -1, over the pairs whose two views are in the system; a negative total flips every position.
 * orientations [num_views][3] angle-axis (world -> camera); edges [num_edges][2] with first < second, each pair at most
 * once; relative_rotations / relative_translations [num_edges][3] = TwoViewInfo::rotation_2 / position_2; the tracks as
 * theia_hip_ligt_positions takes them.
 * Where the reference depends on the order of its hash containers or threads, or is undefined, the rule here is:
 *  - Order: the triangles are in lexicographic (a, b, c) order, and "in order" below means this order.
 *  - A track is skipped for a triangle when any of its three pairs fails the angle test, a midpoint solve meets a
 *    non-positive pivot, or either ratio is not finite and positive.
 *  - The median of k valid ratios is the element of rank k / 2 (integer division, 0-based, ascending: nth_element at
 *    size / 2); the two medians are independent.
 *  - A triangle with k = 0 is dropped before the components are formed (the reference divides by its zero baseline);
 *    components, counts, view indexing and weights are taken over the surviving triangles only.
 *  - Two triangles are connected when they share an edge; the largest component is used, ties go to the one holding the
 *    lexicographically first triangle (the reference sorts by size only).
 *  - The held view is a of the first used triangle.
 *  - FromTwoVectors is Eigen's arithmetic: both normalised, c = v0 . v1, axis v0 x v1, s = sqrt(2 (1 + c)), the quaternion
 *    (s / 2, axis / s) and its matrix.  Where c < -1 + 1e-12 Eigen takes an SVD; here the result is the rotation by pi,
 *    2 u u' - I, about u = normalize(v0 x e_k), k the first component of v0 of the smallest magnitude (three cameras on a
 *    line give t12 parallel to t01).
 *  - Every entry of H is summed in triangle order by one owner, within a triangle the three constraint rows in the
 *    reference's order.  No floating-point atomics anywhere: two runs are bit-identical.
 * positions_out [num_views][3] and estimated_out [num_views]: a view of the system gets its position (the held view zeros)
 * and 1; a view outside it gets 0 and its positions_out row is left untouched.  Optional outputs: triplets_out
 * [triplet_capacity][3], triplet_state_out [triplet_capacity] (0 used, 1 no ratios, 2 other component), baselines_out
 * [triplet_capacity][3] (zeros for state 1): the first triplet_capacity triangles, summary->num_triplets is the total;
 * system_out [3 (m - 1)]^2 row-major, H before the shift, both triangles (m = summary->num_views_in_system; size it for
 * num_views); system_index_out [num_views]: the view's block in H, -1 held, -2 not in the system.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing written; checked before the device is touched): a view index out of range, an
 * edge with first >= second, a duplicate edge, decreasing track_offsets, a track naming a view twice,
 * max_power_iterations <= 0, a non-positive or non-finite eigensolver_threshold, fewer than 3 edges; the same code,
 * outputs untouched, after the stage that finds it when the graph has no triangle or no triangle has ratios.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the triangle list (24 bytes per triangle, at most INT32_MAX / 3 triangles), the ratio
 * scratch (one triangle with more than 2^24 possible common tracks) or the dense (3 (m - 1) + 1)^2 array of doubles
 * (twice with system_out) do not fit.  THEIA_HIP_ERR_INTERNAL: the factorisation failed even with the shift (outputs
 * untouched, summary holds the shift). */
typedef struct theia_linear_triplet_options {   /* LinearPositionEstimator::Options (linear_position_estimator.h) */
  int32_t max_power_iterations, reserved;   /* 1000; the reference declares both and reads neither */
  double eigensolver_threshold;             /* 1e-8 */
} theia_linear_triplet_options;
typedef struct theia_linear_triplet_summary {
  int32_t num_triplets;                  /* triangles found */
  int32_t triplets_without_ratios;       /* state 1 */
  int32_t triplets_in_other_components;  /* state 2 */
  int32_t triplets_used;                 /* state 0 */
  int32_t num_views_in_system;   /* m: the held view and the 3 (m - 1) unknowns' views */
  int32_t iterations, converged; /* converged: the step test passed within max_power_iterations */
  int32_t sign_votes, flipped;   /* the total of the +1 / -1 votes; 1 = every position was negated */
  int32_t reserved;
  double eigenvalue;             /* the last iterate's Rayleigh quotient minus the shift */
  double shift;                  /* mu */
  double setup_ms, triplets_ms, ratios_ms, assemble_ms, factor_ms, eig_ms;   /* set-up = checks, lists, uploads */
} theia_linear_triplet_summary;
int theia_hip_linear_triplet_positions(
    int32_t num_views, const double* orientations /*[num_views][3] angle-axis, world -> camera*/,
    int32_t num_edges, const int32_t* edges /*[num_edges][2], first < second*/,
    const double* relative_rotations /*[num_edges][3]*/, const double* relative_translations /*[num_edges][3]*/,
    int32_t num_tracks, const int32_t* track_offsets /*[num_tracks+1]*/,
    const int32_t* obs_view /*[num_obs]*/, const double* obs_feature /*[num_obs][2], normalised*/,
    const theia_linear_triplet_options* options /*NULL = defaults*/,
    double* positions_out /*[num_views][3]*/, uint8_t* estimated_out /*[num_views]*/,
    int32_t triplet_capacity, int32_t* triplets_out /*optional [triplet_capacity][3]*/,
    uint8_t* triplet_state_out /*optional [triplet_capacity]*/, double* baselines_out /*optional [triplet_capacity][3]*/,
    double* system_out /*optional*/, int32_t* system_index_out /*optional [num_views]*/,
    theia_linear_triplet_summary* summary);

/* FilterViewPairsFromRelativeTranslation (sfm/filter_view_pairs_from_relative_translation.cc:264-312, step 6 of the global
 * pipeline, sfm/global_reconstruction_estimator.cc:126-138; options: filter_view_pairs_from_relative_translation.h:48-66):
 * Wilson & Snavely's 1DSfM outlier test on the device (csrc/view_pair_filters.hip).  The translations are rotated into the
 * global frame (:67-84), their mean and variance give num_iterations random axes (:178-217), every axis orders the views by
 * the greedy minimum-feedback-arc-set heuristic of :86-160 (one workgroup per axis), and a pair whose projections
 * contradict the orderings by more than translation_projection_tolerance * num_iterations in total is removed (:236-305).
 * pairs [n_pairs][2] = (first, second) view indices, each unordered pair at most once; orientations [n_views][3] angle-axis;
 * position_2 [n_pairs][3] = TwoViewInfo::position_2.
 * Axes: three RandGaussian(mean[k], variance[k]) per iteration in the order x, y, z, iteration after iteration, from *rng,
 * which is left where the draws end (the reference with num_threads = 1); with axes_in they are used as given and rng is
 * neither read nor advanced.
 * Where the reference's result depends on the order of its hash maps, the rule here is: the lowest view index among the
 * sources, the lowest view index among equal scores, initial weights summed in pair order, iterations added in order.
 * Fewer than two pairs: the reference's variance is 0 / 0, its axes are NaN and no pair is judged; here nothing is
 * launched, removed and bad_weight are zeroed, the other outputs are left untouched, and rng still advances by the draws.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing launched, outputs and rng untouched): a view index out of range, a pair naming one
 * view twice, an unordered pair listed twice, num_iterations <= 0, a negative or NaN tolerance, rng and axes_in both NULL.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the workspace, O(num_iterations x (n_pairs + n_views)): 24 bytes per iteration and pair,
 * 4 per iteration and view, and 28 more per iteration and view beyond THEIA_MFAS_LDS_MAX_VIEWS views.
 * THEIA_MFAS_LDS_MAX_VIEWS: up to this many views (named by a pair or not) the ordering keeps its per-view state in the
 * CU's LDS; with more it runs out of a global workspace.  Same results on both routes. */
#define THEIA_MFAS_LDS_MAX_VIEWS 5632
struct theia_rng_state;
typedef struct theia_translation_filter_options {   /* filter_view_pairs_from_relative_translation.h:48-66 */
  int32_t num_iterations, reserved;                 /* 48 */
  double translation_projection_tolerance;          /* 0.08 */
} theia_translation_filter_options;
int theia_hip_filter_view_pairs_from_relative_translation(
    int32_t n_views, int32_t n_pairs, const int32_t* pairs /*[n_pairs][2]*/,
    const double* orientations /*[n_views][3]*/, const double* position_2 /*[n_pairs][3]*/,
    const theia_translation_filter_options* opt /* NULL = the defaults above */,
    struct theia_rng_state* rng /* declared below; drawn from and advanced; may be NULL when axes_in is given */,
    const double* axes_in     /* optional [num_iterations][3], unit vectors: used instead of drawing */,
    uint8_t* removed          /* [n_pairs] */,
    double* bad_weight        /* optional [n_pairs] */,
    int32_t* order            /* optional [num_iterations][n_views], -1 for a view no pair names */,
    double* axes_out          /* optional [num_iterations][3] */,
    double* rotated           /* optional [n_pairs][3]: the translations in the global frame */);

/* Host-side account of the calling thread's last theia_hip_filter_view_pairs_from_relative_translation call that launched
 * (development and timing aid, scripts/gpu_time_translation_filter.py): wall times of its stages, the ordering steps
 * that took a source and those that took the arg-max of the score (summed over the iterations), and the route taken. */
typedef struct theia_translation_filter_stats {
  double setup_ms, rotate_project_ms, order_ms, weights_ms, total_ms;   /* set-up = checks, CSR, allocation, upload */
  int64_t source_steps, argmax_steps;
  int32_t lds_route, order_threads;   /* 1: per-view state in LDS, 0: global workspace; lanes per ordering workgroup */
} theia_translation_filter_stats;
int theia_hip_translation_filter_last_stats(theia_translation_filter_stats* out);

/* FilterViewPairsFromOrientation (sfm/filter_view_pairs_from_orientation.cc:65-103, step 4 of the global pipeline): a pair
 * stays when |MultiplyRotations(-rotation_2, MultiplyRotations(r_second, -r_first))|^2 <= DegToRad(max degrees)^2 (:46-63);
 * a pair naming a view without an orientation (has_orientation[view] == 0; NULL = every view has one) is removed (:73-82).
 * removed [n_pairs].  THEIA_HIP_ERR_INVALID_ARGUMENT (nothing launched, removed untouched): a view index out of range, a
 * pair naming one view twice, an unordered pair listed twice, a negative or NaN angle (the reference's CHECK_GE). */
int theia_hip_filter_view_pairs_from_orientation(
    int32_t n_views, int32_t n_pairs, const int32_t* pairs, const double* orientations,
    const uint8_t* has_orientation /* optional [n_views]: a pair naming a view without one is removed */,
    const double* rotation_2 /*[n_pairs][3]*/, double max_relative_rotation_difference_degrees,
    uint8_t* removed);

/* FilterViewGraphCyclesByRotation (sfm/filter_view_graph_cycles_by_rotation.cc:54-145; pybind sfm.cc:926), the one filter
 * that needs no global orientations: for every triangle a < b < c (in view index) of the view graph,
 * loop = R_bc * R_ab * R_ac' (:70-71), every R the ceres::AngleAxisToRotationMatrix of that pair's rotation_2 in ascending
 * orientation, and the triangle's error is RadToDeg(|RotationMatrixToAngleAxis(loop)|) (:72-79).
 * removed[e] = !(the smallest error over the triangles of pair e < max_loop_error_degrees), strict as :132; a pair in no
 * triangle is removed.  A NaN error validates nothing: the minimum ignores it, and a pair whose errors are all NaN reports
 * +inf.  A NaN or negative threshold removes every pair (the reference has no CHECK here).
 * Extension: a pair may be listed (b, a) with b > a; its rotation_2 then belongs to that orientation and the ascending
 * matrix is its transpose (the reference's ViewIdPair is always ascending).
 * Every output is a minimum or an integer sum, so two calls on the same input give the same bytes.  num_triangles counts
 * every triangle once.  n_pairs == 0: returns 0, launches nothing, num_triangles = 0.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing launched, outputs untouched): a view index out of range, a pair naming one view
 * twice, an unordered pair listed twice, a NULL pairs, rotation_2 or removed with n_pairs > 0.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the workspace, 133 bytes per pair and 8 per view. */
int theia_hip_filter_view_graph_cycles_by_rotation(
    int32_t n_views, int32_t n_pairs, const int32_t* pairs /*[n_pairs][2] (first, second)*/,
    const double* rotation_2 /*[n_pairs][3] = TwoViewInfo::rotation_2 of (first, second)*/,
    double max_loop_error_degrees,
    uint8_t* removed                 /* [n_pairs] */,
    double*  min_loop_error_degrees  /* optional [n_pairs]: smallest loop error over the pair's triangles, +inf if none */,
    int32_t* triangles_per_pair      /* optional [n_pairs] */,
    int64_t* num_triangles           /* optional: triangles of the graph, each counted once */);

/* RemoveDisconnectedViewPairs (sfm/view_graph/remove_disconnected_view_pairs.cc:48-95; pybind sfm.cc:940), which the
 * reference pipeline runs after every filter: only the largest connected component of the view graph stays.  Largest by
 * number of views; among equally large components the one holding the smallest view index (the reference takes whichever
 * its hash map yields first, :62-69).  A view of another component gets removed_views = 1 and every pair naming it
 * removed_pairs = 1.  A view that no pair names is neither kept nor removed: removed_views = 0, component = -1.
 * No pairs: nothing is removed, returns 0.  Runs on the host (a union-find over n_views nodes) and never initialises a device.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (outputs untouched): a view index out of range, a pair naming one view twice, an unordered
 * pair listed twice, a NULL pairs, removed_pairs or removed_views with n_pairs > 0. */
int theia_hip_remove_disconnected_view_pairs(
    int32_t n_views, int32_t n_pairs, const int32_t* pairs /*[n_pairs][2]*/,
    uint8_t* removed_pairs /*[n_pairs]*/, uint8_t* removed_views /*[n_views]*/,
    int32_t* component /* optional [n_views]: smallest view index of the view's component, -1 for a view no pair names */);

/* Multi-GPU (one process per GPU): tracks are sharded by the caller; each
 * rank's handle holds its shard plus ALL cameras.  The reduced camera system
 * (and the scalar reductions) are summed across ranks through this callback,
 * which the host implements with RCCL (ncclAllReduce(sum, fp64)) -- see
 * pytheiasfm_amd/distributed.py and INTEGRATION.md.  The buffer is device
 * memory; `stream` is the hipStream_t the library enqueued its producers on. */
enum { THEIA_REDUCE_SUM = 0, THEIA_REDUCE_MAX = 1 };
typedef int (*theia_allreduce_fn)(void* ctx, void* device_buffer,
                                  size_t count_f64, int op, void* stream);
int theia_hip_ba_set_allreduce(theia_ba_handle h, theia_allreduce_fn fn,
                               void* ctx);

/* Inner iterations (options.use_inner_iterations, the reference's default) in a sharded solve.  A camera's residual blocks
 * are spread over the track shards, so each rank is given the FULL problem's observations once: after every trust-region
 * candidate the shards' candidate points are summed into the full point set (one all-reduce of 4 * num_points doubles),
 * every rank sweeps ALL cameras and intrinsics groups over the full observation set -- the same sums on every rank, nothing
 * to exchange afterwards --, then its own tracks, and the cost and the step norms of the sweep are all-reduced (4 doubles).
 * `full_problem`: the unsharded problem (same cameras and groups as the shard; every point, observation and camera prior);
 * point_global_index[shard points] = index of each of the shard's points in it.  The handle must have been created with
 * use_inner_iterations = 1.  Without this call a sharded run with inner iterations returns ERR_UNSUPPORTED.  When the
 * shard geometry is known (theia_hip_ba_set_shard / set_rccl) the cameras and the groups are dealt to the ranks by index and
 * their results summed (two more small all-reduces); otherwise every rank sweeps all of them. */
int theia_hip_ba_set_inner_global(theia_ba_handle h, const theia_ba_problem* full_problem, const int64_t* point_global_index);

/* The same all-reduce issued by the library itself: `ncclAllReduce` (RCCL) on the solve's own HIP stream, no host
 * callback inside the LM iteration.  librccl is looked up at run time (the copy the process already loaded, else
 * /opt/rocm/lib): no link-time dependency.  Rank 0 obtains the 128-byte id and hands it to the other ranks by any
 * channel the host has; every rank then creates its communicator and attaches it to its handle (which also declares
 * the shard geometry, as theia_hip_ba_set_shard).  The communicator outlives the handles using it and is destroyed
 * by the host. */
int theia_hip_rccl_unique_id(void* out128);
int theia_hip_rccl_comm_create(const void* id128, int32_t rank, int32_t world_size, void** comm_out);
int theia_hip_rccl_comm_destroy(void* comm);
/* ranks the communicator spans as RCCL itself reports them (ncclCommCount): what a scaling run quotes as its width */
int theia_hip_rccl_comm_count(void* comm, int32_t* count_out);
int theia_hip_ba_set_rccl(theia_ba_handle h, void* comm, int32_t rank, int32_t world_size);

/* ------------------------------------------------------------------ RANSAC */
/* src/theia/solvers/sample_consensus_estimator.h:58-126 */
typedef struct theia_ransac_params {
  double error_thresh;
  double failure_probability;
  double min_inlier_ratio;
  int32_t min_iterations;
  int32_t max_iterations;
  int32_t use_mle;
  int32_t use_lo;              /* LO-RANSAC: RefineModel of the absolute-pose (BundleAdjustView) and relative-pose
                                  (BundleAdjustTwoViewsAngular; also the uncalibrated one), homography
                                  (OptimizeHomography) and fundamental-matrix (OptimizeFundamentalMatrix)
                                  estimators as device batches, the default "return true" of the others */
  int32_t lo_start_iterations;
  int32_t use_Tdd_test;        /* reference: "Not currently implemented"  */
  uint32_t seed;               /* seeds the mt19937 stream (util/random.cc:60-66),
                                  i.e. RandomNumberGenerator(seed)        */
  int32_t ransac_type;         /* THEIA_RANSAC_* (create_and_initialize_ransac_variant.h:52) */
} theia_ransac_params;

/* RansacType: RANSAC = RandomSampler + InlierSupport/MLE; PROSAC = ProsacSampler
 * (prosac_sampler.cc:53-128, data sorted by quality, best first); LMED =
 * RandomSampler + LmedQualityMeasurement (lmed.h:64-70); EXHAUSTIVE =
 * ExhaustiveSampler (exhaustive_sampler.cc:45-79: every pair in order), which
 * CHECK-fails in the reference unless the estimator's sample size is 2, so it
 * is accepted for THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION only and returns
 * THEIA_HIP_ERR_INVALID_ARGUMENT with the reference's message otherwise. */
enum { THEIA_RANSAC_RANSAC = 0, THEIA_RANSAC_PROSAC = 1, THEIA_RANSAC_LMED = 2, THEIA_RANSAC_EXHAUSTIVE = 3 };

void theia_ransac_params_default(theia_ransac_params* p);

/* estimator ids: which Estimate* front-end is replaced */
enum {
  /* EstimateRelativePose, estimators/estimate_relative_pose.cc:159-172 */
  THEIA_EST_RELATIVE_POSE = 0,
  /* EstimateEssentialMatrix, estimators/estimate_essential_matrix.cc:90-106 */
  THEIA_EST_ESSENTIAL_MATRIX = 1,
  /* EstimateCalibratedAbsolutePose, estimate_calibrated_absolute_pose.cc:176-190 */
  THEIA_EST_ABSOLUTE_POSE_KNEIP = 2,
  THEIA_EST_ABSOLUTE_POSE_DLS = 3,
  THEIA_EST_ABSOLUTE_POSE_SQPNP = 4,
  /* EstimateFundamentalMatrix, estimators/estimate_fundamental_matrix.cc:105-121
   * (normalised 8-point + squared Sampson distance; the error threshold is in
   * squared pixels as in the reference) */
  THEIA_EST_FUNDAMENTAL_MATRIX = 5,
  /* EstimateHomography, estimators/estimate_homography.cc:120-135 (4-point DLT,
   * asymmetric transfer error) */
  THEIA_EST_HOMOGRAPHY = 6,
  /* EstimateDominantPlaneFromPoints, estimate_dominant_plane_from_points.cc:95-107
   * (error = point-to-plane distance, not squared) */
  THEIA_EST_DOMINANT_PLANE = 7,
  /* EstimateRelativePoseWithKnownOrientation,
   * estimate_relative_pose_with_known_orientation.cc:66-81 (2 correspondences) */
  THEIA_EST_RELATIVE_POSE_KNOWN_ORIENTATION = 8,
  /* EstimateUncalibratedRelativePose, estimate_uncalibrated_relative_pose.cc:204-220:
   * 8-point F, focal lengths from F, E = K2 F K1 decomposed with the cheirality vote;
   * data in pixels with the principal point removed.  estimator_params = {min, max}
   * focal length (both >= 1 to be applied, as in the reference). */
  THEIA_EST_UNCALIBRATED_RELATIVE_POSE = 9,
  /* EstimateAbsolutePoseWithKnownOrientation, estimate_absolute_pose_with_known_orientation.cc:132-153:
   * 2 correspondences [u v X Y Z] whose features the caller has rotated into the world frame
   * (RotateCorrespondences, :53-72); model = camera position (3) */
  THEIA_EST_ABSOLUTE_POSE_KNOWN_ORIENTATION = 10,
  /* EstimateTriangulation, estimate_triangulation.cc:69-166: one problem = one track, datum = one observation WITH ITS
   * CAMERA (PointObservation, :53-58), 33 doubles:
   *   [0..11]  projection matrix [R | -R c], row-major 3 x 4 (:122-129)
   *   [12..13] normalised feature = hnormalized(PixelToNormalizedCoordinates(pixel)) (:132-135, the caller's camera class)
   *   [14..15] observed pixel
   *   [16..21] camera extrinsics: position (3), angle-axis (3)      [22] camera model (THEIA_CAM_*)     [23..32] intrinsics
   * Minimal sample = 2 observations -> Triangulate() (triangulation.cc:109-125: essential matrix of the two poses, the
   * optimal image-point correction, DLT by the 4 x 4 SVD), kept only if the point is in front of both cameras (:82-87);
   * Error = squared pixel reprojection error through Camera::ProjectPoint, DBL_MAX when the depth is not positive (:92-101).
   * model = homogeneous point (4).  The reference runs EXHAUSTIVE over all pairs for <= 15 observations with
   * min = max iterations = n (n - 1) / 2, RANSAC otherwise (:147-159): the caller passes that choice in the parameters. */
  THEIA_EST_TRIANGULATION = 11,
  /* EstimateRadialHomographyMatrix (estimate_radial_distortion_homography.cc:52-111): datum =
   * RadialDistortionFeatureCorrespondence (estimate_radial_distortion_homography.h:56-70), 12 doubles:
   *   [0,1] feature_left  [2,3] feature_right (pixels, principal point removed)  [4,5] normalized_feature_left
   *   [6,7] normalized_feature_right  [8] focal_length_estimate_left  [9] focal_length_estimate_right
   *   [10] min_radial_distortion  [11] max_radial_distortion (read from the first datum of a sample, as the reference does).
   * EstimateModel = SixPointRadialDistortionHomography (six_point_radial_distortion_homography.cc:62-148: null space of
   * the 6 x 8 constraint, a quadratic, least-squares direction of a 6 x 5 system), up to two models per sample; Error =
   * CheckRadialSymmetricError (:201-239).  model = RadialHomographyResult: H (9, row-major), l1, l2 (then H^-1, 9 doubles,
   * kept for the scoring kernels). */
  THEIA_EST_RADIAL_HOMOGRAPHY = 12,
  /* EstimateSimilarityTransformation2D3D (estimate_similarity_transformation_2d_3d.cc:72-178): datum =
   * CameraAndFeatureCorrespondence2D3D (sfm/similarity_transformation.h / estimators header), 26 doubles:
   *   [0..2] camera.PixelToUnitDepthRay(observation).normalized() (world frame; precomputed per datum: it does not depend on
   *          the model)   [3..6] point3d (homogeneous)   [7,8] observation pixel   [9..14] camera extrinsics: position,
   *          angle-axis   [15] camera model (THEIA_CAM_*)   [16..25] intrinsics.
   * EstimateModel = GdlsSimilarityTransform on four data (gdls_similarity_transform.cc:67-228: the DLS pipeline with the
   * generalised cost matrix; Macaulay terms of one Estimate() counted from 0 as for DLS), up to 27 models; Error = squared
   * pixel error of the camera moved by the transformation (TransformCamera), DBL_MAX behind it.
   * model = SimilarityTransformation: rotation (9, row-major), translation (3), scale. */
  THEIA_EST_SIMILARITY_2D3D = 13,
  /* EstimateUncalibratedAbsolutePose (estimate_uncalibrated_absolute_pose.cc:60-141): datum = FeatureCorrespondence2D3D
   * [u v X Y Z] with the principal point removed from the pixel; sample = 4; EstimateModel = FourPointPoseAndFocalLength
   * (P4Pf, four_point_focal_length.cc:100-222), up to 10 models; Error = squared reprojection error of the projection
   * matrix (:88-97, no cheirality test).  model = the 3 x 4 projection matrix K [R | t], row-major (12 doubles); the
   * reference's DecomposeProjectionMatrix step (:124-138: rotation, position, focal length) is left to the caller (the
   * Python mirror does it).  The elimination template is not the reference's generated one. */
  THEIA_EST_UNCALIBRATED_ABSOLUTE_POSE = 14,
  /* EstimateRigidTransformation2D3D (estimate_rigid_transformation_2d_3d.cc:62-182): datum = CameraAndFeatureCorrespondence2D3D in
   * the 26-double row of THEIA_EST_SIMILARITY_2D3D ([0..2] the observation's normalised world-frame ray, [3..6] point3d, [7,8]
   * pixel, [9..14] camera position | angle-axis, [15] camera model, [16..25] intrinsics); the overload for
   * FeatureCorrespondence2D3D (:159-182) is the same call with identity pinhole cameras (focal length 1).  Sample = 4;
   * EstimateModel = Upnp::EstimatePose (pose/upnp.cc:462-493: the 8-solution symmetric template, eliminated by the reference's own
   * Gauss-Jordan), up to 8 models; Error = squared pixel error of R X + t seen by the datum's camera, DBL_MAX behind it (:116-129).
   * As in the reference, the estimator's UPnP cost parameters ACCUMULATE over the samples of one Estimate() call (upnp.cc:191-200
   * adds to a member of the one Upnp object the estimator keeps): hypothesis k is solved from the samples 0 .. k.
   * model = RigidTransformation: rotation (9, row-major), translation (3). */
  THEIA_EST_RIGID_TRANSFORMATION_2D3D = 15,
  /* EstimateRadialDistUncalibratedAbsolutePose (estimate_radial_dist_uncalibrated_absolute_pose.cc:163-189): datum =
   * FeatureCorrespondence2D3D [u v X Y Z] (pixels with the principal point removed, as they were observed: distorted); sample = 4;
   * EstimateModel = FourPointsPoseFocalLengthRadialDistortion (pose/four_point_focal_length_radial_distortion.cc:68-288 and
   * _helper.cc: the 40 x 50 elimination template reduced through Eigen::FullPivLU of its transposed 37 x 40 block, 13 x 13 action
   * matrix), up to 13 models; Error = squared distance between the feature and the projection distorted by the division model,
   * 1e10 when the translation's z is negative (:130-147).  estimator_params (required) = RadialDistUncalibratedAbsolutePoseMetaData
   * {max_focal_length, min_focal_length, max_radial_distortion, min_radial_distortion} and a fifth entry "first call of the
   * process" (0 / 1).  The solver multiplies its null-space basis by a "random rotation" made from three RandDouble(-0.5, 0.5)
   * (:134-141), and every RandomNumberGenerator object of the reference shares ONE std::mt19937 (util/random.cc:46-66): the draws
   * come out of the SAMPLER's stream, three after every sample -- reproduced here; with the fifth entry set, the stream is re-seeded
   * with 42 after the first sample, as the solver's function-static RandomNumberGenerator(42) does the first time it runs in a
   * process.  model = rotation (9, row-major), translation (3), focal_length, radial_distortion. */
  THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE = 16,
  /* CameraAlignmentEstimator of AlignReconstructionsRobust (sfm/transformation/align_reconstructions.cc:54-93): datum =
   * CameraCorrespondence [camera1 (3) | camera2 (3)], two camera positions; sample = 4; EstimateModel =
   * AlignPointCloudsUmeyama(positions2 -> positions1) on the four data (align_point_clouds.cc:56-150, in the reference's
   * sequential order), always one model: a degenerate sample (collinear, coplanar, or small -- the rule is on absolute
   * singular values) yields the identity transformation, which is scored like any other; Error = |camera1 - (s R camera2 + t)|^2.
   * RefineModel is the default "return true".  model = SimilarityTransformation: rotation (9, row-major), translation (3),
   * scale -- the layout of THEIA_EST_SIMILARITY_2D3D.  (csrc/alignment_device.h) */
  THEIA_EST_CAMERA_ALIGNMENT = 17
};

/* A batch of independent estimation problems ("pairs").  Datum layout:
 *   relative pose / essential: FeatureCorrespondence = [x1 y1 x2 y2]
 *     (matching/feature_correspondence.h; only Feature::point_ is used)
 *     (also fundamental matrix, homography, known-orientation relative pose)
 *   absolute pose: FeatureCorrespondence2D3D = [u v X Y Z]
 *     (sfm/feature_correspondence_2d_3d.h:42-49)
 *   dominant plane: Eigen::Vector3d = [X Y Z]
 *   triangulation: one observation with its camera, 33 doubles (THEIA_EST_TRIANGULATION)
 *   radial-distortion homography: RadialDistortionFeatureCorrespondence, 12 doubles (THEIA_EST_RADIAL_HOMOGRAPHY)
 *   similarity 2D-3D, rigid transformation 2D-3D: CameraAndFeatureCorrespondence2D3D, 26 doubles (THEIA_EST_SIMILARITY_2D3D)
 *   uncalibrated absolute pose (with or without radial distortion): FeatureCorrespondence2D3D = [u v X Y Z], pixels with the
 *     principal point removed
 *   camera alignment: CameraCorrespondence = [camera1 (3) | camera2 (3)] (THEIA_EST_CAMERA_ALIGNMENT) */
typedef struct theia_ransac_batch {
  int32_t estimator;           /* THEIA_EST_*                              */
  int32_t num_problems;
  const int64_t* offsets;      /* [num_problems+1] datum offsets           */
  const double* data;          /* [offsets[num_problems]][datum_size]      */
  const double* estimator_params; /* estimator constants (see THEIA_EST_*), or NULL; required (not NULL) for
                                   * THEIA_EST_UNCALIBRATED_RELATIVE_POSE and THEIA_EST_RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE */
  const uint32_t* seeds;       /* [num_problems] RandomNumberGenerator seed of each problem, or NULL = params.seed + index.
                                  Lets a caller keep a pair's sample stream when it re-batches or shards the pairs. */
} theia_ransac_batch;

/* Result per problem.  model layout:
 *   RELATIVE_POSE:    E(9, row-major) R(9, row-major) position(3)  = 21
 *   ESSENTIAL_MATRIX: E(9)                                          = 9
 *   ABSOLUTE_POSE_*:  R(9, row-major) position(3)                   = 12
 *   FUNDAMENTAL_MATRIX / HOMOGRAPHY: 3x3 row-major                  = 9
 *   DOMINANT_PLANE:   point(3) unit_normal(3)                       = 6
 *   RELATIVE_POSE_KNOWN_ORIENTATION: unit position of camera 2      = 3
 *   UNCALIBRATED_RELATIVE_POSE: F(9) R(9) position(3) focal_length1 focal_length2 = 23
 *   UNCALIBRATED_ABSOLUTE_POSE: projection matrix 3 x 4, row-major    = 12
 *   RIGID_TRANSFORMATION_2D3D: R(9, row-major) translation(3)        = 12
 *   RADIAL_DIST_UNCALIBRATED_ABSOLUTE_POSE: R(9) translation(3) focal_length radial_distortion = 14
 *   SIMILARITY_2D3D / CAMERA_ALIGNMENT: R(9, row-major) translation(3) scale = 13 */
#define THEIA_RANSAC_MODEL_STRIDE 24
typedef struct theia_ransac_result {
  int32_t* success;            /* [num_problems] Estimate() return value; 0 (with no inliers and a zero
                                * model) for a problem with fewer data than the minimal sample, where the
                                * reference's sampler CHECK-fails -- the rest of the batch still runs */
  double* models;              /* [num_problems][THEIA_RANSAC_MODEL_STRIDE]*/
  int32_t* num_inliers;        /* [num_problems]                           */
  uint8_t* inlier_mask;        /* [offsets[num_problems]] 1 = inlier       */
  int32_t* num_iterations;     /* [num_problems] RansacSummary             */
  double* confidence;          /* [num_problems]                           */
  /* totals over the batch, for hypotheses/s accounting */
  int64_t hypotheses_evaluated;/* minimal samples fitted + fully scored    */
  int64_t models_scored;       /* models scored against all data           */
  double time_fit_score_seconds; /* device time in the fit+score kernels   */
  int32_t* num_lo_iterations;  /* [num_problems] RansacSummary::num_lo_iterations, or NULL */
  double time_fit_seconds;     /* device time of the model-fit kernels (HIP events on the library's stream) */
  double time_score_seconds;   /* device time of the scoring kernels                                        */
} theia_ransac_result;

/* Replaces SampleConsensusEstimator<E>::Estimate
 * (solvers/sample_consensus_estimator.h:300-415) with Ransac<E> +
 * RandomSampler (ransac.h:57-61, random_sampler.cc:53-72), for every problem
 * of the batch.  Problem i uses RandomNumberGenerator(seed + i). */
int theia_hip_ransac_estimate_batch(const theia_ransac_batch* batch,
                                    const theia_ransac_params* params,
                                    theia_ransac_result* result);

/* ---- generator state carried across Estimate() calls
 * The reference keeps ONE thread_local std::mt19937 (util/random.cc:46-66); every RandomNumberGenerator object is a view onto
 * it, and a pipeline hands one generator to every estimate it makes, so call k starts where call k - 1 stopped.  A
 * theia_rng_state stands for that generator of one reference thread, owned by the caller.  mt + pos are exactly what
 * libstdc++'s operator<<(std::mt19937) prints (the 624 words of _M_x, then _M_p), and numpy's RandomState.get_state() key and
 * pos: a host moves the state to and from a real std::mt19937 through a stringstream. */
typedef struct theia_rng_state {
  uint32_t mt[624];             /* std::mt19937 words, in libstdc++'s order (_M_x) */
  int32_t pos;                  /* libstdc++ _M_p, 0..624; 624 right after seeding */
  int32_t p4pfr_static_seeded;  /* the P4Pfr solver's function-static RandomNumberGenerator(42) has already run */
  int64_t dls_calls;            /* DlsPnp / gDLS calls so far on this stream (4 glibc rand() draws each) */
} theia_rng_state;

/* Host only (no GPU).  seed = RandomNumberGenerator(seed) / Seed(seed): resets mt and pos only.  rand_int = n draws of
 * RandInt(lo, hi) (uniform_int_distribution<int>, libstdc++'s Lemire reduction), rand_double = n draws of RandDouble(lo, hi)
 * (generate_canonical<double, 53>: two words per draw), discard = `words` raw 32-bit outputs.  rand_gaussian = n draws of
 * RandGaussian(mean, std_dev) (util/random.cc:87-91: a fresh std::normal_distribution<double> per draw, so the polar pair's
 * second value is dropped; four words per trial, trials rejected until 0 < r2 <= 1; the number of words a draw takes does
 * not depend on mean or std_dev, which are not range-checked, as in the reference).  An argument error (NULL state,
 * pos outside [0, 624], n < 0, lo > hi) leaves the state untouched. */
int theia_hip_rng_seed(theia_rng_state* state, uint32_t seed);
int theia_hip_rng_rand_int(theia_rng_state* state, int32_t lo, int32_t hi, int32_t n, int32_t* out);
int theia_hip_rng_rand_double(theia_rng_state* state, double lo, double hi, int32_t n, double* out);
int theia_hip_rng_rand_gaussian(theia_rng_state* state, double mean, double std_dev, int32_t n, double* out);
int theia_hip_rng_discard(theia_rng_state* state, uint64_t words);

typedef struct theia_ransac_streams {
  int32_t num_streams;
  const int32_t* stream_of_problem; /* [num_problems]; NULL = every problem on stream 0 */
  theia_rng_state* states;          /* [num_streams], read at entry, advanced in place */
} theia_ransac_streams;

/* theia_hip_ransac_estimate_batch with the generators carried: the problems of one stream are successive Estimate() calls
 * of one reference thread, in increasing problem index; streams are independent threads.  After the call every state is
 * what the reference generator holds after that stream's last Estimate(): RANSAC / LMED take m RandInt per iteration (a
 * fresh index permutation per call), PROSAC its draws (its sample counter restarting per call), EXHAUSTIVE none; P4Pfr three
 * RandDouble after every sample, re-seeded with 42 after its first sample when p4pfr_static_seeded == 0 (which it then sets;
 * this replaces estimator_params[4], of which only the four limits are read); DLS / gDLS call k of a problem uses the
 * Macaulay terms of call dls_calls + k, and dls_calls grows by num_iterations.  LO refinement draws nothing.  params.seed
 * is not read and batch->seeds must be NULL.  An undersized problem gets success = 0 and leaves its stream untouched.  On
 * an argument error (a stream id out of range, pos outside [0, 624], a NULL state) nothing is written. */
int theia_hip_ransac_estimate_streams(const theia_ransac_batch* batch, const theia_ransac_params* params,
                                      const theia_ransac_streams* streams, theia_ransac_result* result);

/* Directly bound minimal solvers (src/pytheia/sfm/sfm.cc:573-592,
 * pose_wrapper.cc:166-173).  Batched: `num` independent minimal problems.
 *  five point: in = [num][5][4] (x1 y1 x2 y2), out E = [num][10][9],
 *              num_solutions[num]  (five_point_relative_pose.cc:212-293)
 *  p3p:        in = [num][3][5] (u v X Y Z), out R=[num][4][9], t=[num][4][3]
 *              (perspective_three_point.cc PoseFromThreePoints)            */
int theia_hip_five_point_relative_pose(int32_t num, const double* corr,
                                       double* essential_matrices,
                                       int32_t* num_solutions);
int theia_hip_pose_from_three_points(int32_t num, const double* corr2d3d,
                                     double* rotations, double* translations,
                                     int32_t* num_solutions);
/* SQPnP (sfm/pose/sqpnp.h:58-77, bound in src/pytheia/sfm/sfm.cc:592), batched:
 * problem i uses points [offsets[i], offsets[i+1]) of features[.][2] (normalised
 * image coordinates) and world_points[.][3] (>= 3 points, else 0 solutions).
 * Outputs per problem up to 18 solutions: quaternions[num][18][4] = [w x y z]
 * (world -> camera rotation), translations[num][18][3], zero padded. */
int theia_hip_sqpnp(int32_t num, const int64_t* offsets, const double* features,
                    const double* world_points, double* quaternions,
                    double* translations, int32_t* num_solutions);

/* DlsPnp (sfm/pose/dls_pnp.h:56-67, bound in src/pytheia/sfm/sfm.cc:577), batched like theia_hip_sqpnp; up to 27
 * solutions per problem: quaternions[num][27][4] = [w x y z] (world -> camera), translations[num][27][3], zero padded.
 * The reference mixes a random linear form into the Macaulay matrix: 100 * Eigen::Vector4d::Random() =
 * four std::rand() draws per call, never seeded (dls_pnp.cc:134).  Problem i takes the draws of the
 * call_index[i]-th DlsPnp call of a process (call_index == NULL: i).  theia_hip_dls_macaulay_terms returns those
 * terms, out[num_calls][4], from the library's restatement of glibc's rand() (host only, needs no GPU). */
int theia_hip_dls_pnp(int32_t num, const int64_t* offsets, const double* features,
                      const double* world_points, const int64_t* call_index,
                      double* quaternions, double* translations, int32_t* num_solutions);
void theia_hip_dls_macaulay_terms(int64_t first_call, int64_t num_calls, double* out);
/* P4Pf (FourPointPoseAndFocalLength, sfm/pose/four_point_focal_length.cc:100-222; bound in pose_wrapper.cc), batched:
 * corr2d3d = [num][4][5] (u v X Y Z, principal point removed), projection_matrices = [num][10][12] (3 x 4 row-major,
 * zero padded), num_solutions[num] (0 for a degenerate sample; the reference returns -1 there). */
int theia_hip_four_point_pose_and_focal_length(int32_t num, const double* corr2d3d, double* projection_matrices,
                                               int32_t* num_solutions);
/* P4Pfr (FourPointsPoseFocalLengthRadialDistortion, sfm/pose/four_point_focal_length_radial_distortion.cc:68-288; bound in
 * pose_wrapper.cc:189-215 / src/pytheia/sfm/sfm.cc:581), batched: corr2d3d = [num][4][5] (u v X Y Z, distorted pixels with the
 * principal point removed); limits = {max_focal_length, min_focal_length, max_radial_distortion, min_radial_distortion}
 * (RadialDistUncalibratedAbsolutePoseMetaData; the reference's CHECKs -> THEIA_HIP_ERR_INVALID_ARGUMENT); rotation_draws =
 * [num][3] the three RandDouble(-0.5, 0.5) each call takes from the process-wide generator (:134-138), or NULL = the draws of the
 * first num calls of a fresh process (the solver's static RandomNumberGenerator(42)).  models = [num][13][14]: rotation (9,
 * row-major), translation (3), focal length, radial distortion, zero padded; num_solutions[num] = solutions that passed the
 * focal-length / distortion range tests; num_solver_solutions[num] (may be NULL) = the solver's valid_solutions BEFORE those
 * tests -- the reference's return value is `valid_solutions.size() > 0` (:287), so it can report success with empty outputs. */
int theia_hip_four_point_focal_length_radial_distortion_ex(int32_t num, const double* corr2d3d, const double* limits,
                                                           const double* rotation_draws, double* models, int32_t* num_solutions,
                                                           int32_t* num_solver_solutions);
/* the same without the trailing output: the symbol and ABI of the earlier library versions (a caller built against the
 * six-argument declaration must not find a seven-argument function behind it) */
int theia_hip_four_point_focal_length_radial_distortion(int32_t num, const double* corr2d3d, const double* limits,
                                                        const double* rotation_draws, double* models, int32_t* num_solutions);

/* FindKNearestNeighbors of GuidedEpipolarMatcher (matching/guided_epipolar_matcher.cc:356-412), the descriptor search behind
 * the guided_matching branch of TwoViewMatchGeometricVerification::VerifyMatches (two_view_match_geometric_verification.cc:
 * 157-170), for all epiline groups of an image pair in one launch: group g has the query features q_idx[q_off[g] ..
 * q_off[g+1]) of image 1 (rows of desc1 [n1][dim]) and the candidate features c_idx[c_off[g] .. c_off[g+1]) of image 2 (rows
 * of desc2 [n2][dim]); for every query, in q order: nn_dist[2] = the two smallest squared L2 distances (float, summed over
 * the dimensions in sequence), nn_index[2] = the candidates' feature indices (ties: the earlier candidate of the list, as the
 * reference's partial_sort of (distance, position) pairs; -1 / FLT_MAX where the group has fewer than two candidates). */
int theia_hip_guided_knn(int32_t num_groups, const int64_t* q_off, const int32_t* q_idx, const int64_t* c_off,
                         const int32_t* c_idx, int32_t n1, int32_t n2, int32_t dim, const float* desc1, const float* desc2,
                         float* nn_dist, int32_t* nn_index);
/* BruteForceFeatureMatcher::MatchImagePair (matching/brute_force_feature_matcher.cc:48-115) as FeatureMatcher::MatchImages
 * (matching/feature_matcher.cc:104-228) drives it, for a whole match graph.  The squared L2 distance of two float descriptors is
 * taken in the expansion matching/distance.h:46-47 names, every operation fixed: dot = fmaf chain over k ascending from +0 (ONE
 * accumulator: the FP32 MFMA), nrm = the same chain over d[k] * d[k], d = max(fmaf(-2, dot, nrm1 + nrm2), 0).  The two nearest
 * per query are taken under (distance, candidate index) ascending (the reference's partial_sort leaves ties open); the ratio
 * test is (double)d0 < (double)(lowes_ratio * lowes_ratio) * (double)d1 with the product in float, as the reference's types make
 * it (:56-57, :77).  The reverse pass reads the same matrix by columns.  Stated deviations: a side with one candidate has
 * d1 = +inf / index -1 and passes the ratio test, a side with none yields no match (the reference reads past its vector there).
 * Both entry points return THEIA_HIP_ERR_INVALID_ARGUMENT (outputs untouched) for a descriptor with a NaN or infinite value or
 * with a squared norm beyond FLT_MAX: every distance to it would be NaN. */
typedef struct theia_brute_force_options {
  int32_t keep_only_symmetric_matches;  /* feature_matcher_options.h:66-87: true */
  int32_t use_lowes_ratio;              /* true */
  float lowes_ratio;                    /* 0.8f */
  int32_t min_num_feature_matches;      /* 30 */
  int32_t max_pairs_per_launch;         /* 0 = as many pairs per chunk as the library's workspace budget holds; the result does
                                         * not depend on it */
} theia_brute_force_options;
void theia_hip_brute_force_options_default(theia_brute_force_options* options);
/* One pair, the search alone (no ratio test, no pair rule): desc1 [n1][dim], desc2 [n2][dim]; fwd_dist / fwd_index [n1][2] = the
 * two nearest features of image 2 for every feature of image 1, rev_dist / rev_index [n2][2] the two nearest of image 1 for
 * every feature of image 2; +inf / -1 where the other side has fewer than two features. */
int theia_hip_brute_force_knn2(int32_t n1, int32_t n2, int32_t dim, const float* desc1, const float* desc2, float* fwd_dist,
                               int32_t* fwd_index, float* rev_dist, int32_t* rev_index);
/* The whole rule for num_pairs image pairs: image i has the rows feat_off[i] .. feat_off[i+1] of descriptors [total][dim]
 * (uploaded once per call), pair k matches image pair_image1[k] against pair_image2[k].  Per pair: the forward matches in
 * ascending feature1 index; with keep_only_symmetric_matches, i -> j stays iff j passed the reverse test and its nearest is i
 * (IntersectMatches, feature_matcher_utils.cc:48-70); pair_ok[k] = final count >= min_num_feature_matches (:114; the early
 * return of :82-84 is implied), and a pair that is not ok returns no matches.  match_off [num_pairs + 1]; match_feature1 /
 * match_feature2 / match_distance hold the matches of all pairs, capacity = the sum over the pairs of image 1's feature count.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (outputs untouched) for bad sizes, null arrays, image indices out of range or offsets that
 * decrease; zero pairs and images without features are valid. */
int theia_hip_brute_force_match_pairs(int32_t num_images, const int64_t* feat_off, int32_t dim, const float* descriptors,
                                      int32_t num_pairs, const int32_t* pair_image1, const int32_t* pair_image2,
                                      const theia_brute_force_options* options, uint8_t* pair_ok, int64_t* match_off,
                                      int32_t* match_feature1, int32_t* match_feature2, float* match_distance);
/* TrackBuilder (sfm/track_builder.cc:62-77, :156-209 over math/graph/connected_components.h:87-119, then
 * Reconstruction::AddTrack, reconstruction.cc:314-351) for a whole match graph in one call: the indexed matches in the CSR form
 * theia_hip_brute_force_match_pairs and the indexed verification return, the tracks in the flat form theia_ba_problem takes
 * (obs_view / obs_track are its obs_cam / obs_pt).  A node is one (view, feature), an edge one match; the edge order is pair
 * order, then match order; a pair or a match may appear more than once.  The reference's rule:
 *   1. for each edge in order, both endpoints become components of size 1 if they are new; then, unless the endpoints already
 *      share a component or size(a) + size(b) > max_track_length, the two components merge (the partition depends on the order);
 *   2. a component of fewer than min_track_length nodes is dropped (counted before rule 3);
 *   3. of the features a component holds in one view the first is kept, the others are num_inconsistent_features;
 *   4. every track has >= 2 observations: min_track_length < 2, max_track_length <= 0 and an edge inside one view are refused.
 * What the reference leaves to hash order is stated here: a node's id is feat_off[view] + feature; rule 3 keeps the LOWEST
 * feature index of a view; tracks are in ascending order of their smallest node id; the observations of a track are in ascending
 * node id (by view, then feature).  Stated deviations: the node key is the feature INDEX (the reference keys on coordinates, so
 * two indices of one view with equal coordinates are one node there; the Python mirror merges them before the call);
 * BuildTracksIncremental is not built.  The components without the cap are found on the device; those larger than
 * max_track_length are replayed on the host over their own edges in input order (stats says how many).
 * Outputs, sized by the caller: track_off [match_off[num_pairs] + 1]; obs_view / obs_feature / obs_track
 * [min(2 * match_off[num_pairs], feat_off[num_views])]; the first num_tracks + 1 / num_observations entries are written.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing written): the refusals of rule 4, a feature index outside its view, a view index
 * outside [0, num_views), offsets that do not start at 0 or that decrease, feat_off[num_views] or match_off[num_pairs] >= 2^31,
 * null arrays.  Zero pairs or zero matches: 0, num_tracks = 0, track_off[0] = 0.  THEIA_HIP_ERR_NO_DEVICE without a device:
 * there is no CPU fallback.  The result is the same on every run. */
typedef struct theia_track_builder_options {
  int32_t min_track_length;   /* reconstruction_builder.h:81-85: 2 */
  int32_t max_track_length;   /* 50 */
} theia_track_builder_options;
typedef struct theia_track_builder_stats {
  int64_t num_nodes;                      /* (view, feature) pairs that appear in a match */
  int64_t num_components;                 /* without the cap */
  int64_t num_oversized_components;       /* of those, larger than max_track_length: replayed on the host */
  int64_t num_replayed_correspondences;   /* the edges of the oversized components */
  int64_t num_small_components;           /* dropped by rule 2 (after the cap) */
  int64_t num_inconsistent_features;      /* dropped by rule 3 */
  int64_t num_tracks;
  int64_t num_observations;
} theia_track_builder_stats;
/* host clock around the phases of the calling thread's last theia_hip_build_tracks that reached the device, each ended by a
 * device synchronise */
typedef struct theia_track_builder_timings {
  double upload_ms, components_ms, replay_ms, emit_ms, download_ms, total_ms;
} theia_track_builder_timings;
void theia_hip_track_builder_options_default(theia_track_builder_options* options);
int theia_hip_build_tracks(int32_t num_views, const int64_t* feat_off, int32_t num_pairs, const int32_t* pair_view1,
                           const int32_t* pair_view2, const int64_t* match_off, const int32_t* feature1, const int32_t* feature2,
                           const theia_track_builder_options* options, int64_t* track_off, int32_t* obs_view,
                           int32_t* obs_feature, int32_t* obs_track, theia_track_builder_stats* stats);
int theia_hip_track_builder_last_timings(theia_track_builder_timings* out);
/* The image-pair selection in front of the matcher, as FeatureExtractorAndMatcher::
 * SelectImagePairsWithGlobalDescriptorMatching (sfm/feature_extractor_and_matcher.cc:356-381; on by default with 100 neighbours,
 * sfm/reconstruction_builder.h:113-118) runs it: one global descriptor per image, then GraphMatch.
 *
 * theia_hip_mean_pool_descriptors: FisherVectorExtractor::ExtractGlobalDescriptor (matching/fisher_vector_extractor.cc:56-69),
 * the element-wise mean in this fork, for every image of the flat feat_off / descriptors [total][dim] form the matcher takes:
 * pooled = +0; for the image's features in order: pooled += f (float); pooled /= float(n), correctly rounded.  Bit for bit the
 * reference's (element-wise float adds in feature order are the same whatever Eigen vectorises).  THEIA_HIP_ERR_INVALID_ARGUMENT
 * (nothing written): negative num_images, dim < 1, null arrays, feat_off that does not start at 0 or decreases, an image without
 * features (the reference's CHECK_GT, :58), num_images * dim >= 2^31, and -- the one refusal that reads the data, on the device --
 * a NaN among the descriptors (the reference's CHECK, :64).  num_images == 0 returns 0. */
int theia_hip_mean_pool_descriptors(int32_t num_images, const int64_t* feat_off, int32_t dim, const float* descriptors,
                                    float* global_descriptors /*[num_images][dim]*/);
/* theia_hip_graph_match: GraphMatch (matching/graph_match.cc:48-130) on global_descriptors [num_images][dim].  With
 * k = min(num_images - 1, num_nearest_neighbors) (:56-58), for i ascending: image i's k nearest images under (squared distance,
 * image index) ascending (the partial_sort of pair<float, int>, :78-80); for each such neighbour s, every image currently in
 * ranked[s] gets i into its expanded set (:88-92), then i and s enter each other's ranked sets (:96-97).  Selected: every ranked
 * or expanded entry (a, m) with a < m (:108-122), once.  The rule depends on the order of i, and an expanded entry (a, i) with
 * a > i is dropped, not turned around; both are kept.  The closed form the device evaluates, with kNN(x) the list above and
 * inv(x) = { y : x in kNN(y) }: a < i is selected iff i in kNN(a) or a in kNN(i); or some s is in kNN(a) and in kNN(i); or some
 * s < i has a in kNN(s) and s in kNN(i).
 * The distance, every operation fixed: d = fmaf chain over the dimensions ascending from +0.0f of (a - b) * (a - b), the float
 * subtraction first, one accumulator; symmetric bit for bit.  Stated deviation: Eigen's (a - b).squaredNorm() (:71) sums in
 * packet order, so the two can order differently two images whose distances differ in the last bits.
 * Outputs: *num_pairs is always the full count; pair_image1 < pair_image2, ascending by (image1, image2), written only when the
 * count fits pair_capacity (ask with capacity 0, call again); knn_index / knn_distance (each may be NULL) [num_images][k], row i
 * the k nearest of image i in ascending (distance, index); stats may be NULL.  The same bytes on every run.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing written, no device touched): negative sizes, dim < 1, num_nearest_neighbors < 0, null
 * arrays with non-zero sizes, num_images * dim >= 2^31, a NaN or infinite global descriptor (a NaN distance has no place in the
 * order).  num_images <= 1 or num_nearest_neighbors == 0: 0 with zero pairs, nothing launched.  THEIA_HIP_ERR_OUT_OF_MEMORY: the
 * num_images^2-bit matrix, the kNN workspace or a row of num_images bits (beyond 262 144 images) does not fit.
 * THEIA_HIP_ERR_NO_DEVICE without a device: there is no CPU fallback. */
typedef struct theia_graph_match_stats {
  int64_t num_nearest_neighbors;   /* k after the clamp to N - 1 */
  int64_t num_ranked_pairs;        /* unordered pairs with i in kNN(a) or a in kNN(i) */
  int64_t num_expanded_pairs;      /* selected by the expansion only */
  int64_t num_pairs;               /* the two together */
} theia_graph_match_stats;
int theia_hip_graph_match(int32_t num_images, int32_t dim, const float* global_descriptors, int32_t num_nearest_neighbors,
                          int64_t pair_capacity, int32_t* pair_image1, int32_t* pair_image2, int64_t* num_pairs,
                          int32_t* knn_index /* optional [num_images][k] */, float* knn_distance /* optional */,
                          theia_graph_match_stats* stats /* optional */);
/* The counting stages of the incremental estimator's inner loop (csrc/next_view.hip).
 *
 * theia_hip_visibility_scores: the VisibilityPyramid score (sfm/visibility_pyramid.cc:47-103) of every view, filled as
 * FindViewsToLocalize fills it (sfm/incremental_reconstruction_estimator.cc:437-447): view v's observations are the rows
 * [obs_off[v], obs_off[v + 1]) of obs_uv (pixels) / obs_track, and only those whose track is estimated count.  With
 * C = 1 << num_pyramid_levels the finest cell of a point is clamp((int)(C * x / width), 0, C - 1) (:71-78) and the same for y
 * with the height, in double, the product first, then the division by the size converted to double.  The reference's cast is
 * undefined for a quotient outside the int range; here the clamp is taken in double before the truncation toward zero, which is
 * the reference's result wherever it has one.  Level i (0 = the coarsest, 2 x 2) has 2^(i+1) cells per side and is the finest
 * level shifted right (:82-90); score = sum_i (occupied cells of level i) * 4^(i+1) (:97-103).  num_estimated_tracks[v] is
 * written for every view; FindViewsToLocalize's cut at 30 (:451) is the caller's.  One workgroup per view, integers only, no
 * global atomic: the same bytes on every run.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (outputs untouched): num_pyramid_levels outside 1..7 (at 8 the reference's int score overflows,
 * 16^8 = 2^32); a negative count; with num_views > 0 a NULL array, a width or height <= 0 (the reference's CHECK_GT, :54-55), a
 * track index outside [0, num_tracks), obs_off that starts below 0 or decreases; and -- the one refusal that reads the data on
 * the device -- a NaN or infinite obs_uv among the observations passed (estimated track or not).  num_views == 0 returns 0 and
 * launches nothing.  THEIA_HIP_ERR_NO_DEVICE without a device: there is no CPU fallback. */
int theia_hip_visibility_scores(int32_t num_views, const int64_t* obs_off /*[num_views+1]*/,
                                const double* obs_uv /*[total][2] pixels*/, const int32_t* obs_track /*[total]*/,
                                int32_t num_tracks, const uint8_t* track_estimated /*[num_tracks]*/,
                                const int32_t* image_size /*[num_views][2] width, height*/, int32_t num_pyramid_levels,
                                int32_t* num_estimated_tracks /*[num_views]*/, int32_t* score /*[num_views]*/);
/* theia_hip_set_underconstrained_unestimated: the estimators' SetUnderconstrainedAsUnestimated loop
 * (incremental_reconstruction_estimator.cc:612-620, global_reconstruction_estimator.cc:100-110) as written: both counts start at
 * -1; while BOTH are non-zero, SetUnderconstrainedViewsToUnestimated (reconstruction_estimator_utils.cc:321-350: every estimated
 * view with fewer than 3 estimated tracks is cleared), then SetUnderconstrainedTracksToUnestimated (:291-319: every estimated
 * track with fewer than 2 estimated views is cleared, reading the views the view pass just updated).  The condition is `&&`, not
 * a fixed point: the loop ends as soon as either pass removed nothing, so a view can be left with two estimated tracks.  Inside a
 * pass the flags that are read do not change, hence the parallel pass equals the sequential one.  view_estimated /
 * track_estimated are updated in place; views_removed / tracks_removed are totals over the rounds, *rounds the number of loop
 * iterations (each may be NULL).  The observations follow theia_ba_problem's convention, at most one per (view, track); this is
 * not validated (a repeated row would be counted twice).
 * THEIA_HIP_ERR_INVALID_ARGUMENT (nothing written): a negative count, a view or track index out of range, NULL index arrays with
 * num_obs > 0, a NULL flag array with a non-zero count.  THEIA_HIP_ERR_NO_DEVICE without a device. */
int theia_hip_set_underconstrained_unestimated(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                               const int32_t* obs_track, uint8_t* view_estimated /*in/out*/,
                                               uint8_t* track_estimated /*in/out*/, int32_t* views_removed,
                                               int32_t* tracks_removed, int32_t* rounds /*optional, each*/);
/* Pixels to camera points, normalised features and world rays for all eight camera models (csrc/unproject.hip,
 * csrc/unproject_device.h): Camera::PixelToNormalizedCoordinates and Camera::PixelToUnitDepthRay (sfm/camera/camera.cc:218-230)
 * over CameraIntrinsicsModel::ImageToCameraCoordinates (camera_intrinsics_model.cc:150-167), one lane per observation.  Every
 * model's PixelToCameraCoordinates is restated operation for operation, in the reference's order, without FMA contraction:
 *   PINHOLE pinhole_camera_model.h:213-300; PINHOLE_RADIAL_TANGENTIAL pinhole_radial_tangential_camera_model.h:222-362;
 *   FISHEYE fisheye_camera_model.h:191-341; FOV fov_camera_model.h:183-305; DIVISION_UNDISTORTION
 *   division_undistortion_camera_model.h:232-321; DOUBLE_SPHERE double_sphere_camera_model.h:189-286 (XI slot 5, ALPHA slot 6);
 *   EXTENDED_UNIFIED extended_unified_camera_model.h:189-285; ORTHOGRAPHIC orthographic_camera_model.h:188-274 (epsilon 1e-16).
 * The arrays are theia_ba_problem's: observation k is the pixel obs_uv[k] of camera obs_cam[k] (NULL: camera 0), whose
 * intrinsics are the row cam_group[camera] of `intrinsics` under the model group_model[group]; cam_ext is read only for the
 * world rays (its angle-axis half, through the library's angle-axis -> matrix routine, ceres' small-angle branch included).
 * Outputs, each optional (NULL: neither computed nor downloaded):
 *   camera_point   [n][3] ImageToCameraCoordinates
 *   normalized     [n][2] .hnormalized(): x / z, y / z -- the normalized_features row of the position, localisation and
 *                  triangulation entries
 *   world_ray      [n][3] PixelToUnitDepthRay = R' camera_point
 *   world_ray_unit [n][3] world_ray / |world_ray| -- theia_hip_estimate_tracks' obs_ray_dir
 *   status         [n] bit 0 = valid (the model's return value); bit 1 = converged: the fixed-point loop of models 0, 1, 2, 7
 *                  left by its break (or by the fisheye's early return); always set for the closed forms 3, 4, 5, 6
 *   iterations     [n] loop trips run (at most 100), 0 for the closed forms.  The reference silently returns the 100th iterate
 *                  of a loop that has not settled; so does this call, with bit 1 clear.
 * STATED DEVIATION: where a model returns false (DOUBLE_SPHERE / EXTENDED_UNIFIED beyond their domain, alpha > 0.5)
 * ImageToCameraCoordinates ignores the bool and returns an uninitialised vector; here every output of such an observation is
 * NaN and its valid bit is clear.  A NaN pixel is not refused: it propagates as in the reference.
 * *summary (optional): the counts over the call, and the kernel's and the call's time.
 * THEIA_HIP_ERR_INVALID_ARGUMENT, before the device is touched and with nothing written: a negative count; a NULL obs_uv with
 * num_obs > 0, a NULL cam_group with num_cameras > 0, a NULL intrinsics or group_model with num_groups > 0; obs_cam[k] outside
 * [0, num_cameras) (obs_cam NULL with num_obs > 0: no camera 0), cam_group[c] outside [0, num_groups), group_model[g] outside
 * 0..7; world_ray or world_ray_unit asked for with num_obs > 0 and cam_ext NULL.  num_obs == 0 returns 0 and launches nothing.
 * THEIA_HIP_ERR_NO_DEVICE without a device (there is no CPU fallback), THEIA_HIP_ERR_OUT_OF_MEMORY when a buffer cannot be had. */
typedef struct theia_unproject_summary {
  int64_t num_invalid;        /* observations with the valid bit clear                      */
  int64_t num_not_converged;  /* observations with the converged bit clear                  */
  int32_t max_iterations;     /* largest entry of `iterations`                              */
  int32_t reserved;
  double kernel_ms;           /* the kernel alone (device events)                           */
  double call_ms;             /* the whole call: validation, upload, kernel, download       */
} theia_unproject_summary;
int theia_hip_unproject(int64_t num_obs, const double* obs_uv /*[n][2]*/, const int32_t* obs_cam /*[n], NULL = camera 0*/,
                        int32_t num_cameras, const int32_t* cam_group /*[num_cameras]*/,
                        const double* cam_ext /*[num_cameras][6] position, angle-axis; NULL allowed when no world ray is asked for*/,
                        int32_t num_groups, const double* intrinsics /*[num_groups][THEIA_MAX_INTRINSICS]*/,
                        const int32_t* group_model /*[num_groups]*/,
                        double* camera_point, double* normalized, double* world_ray, double* world_ray_unit,
                        uint8_t* status, uint8_t* iterations, theia_unproject_summary* summary /*or NULL*/);
/* ---- reconstruction alignment (sfm/transformation/; csrc/alignment.hip, csrc/alignment_device.h) ----
 * AlignPointCloudsUmeyamaWithWeights (align_point_clouds.cc:56-150; weights == NULL: AlignPointCloudsUmeyama, :45-54) for a
 * batch of point-cloud pairs: problem p owns the points offsets[p] .. offsets[p + 1] of left, right [.][3] and weights [.].
 * Per problem the similarity that maps left onto right, right ~ s R left + t: rotation [p][9] row-major, translation [p][3],
 * scale [p] and status [p] (THEIA_ALIGN_OK / THEIA_ALIGN_DEGENERATE).  The arithmetic is the reference's: weighted
 * centroids, sigma of the left cloud, the centred cross-correlation over the weight sum, the Jacobi SVD of its transpose
 * (Eigen::JacobiSVD restated, csrc/small_linalg.h svd3), s(2,2) = -1 when det(U) det(V^T) <= 0, scale = (s0 + s1 + s(2,2) s2) /
 * sigma, R = U S V^T, t = right centroid - scale * (R * left centroid).
 * THEIA_ALIGN_DEGENERATE: max_sv / (min_sv + 1e-12) > 1e6 or min_sv < 1e-8 -- the reference's test, on ABSOLUTE singular
 * values (a cloud of small extent is "degenerate" whatever its shape); the result is then identity / zero / 1, as the
 * reference returns it with a warning.
 * STATED DEVIATION: the reference adds point after point; here every sum is a fixed tree (a lane's strided partial sums, then
 * the XOR butterfly over the wave, then the waves of a workgroup in order), so a call returns the same bytes on every run, but
 * not the sequential sum's last bits.  Problems of up to THEIA_ALIGN_WAVE_MAX_POINTS points take one wavefront each (four per
 * workgroup), larger ones one workgroup of 256 lanes.
 * THEIA_HIP_ERR_INVALID_ARGUMENT, before the device is touched and with nothing written: num_problems < 0; a NULL offsets,
 * left, right or output array with num_problems > 0; offsets[0] != 0 or decreasing offsets; a problem without points (the
 * reference reads left[0]); a negative weight (CHECK_GE); a problem whose weights do not sum to more than zero (CHECK_GT); a
 * non-finite coordinate or weight.  num_problems == 0 returns 0 and launches nothing.
 * timings_ms (optional, [2]): the kernels alone (device events) | the whole call. */
enum { THEIA_ALIGN_OK = 0, THEIA_ALIGN_DEGENERATE = 1 };
#define THEIA_ALIGN_WAVE_MAX_POINTS 256
int theia_hip_align_point_clouds(int32_t num_problems, const int64_t* offsets /*[num_problems+1]*/,
                                 const double* left /*[.][3]*/, const double* right /*[.][3]*/,
                                 const double* weights /*[.] or NULL = all ones*/, double* rotation /*[p][9]*/,
                                 double* translation /*[p][3]*/, double* scale /*[p]*/, int32_t* status /*[p]*/,
                                 double* timings_ms /*[2] or NULL*/);
/* TransformReconstruction (transform_reconstruction.cc:48-94) on flat arrays, in place: one lane per camera or point.
 * cameras [n][6] = position | angle-axis (theia_ba_problem's cam_ext) with camera_estimated [n] (NULL: all estimated);
 * points [m][4] homogeneous with point_estimated [m] (NULL: all).  Entries whose mask byte is 0 keep their bytes.
 *   camera position    c' = s * (R c) + t          (TransformPoint; the order is this library's STATED order: every row of
 *                      R times the vector, products added left to right, then the scale, then the translation -- Eigen's
 *                      own evaluation order of `scale * rotation * point` is not claimed)
 *   camera orientation R_cam' = R_cam R^T through ceres' AngleAxisToRotationMatrix / RotationMatrixToAngleAxis
 *                      (Camera::Get/SetOrientation..., csrc/rotation_maps.h)
 *   point              p = (x / w, y / w, z / w) (hnormalized), p' = s * (R p) + t, w' = 1 (homogeneous); w == 0 divides as
 *                      the reference does and propagates
 * As in the reference, tracks' inverse depths and reference bearing vectors are not touched.
 * THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched: a negative count; a NULL cameras / points with a non-zero
 * count; a NULL or non-finite rotation, translation or scale.  Both counts zero: returns 0, launches nothing. */
int theia_hip_transform_reconstruction(int32_t num_cameras, double* cameras /*[n][6]*/, const uint8_t* camera_estimated,
                                       int64_t num_points, double* points /*[m][4]*/, const uint8_t* point_estimated,
                                       const double* rotation /*[9] row-major*/, const double* translation /*[3]*/,
                                       double scale, double* timings_ms /*[2] or NULL*/);
/* AlignRotations (sfm/transformation/align_rotations.cc:127-156; pybind sfm.cc AlignRotations): the rotation R(w) that takes
 * `rotation` onto `gt_rotation`, rotation_i R(w) ~ gt_rotation_i, by the reference's ceres::Solve restated on the device
 * (csrc/alignment.hip k_align_rotations; the twelfth Levenberg-Marquardt loop on the rules of csrc/lm_rules.h), then
 * ApplyRotationTransformation (:100-123): rotation_i becomes AngleAxis(R(rotation_i) R(w)).  All vectors are angle-axis.
 * One 3-parameter block w starting at zero, one residual block per rotation, no loss; the residual is the reference's as
 * written, gt_i - AngleAxis(R(rotation_i) R(w)) -- a DIFFERENCE OF ANGLE-AXIS VECTORS, which wraps near pi (two nearly equal
 * rotations on either side of a half turn have a residual of about 2 pi): kept.  Jacobians in closed form, with Ceres'
 * small-angle branches (csrc/rotation_derivatives.h).  Options as the reference leaves them: function_tolerance 0 (the rule
 * then fires only on a cost that does not change at all), and Ceres 2.2's defaults -- 50 iterations, gradient tolerance
 * 1e-10, parameter tolerance 1e-8, initial radius 1e4, maximum radius 1e16, Jacobi scaling.
 * STATED DEVIATION: DENSE_QR on the 3-column Jacobian is solved as the 3 x 3 normal equations (Cholesky in registers), and
 * the sums over the rotations are fixed trees, not sequential: rounding level.  Two calls on one input return the same bytes.
 * alignment [3] (out) = w; after THEIA_ROTATION_TERM_FAILURE w = 0, as Ceres leaves a block of a failed solve as passed in,
 * and the rotations still go through ApplyRotationTransformation, as the reference applies whatever the solve left.
 * trace_out (optional) [trace_capacity][5]: (cost, gradient max norm, step norm, radius, accepted) per row, row 0 the start,
 * in theia_hip_nonlinear_rotations' convention; summary->trace_size rows are written.  Returns 0 whatever the termination.
 * THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched, with nothing but the zeroed summary written: num_rotations < 1;
 * a NULL gt_rotation, rotation or alignment; trace_capacity < 0, or > 0 with a NULL trace_out; a non-finite entry. */
typedef struct theia_align_rotations_summary {
  int32_t iterations;              /* passes of the loop, as theia_nonlinear_rotation_summary counts them */
  int32_t num_successful_steps, num_unsuccessful_steps, num_invalid_steps;
  int32_t termination;             /* THEIA_ROTATION_TERM_* */
  int32_t trace_size;
  double initial_cost, final_cost, final_radius, final_gradient_max_norm, seconds;
} theia_align_rotations_summary;
int theia_hip_align_rotations(int32_t num_rotations, const double* gt_rotation /*[n][3]*/, double* rotation /*[n][3], in/out*/,
                              double* alignment /*[3], out*/, theia_align_rotations_summary* summary /*or NULL*/,
                              double* trace_out /*optional*/, int32_t trace_capacity);
/* ---- Sim(3) point-cloud alignment (csrc/sim3_alignment.hip, csrc/sim3_device.h) ----
 * The tangent of Sim(3) is Sophus': a [7] = upsilon (3) | omega (3) | sigma, with Sim3::exp(a) = (exp(sigma) R(omega),
 * W(omega, sigma) upsilon).  (The reference's comments name another order; its code uses this one.)
 *
 * theia_hip_sim3_maps: `count` conversions, one lane each.
 *   THEIA_SIM3_MAP_EXP         in a [7]                     out sR [9] row-major | t [3]      Sophus::Sim3d::exp (sim3.hpp:557-572)
 *   THEIA_SIM3_MAP_LOG         in scale | R [9] | t [3]     out a [7]                         Sim3d(RxSO3d(scale, R), t).log() (:144-164)
 *   THEIA_SIM3_MAP_FROM_RTS    in R [9] | t [3] | scale     out a [7]                         Sim3FromRotationTranslationScale
 *                                                                                            (align_point_clouds.cc:288-298)
 *   THEIA_SIM3_MAP_TO_RTS      in a [7]                     out R [9] | t [3] | scale         Sim3ToRotationTranslationScale (:300-317)
 *   THEIA_SIM3_MAP_TO_MATRIX4  in a [7]                     out [4][4] row-major              Sim3ToHomogeneousMatrix
 *                                                                                            (transformation_wrapper.cc:125-132)
 * LOG / FROM_RTS write NaN where Sophus would abort (a scale outside [1e-10, 1e10)).  THEIA_HIP_ERR_INVALID_ARGUMENT: an
 * unknown op, count < 0, a NULL array with count > 0.  count == 0 returns 0. */
enum { THEIA_SIM3_MAP_EXP = 0, THEIA_SIM3_MAP_LOG = 1, THEIA_SIM3_MAP_FROM_RTS = 2, THEIA_SIM3_MAP_TO_RTS = 3,
       THEIA_SIM3_MAP_TO_MATRIX4 = 4 };
int theia_hip_sim3_maps(int32_t op, int64_t count, const double* in, double* out);
/* OptimizeAlignmentSim3's ceres::Solve (align_point_clouds.cc:200-282, alignment_error.h:60-161) for a batch of problems,
 * restated on the device: the thirteenth Levenberg-Marquardt loop on the rules of csrc/lm_rules.h.  Problem p owns the
 * points offsets[p] .. offsets[p + 1] of source, target [.][3], weights [.] and normals [.][3]; one 7-parameter block that
 * starts at start[p]; one residual block per point:
 *   THEIA_SIM3_POINT_TO_POINT          w_i (y_i - exp(a) x_i)                       (3 rows)
 *   THEIA_SIM3_ROBUST_POINT_TO_POINT   the same under ceres::HuberLoss(huber_threshold)
 *   THEIA_SIM3_POINT_TO_PLANE          w_i n_i . (y_i - exp(a) x_i), n_i normalised (1 row); with normals == NULL
 *                                      point-to-point, as the reference falls back (:228-238)
 * w_i = weights[i], or options[p].point_weight when weights == NULL; the weight multiplies the residual (it is not
 * squared, and may be negative or zero).  Jacobians in closed form, equal to what Ceres' Jets give in every branch of
 * Sophus' maps.  Options as :258-266 leave them with Ceres 2.2: max_num_iterations = max_iterations, function tolerance
 * 1e-6, gradient tolerance 1e-10, parameter tolerance 1e-8, initial radius 1e4, maximum radius 1e16, Jacobi scaling.
 * The entry starts where `start` says and has no policy of its own (the reference as written always starts at
 * (0,0,0,0,0,0,1); pytheiasfm_amd/alignment.py keeps that).
 * STATED DEVIATIONS: SPARSE_SCHUR over the single 7-block is solved as the 7 x 7 normal equations (Cholesky) -- the same
 * system in exact arithmetic; the sums over the points are fixed trees, not sequential: rounding level.  A problem's output
 * bytes do not depend on the other problems of the batch nor on the run.
 * Problems of up to THEIA_SIM3_GROUP_MAX_POINTS points run whole in one workgroup and one launch (all of them together);
 * a larger one runs two kernels per pass over a grid that depends on its point count only (summary.route = 1).
 * A failed factorisation, a non-finite step or a model cost change that is not positive is an invalid step; after
 * THEIA_SIM3_TERM_FAILURE (five in a row) params_out = start.  A problem without points is no error: THEIA_SIM3_TERM_NO_POINTS,
 * success 0, params_out = start (:172-175).
 * params_out [P][7]; summary_out [P]; trace_out (optional) [P][trace_capacity][5] = (cost, gradient max norm, step norm,
 * radius, accepted) per row as theia_hip_align_rotations writes them, summary.trace_size rows per problem; timings_ms
 * (optional) [2] = the kernels (device events) | the whole call.  Returns 0 whatever the terminations.
 * THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched and with no output written: num_problems < 0; a NULL offsets,
 * start, options, params_out or summary_out, or a NULL source / target with points; offsets[0] != 0 or descending offsets; a
 * non-finite coordinate, weight, normal (when normals are read) or start; a zero normal; max_iterations < 0;
 * huber_threshold <= 0 for the robust type; an unknown type; trace_capacity < 0, or > 0 with a NULL trace_out.
 * num_problems == 0 returns 0. */
enum { THEIA_SIM3_POINT_TO_POINT = 0, THEIA_SIM3_ROBUST_POINT_TO_POINT = 1, THEIA_SIM3_POINT_TO_PLANE = 2 };
enum {
  THEIA_SIM3_TERM_NO_POINTS = 0,
  THEIA_SIM3_TERM_GRADIENT_TOLERANCE = 1,    /* 1, 2, 3, 6: ceres::CONVERGENCE */
  THEIA_SIM3_TERM_FUNCTION_TOLERANCE = 2,
  THEIA_SIM3_TERM_PARAMETER_TOLERANCE = 3,
  THEIA_SIM3_TERM_MAX_ITERATIONS = 4,        /* ceres::NO_CONVERGENCE */
  THEIA_SIM3_TERM_FAILURE = 5,               /* ceres::FAILURE */
  THEIA_SIM3_TERM_MIN_RADIUS = 6
};
/* The largest problem of the group route.  Measured on the MI355X. */
#define THEIA_SIM3_GROUP_MAX_POINTS 4096
typedef struct theia_sim3_alignment_options {
  int32_t alignment_type;          /* THEIA_SIM3_* */
  int32_t max_iterations;
  double point_weight;
  double huber_threshold;
} theia_sim3_alignment_options;
typedef struct theia_sim3_alignment_summary {
  int32_t termination;             /* THEIA_SIM3_TERM_* */
  int32_t success;                 /* 1 iff ceres::CONVERGENCE (:269) */
  int32_t num_iterations;          /* Ceres' summary.iterations.size() (:271): iteration 0 and every iteration that ended
                                      in an accepted, rejected or (non-final) invalid step */
  int32_t num_successful_steps, num_unsuccessful_steps, num_invalid_steps;
  int32_t trace_size;
  int32_t route;                   /* 0: one workgroup; 1: the grid */
  double initial_cost, final_cost;
  double alignment_error;          /* mean |y_i - exp(a) x_i|, unweighted, at params_out (:275-281) */
} theia_sim3_alignment_summary;
int theia_hip_optimize_alignment_sim3(int32_t num_problems, const int64_t* offsets /*[P+1]*/, const double* source /*[.][3]*/,
                                      const double* target /*[.][3]*/, const double* weights /*[.] or NULL*/,
                                      const double* normals /*[.][3] or NULL*/, const double* start /*[P][7]*/,
                                      const theia_sim3_alignment_options* options /*[P]*/, double* params_out /*[P][7]*/,
                                      theia_sim3_alignment_summary* summary_out /*[P]*/, double* trace_out /*optional*/,
                                      int32_t trace_capacity, double* timings_ms /*[2] or NULL*/);
/* ---- Sim(3) pose-graph optimisation of camera poses (csrc/pose_graph_sim3.hip, csrc/pose_graph_sim3_device.h; DESIGN.md
 * 3.6x) ----
 * The problem AlignOverlapReconstructionsWithPointsAndPosesRobust declares (sfm/transformation/align_reconstructions.h:61-68)
 * and the reference never defines, built from the pieces it ships: one Sim3ReconAlignErrorTerm
 * (pose_graph_sim3_error.h:46-103) per edge, every node a 7-vector on Sim3Manifold
 * (align_reconstructions_pose_graph_optim.cc:39-81), nodes optionally held (SetParameterBlockConstant), solved by Ceres 2.2's
 * TrustRegionMinimizer + LevenbergMarquardtStrategy at ceres::Solver::Options' defaults, restated on the device in FP64: the
 * fourteenth Levenberg-Marquardt loop on the rules of csrc/lm_rules.h.
 * nodes [num_nodes][7], in/out, tangents in Sophus' order upsilon | omega | sigma (a camera: log(Sim3(RxSO3(1, R_c_w),
 * -R_c_w C)), align_reconstructions_pose_graph_optim_test.cc:71-79).  edges [num_edges][2] = (i, j) with measurements
 * [num_edges][7] = log(Sji) and sqrt_information [num_edges][7][7] row-major, or NULL: identity.  Per edge
 *   r = log(Sji exp(x_i) exp(x_j)^-1),  residual = sqrt_information r  (7 rows),
 *   J_i = sqrt_information (I + Jr0 / 2 + Jr0^2 / 12) Adj(exp(x_j)),  J_j = -J_i,
 * Jr0 from the unweighted r with blocks (0,0) = hat(omega_r) + sigma_r I, (0,3) = hat(upsilon_r), (0,6) = -upsilon_r,
 * (3,3) = hat(omega_r); Adj is Sophus' (sim3.hpp).  These are the reference's hand-written Jacobians: the derivative along
 * the manifold's Plus as a truncated series, not the derivative in the ambient vector; they are restated as written.
 * Plus(x, d) = log(exp(x) exp(d')), d'[6] = max(d[6], -20); PlusJacobian is the identity.  The measurement that makes an
 * edge's residual zero is log(exp(x_j) exp(x_i)^-1).
 * fixed [num_nodes] non-zero = held constant (no columns, not in |x|, bits unchanged), or NULL: no node is held -- the
 * gauge (a common similarity on the right) is then free and only the LM diagonal makes the system definite.  A "cross edge"
 * to another reconstruction is an edge to a held node with an identity measurement.  A node without an edge is not in the
 * problem and is left untouched; an edge between two held nodes is not in the problem either; repeated and reversed pairs
 * add up.
 * The system is the dense normal equations of order 7m, m = the free nodes that have an edge (STATED DEVIATION: Ceres would
 * pick a sparse Cholesky -- the same system in exact arithmetic; the sums are trees and the group products are formed on
 * (scale, R, t), not on Sophus' quaternions: rounding level; the gradient max norm is that of the tangent-space gradient, as
 * in every loop of the library).  A pivot that is not positive, a non-finite step, a Plus whose logarithm leaves Sophus' scale
 * range [1e-10, 1e10) and a model cost change that is not positive are invalid steps, not errors; after
 * THEIA_SIM3_TERM_FAILURE (five in a row) the nodes are as passed in, after the cap they hold the last accepted iterate.
 * summary->termination takes the THEIA_SIM3_TERM_* codes (NO_POINTS: nothing to solve, every node of every edge is held).
 * trace_out (optional) [trace_capacity][5]: (cost, gradient max norm, step norm, radius, accepted) per row, row 0 the start,
 * then one row per iteration, in theia_hip_nonlinear_rotations' convention; summary->trace_size rows are written.  Two calls
 * on one input give the same bytes.  Returns 0 whatever the termination.
 * THEIA_HIP_ERR_INVALID_ARGUMENT (checked before the device is touched; nothing written): a NULL summary, nodes, edges or
 * measurements; no node; no edge; an edge naming a node out of range; an edge from a node to itself; a non-finite node,
 * measurement or sqrt_information entry; max_num_iterations < 0; a tolerance that is negative or not finite (zero switches
 * a rule off, as in Ceres); a radius that is not positive and finite; trace_capacity < 0, or > 0 with a NULL trace_out.
 * THEIA_HIP_ERR_OUT_OF_MEMORY: the dense (7m + 1)^2 array of doubles does not fit on the device. */
typedef struct theia_pose_graph_sim3_options {
  int32_t max_num_iterations;          /* 50 */
  int32_t reserved;
  double function_tolerance;           /* 1e-6 */
  double gradient_tolerance;           /* 1e-10 */
  double parameter_tolerance;          /* 1e-8 */
  double initial_trust_region_radius;  /* 1e4 */
  double max_trust_region_radius;      /* 1e16 */
} theia_pose_graph_sim3_options;
typedef struct theia_pose_graph_sim3_summary {
  int32_t iterations;              /* as theia_nonlinear_rotation_summary */
  int32_t num_successful_steps, num_unsuccessful_steps, num_invalid_steps;
  int32_t termination;             /* THEIA_SIM3_TERM_* */
  int32_t num_nodes_in_problem;    /* m */
  int32_t trace_size, reserved;
  double initial_cost, final_cost, final_radius, final_gradient_max_norm, seconds;
  double kernel_ms;                /* device events around the call's kernels */
} theia_pose_graph_sim3_summary;
int theia_hip_pose_graph_sim3(int32_t num_nodes, double* nodes /* [n][7], in/out */, const uint8_t* fixed /* [n] or NULL */,
                              int32_t num_edges, const int32_t* edges /* [E][2] */, const double* measurements /* [E][7] */,
                              const double* sqrt_information /* [E][7][7] or NULL */,
                              const theia_pose_graph_sim3_options* options /*NULL = defaults*/,
                              theia_pose_graph_sim3_summary* summary, double* trace_out /* optional */,
                              int32_t trace_capacity);
/* ---- co-visibility: from a reconstruction back to a view graph, and on to dense stereo (csrc/covisibility.hip; DESIGN.md
 * 3.6w) ----
 * The four entries read a reconstruction as flat arrays: observation k is (obs_view[k], obs_track[k]), rows in any order, at
 * most one per (view, track) as in theia_ba_problem (not validated: a repeated row is counted twice); view_estimated
 * [num_views] and track_estimated [num_tracks] (each NULL: all estimated); cam_ext [num_views][6] = position | angle-axis;
 * points [num_tracks][4] homogeneous.  Every call builds two CSR forms on the host, by three counting passes: the
 * observations by view with every view's tracks ascending, and by track with every track's views ascending; all kernels
 * read these.  Device memory: 8 bytes per observation, 21 per view and 9 per track for the plan, the flags and the row
 * counters (69 and 42 where the poses and points are read); 12 per emitted pair, 48 more with the edge data, 12 more
 * with the scores.  Host memory: 12 bytes per observation.
 * Common refusals, THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched and with every output untouched: a
 * negative count; a view or track index out of range; a NULL required array with a non-zero count.  THEIA_HIP_ERR_NO_DEVICE
 * without a device (there is no CPU fallback); THEIA_HIP_ERR_OUT_OF_MEMORY when one of the buffers above cannot be had.
 * Everything that decides an output's position is integer arithmetic without a global atomic, every floating-point sum has
 * a fixed order, and no floating-point atomic is used: the same input gives the same bytes.
 *
 * theia_hip_covisibility_graph: ViewGraphFromReconstruction (sfm/view_graph/view_graph_from_reconstruction.cc:41-105).
 * For every pair i < j of estimated views, shared = the number of estimated tracks both observe (:63-71, :94-97); the pair
 * is emitted when shared > min_shared_tracks (:99, strict).  pairs [.][2] ascending in (i, j); num_shared [.] =
 * num_verified_matches (:58); optional rotation_2 [.][3] = RotationMatrixToAngleAxis(R_j * R_i') (:47-53, Eigen's product
 * order, ceres' maps as csrc/rotation_maps.h restates them) and position_2 [.][3] = R_i * (c_j - c_i).normalized() (:55-57),
 * the difference divided by sqrt((x x + y y) + z z) without a guard: coincident centres give NaN, which is passed
 * through, not refused (Eigen from 3.3 on returns the zero vector there instead).
 * *num_pairs is always the full count; the arrays are written only when it fits pair_capacity (ask with capacity 0, call
 * again), as theia_hip_graph_match does it.
 * One workgroup per row i counts in int32 counters in its LDS, one per column of a window of column_window views
 * (0 = THEIA_COVISIBILITY_DEFAULT_WINDOW, the 32 KiB the kernel declares; larger values are clamped to it); a row with
 * more columns j > i than one window takes further passes.  The result does not depend on the window.
 * STATED DEVIATIONS: the reference walks ViewIds() in hash-map order and tests only the outer view for IsEstimated(), so
 * which view is "1" of the TwoViewInfo, and whether a pair with one unestimated view appears, depend on that order.  Here
 * view 1 is the smaller index and BOTH views must be estimated (the only consumer, ViewSelectionMVSNet :82, skips an
 * unestimated neighbour anyway).
 * Further refusals: min_shared_tracks < 0, column_window < 0, pair_capacity < 0, a NULL num_pairs, a NULL pairs or
 * num_shared with pair_capacity > 0, rotation_2 or position_2 asked for with cam_ext NULL.  num_views == 0 or
 * num_obs == 0: *num_pairs = 0, returns 0, launches nothing. */
#define THEIA_COVISIBILITY_DEFAULT_WINDOW 8192
int theia_hip_covisibility_graph(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                 const int32_t* obs_track, const uint8_t* view_estimated, const uint8_t* track_estimated,
                                 const double* cam_ext /*[num_views][6]; NULL allowed without edge data*/,
                                 int32_t min_shared_tracks, int32_t column_window, int64_t pair_capacity,
                                 int32_t* pairs /*[.][2]*/, int32_t* num_shared /*[.]*/, double* rotation_2 /*optional [.][3]*/,
                                 double* position_2 /*optional [.][3]*/, int64_t* num_pairs);
/* theia_hip_mvsnet_pair_scores: the score of ViewSelectionMVSNet (mvs/view_selection_mvsnet.cc:39-52, :89-104) for a list
 * of view pairs (the list above, or any; a pair may be listed more than once and in either order):
 *   score[e] = sum over the tracks t both views observe, ascending in t, of ScoreFun(theta_t),
 * with p = xyz / w (hnormalized), ray = (c - p) / sqrt((x x + y y) + z z) for both centres, theta = 180 / pi * acos((r1 r2)_x
 * + ..., products added left to right), sigma = theta <= theta0 ? sigma1 : sigma2, and exp(-(d * d) / (2 * sigma * sigma)),
 * d = theta - theta0 (the reference's pow(., 2) as a product).  As at :89-104 EVERY common track counts, estimated or not;
 * track_mask [num_tracks] (optional) restricts the sum to the tracks whose byte is not 0.  The cosine is not clamped, as in
 * the reference: a NaN term makes the score NaN.  num_common [e] = the number of terms.
 * One team of 16 lanes per pair strides over the shorter of the two sorted track lists and bisects in the longer; a lane
 * adds its hits in ascending order, then one fixed reduction over the team: the order of the sum is a function of the
 * input alone.  A pair is evaluated as (smaller view, larger view), so (i, j) and (j, i) get the same bits.
 * STATED DEVIATION: the reference calls std::set_intersection on View::TrackIds(), the keys of an unordered_map in hash
 * order, which is undefined; the intersection of the sorted lists is what it means.  The sum's association differs from the
 * reference's sequential one at rounding level.
 * Further refusals: a pair naming one view twice; a NaN theta0, sigma1 or sigma2; a sigma of 0; a NULL cam_ext, points,
 * pairs, score or num_common with num_pairs > 0.  num_pairs == 0 returns 0; num_obs == 0 writes zeros; neither launches. */
int theia_hip_mvsnet_pair_scores(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                 const int32_t* obs_track, const double* cam_ext /*[num_views][6]*/,
                                 const double* points /*[num_tracks][4]*/, const uint8_t* track_mask /*optional*/,
                                 int64_t num_pairs, const int32_t* pairs /*[num_pairs][2]*/, double theta0, double sigma1,
                                 double sigma2, double* score /*[num_pairs]*/, int32_t* num_common /*[num_pairs]*/);
/* theia_hip_view_selection_mvsnet: ViewSelectionMVSNet (mvs/view_selection_mvsnet.cc:54-125) in one call: the graph above
 * with min_shared_tracks (the reference's literal 10, :66), the scores above on its pairs without a mask, and for every
 * estimated view its num_neighbors best neighbours.  neighbor [num_views][num_neighbors] (-1 padded), score likewise
 * (0 padded), best first: score descending, NaN after every number, equal scores (and NaNs) by ascending view index.  An
 * unestimated view gets an empty row.  The graph and the scores run on the device and stay there in between; the selection,
 * at most a view's degree items, runs on the host.
 * STATED DEVIATION: the reference keys a std::map by the score (:78, :105), so two neighbours with one score collapse into
 * one, and which of them survives depends on hash order.  Here both stay.
 * Further refusals: num_neighbors < 0, min_shared_tracks < 0, column_window < 0, NaN theta0 / sigma1 / sigma2, a sigma of 0, a
 * NULL cam_ext or points with num_views > 0, a NULL output with num_views * num_neighbors > 0.  num_views == 0 returns 0;
 * num_obs == 0 writes empty rows; neither launches. */
int theia_hip_view_selection_mvsnet(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                    const int32_t* obs_track, const uint8_t* view_estimated, const uint8_t* track_estimated,
                                    const double* cam_ext, const double* points, int32_t min_shared_tracks /*reference: 10*/,
                                    int32_t num_neighbors, double theta0, double sigma1, double sigma2, int32_t column_window,
                                    int32_t* neighbor /*[num_views][num_neighbors]*/, double* score /*likewise*/);
/* theia_hip_find_common_tracks: FindCommonTracksInViews (sfm/find_common_tracks_in_views.cc:58-88) for a batch of queries:
 * query q is the views views[offsets[q] .. offsets[q + 1]), and its answer the ascending list of the tracks every one of
 * them observes, estimated or not, as the reference does (a view may be named twice).  One team of 16 lanes per query:
 * the candidates are the shortest of the views' lists (the first such view of the query), each bisected in the others;
 * count, scan, write.  track_off [num_queries + 1] and *num_found are always written; tracks only when *num_found fits
 * track_capacity (ask with capacity 0, call again).
 * Further refusals: a NULL offsets, views, track_off or num_found with num_queries > 0; offsets[0] != 0 or a query with
 * fewer than 2 views (the reference's CHECK_GT, :60); track_capacity < 0, or > 0 with a NULL tracks.  num_queries == 0
 * returns 0; num_obs == 0 gives empty answers; neither launches. */
int theia_hip_find_common_tracks(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                 const int32_t* obs_track, int32_t num_queries, const int64_t* offsets /*[num_queries+1]*/,
                                 const int32_t* views, int64_t track_capacity, int64_t* track_off /*[num_queries+1]*/,
                                 int32_t* tracks, int64_t* num_found);
/* n draws of RandomNumberGenerator(seed).RandInt(lo, hi) (util/random.cc:46-84): host code that follows the reference's
 * generator outside the RANSAC sampler (the random candidates of GuidedEpipolarMatcher::FindFeaturesNearEpipolarLines). */
int theia_hip_randint_stream(uint32_t seed, int32_t n, int32_t lo, int32_t hi, int32_t* out);
/* Self-check of the cross-lane primitives the bit-exact kernels stand on (wave_reduce.h: the XOR-butterfly sums on permlane swaps
 * + DPP, the wave maximum of |a| as two unsigned reductions, the row broadcasts) against plain shuffle loops on `count` random
 * wavefronts; *mismatches = lanes whose bits differ (0 on a device / compiler the library is right for).  No reference
 * counterpart: a maintainer's first call on new hardware. */
int theia_hip_selftest_wave_primitives(int32_t count, int32_t* mismatches);
/* Self-checks of the team linear algebra of the minimal solvers (csrc/selftest_team_solvers.hip): each runs the team routine in
 * its production launch shape and the one-thread routine it is bit-identical to on `count` caller-supplied inputs and returns
 * both results, for the tests to compare.  No reference counterpart.  THEIA_HIP_ERR_INVALID_ARGUMENT for a bad variant / team /
 * n, count < 1 or a null pointer.  The output buffers are read as well: records the kernels do not write keep their contents.
 * eig_team: variant 0 = eig_team<8, false> (k_fit5_b), n in [1, 10]; 1 = eig_team<8, true> (k_upnp_b, k_p4pfr_b), n in
 * [1, 13]; 2 = eig_team<32, true, 4> with V = X = the matrix's global slot and the rows {0, 9, 3, 1} kept (k_dls_b_team),
 * n in [10, 27]; against eig_general_t<10, false>, <13, true>, <27, true>.  A [count][n][n] row-major; active [count]: 0 =
 * the team returns at once and neither record is written.  Record per matrix, 1 + 2 n + 2 n^2 doubles: ok | wr [n] | wi [n]
 * | H [n][n] (the Schur form; the one-thread H of a second run without vectors) | V [n][n] (variant 2, team: the 4 kept
 * rows, 4 x n).  One-thread ok = -1: its runs with and without vectors disagreed. */
int theia_hip_selftest_eig_team(int32_t variant, int32_t n, int32_t count, const double* A, const int32_t* active,
                                double* team_out, double* single_out);
/* svd9_team<team> (team 5: k_sqp_b / k_hom_b, 9: the earlier shape), with V accumulated or not, against svd_sq<9>.  A
 * [count][9][9]; record per matrix, 171 doubles: U [81] | S [9] | V [81] (the team's V only when with_v). */
int theia_hip_selftest_svd9_team(int32_t team, int32_t with_v, int32_t count, const double* A, double* team_out,
                                 double* single_out);
/* five_point_pre_team<16> (k_fit5_a_team) against five_point_pre.  corr [count][5][4] = (x1, y1, x2, y2); record per
 * problem, 137 doubles: ok | N [9][4] | M [10][10] (N and M only when ok). */
int theia_hip_selftest_five_point_pre_team(int32_t count, const double* corr, double* team_out, double* single_out);
/* Self-checks of the rotation maps of the global-pose stages, one lane per case in 256-thread workgroups, on `count`
 * caller-supplied cases; the tests compare the results with 50-digit arithmetic.  No reference counterpart.
 * THEIA_HIP_ERR_INVALID_ARGUMENT for count < 1, a null pointer or a width that is not positive and finite.
 * rotation_maps (csrc/selftest_rotation_maps.hip): a, b [count][3] angle-axis; record per case, 18 doubles:
 * angle_axis_to_rot(a) [3][3] row-major | rot_to_angle_axis of that matrix [3] | multiply_rotations(a, b) [3] |
 * eigen_rot_to_rotvec of that matrix [3].
 * pairwise_rotation_error (csrc/nonlinear_rotations.hip): the edge record of the NONLINEAR rotation estimator's
 * linearisation for w_i, w_j, rel [count][3], both views free, unit Jacobi scale, SoftL1 of `width`; record per case, 22
 * doubles: J_i [3][3] | J_j [3][3] (row-major, corrected) | corrected residual [3] | the logarithm's branch (0: trace >= 0;
 * 1 + i: largest diagonal entry i). */
int theia_hip_selftest_rotation_maps(int32_t count, const double* a, const double* b, double* out);
int theia_hip_selftest_pairwise_rotation_error(int32_t count, const double* w_i, const double* w_j, const double* rel,
                                               double width, double* out);
/* Self-check of the Sim(3) pose graph's edge term (csrc/pose_graph_sim3.hip): the linearisation's code alone, one lane per
 * edge, on x_i, x_j, measurements [num_edges][7] and sqrt_information [num_edges][7][7] (or NULL: identity);
 * residual_out [num_edges][7] = sqrt_information log(Sji exp(x_i) exp(x_j)^-1), jacobian_i_out [num_edges][7][7] row-major =
 * J_i (J_j is its negative); both NaN where the logarithm is not defined.  The tests compare with tests/pose_graph_sim3_ref.py.
 * THEIA_HIP_ERR_INVALID_ARGUMENT for num_edges outside 1 .. 2^20 or a null pointer other than sqrt_information. */
int theia_hip_selftest_sim3_pose_graph_term(int32_t num_edges, const double* x_i, const double* x_j, const double* measurements,
                                            const double* sqrt_information, double* residual_out, double* jacobian_i_out);
/* Self-check of the trust-region step rules of every Levenberg-Marquardt loop (csrc/lm_rules.h, played by
 * csrc/selftest_lm_rules.hip): a script of 1 .. 16 records runs from a fresh state (radius 1e4, decrease factor 2) once in
 * one device thread and once on the host; the tests compare both with a restatement of Ceres' rules.  No reference
 * counterpart.  THEIA_HIP_ERR_INVALID_ARGUMENT for a count outside 1 .. 16 or a null pointer.
 * records [count][4] = op | a | b | c with op 1: an invalid step; 2: an evaluated step, a = rho, b = max_radius (accepted
 * iff rho > 1e-3, else rejected); 3: the rules before a step, a = gradient max norm, b = gradient_tolerance; 4: the
 * parameter rule, step norm | x norm | tolerance; 5: the function rule, cost | candidate cost | tolerance; 6: the LM
 * diagonal of a at radius b; 7: the Jacobi scale of the squared column norm a; 8, 9: the model cost change on 3 x 3, 6 x 6
 * with packed H[k] = a + k, g[i] = b + i, y[i] = c - i.
 * Output per record, 7 doubles: radius | decrease factor | invalid steps in a row | last step successful | the rule's
 * decision (op 1: 0 = the fifth in a row, the solve fails) | the value (op 2: the radius had the cube been pow(t, 3)) |
 * 1 when the radius floor 1e-32 is reached. */
int theia_hip_selftest_lm_rules(int32_t count, const double* records, double* device_out, double* host_out);

/* The batch entry points above keep their device workspace and the pinned host blocks of their per-round transfers in
 * process-wide caches between calls (up to 6 GiB of device memory and 2 GiB of pinned host memory); the buffers of a
 * destroyed BA handle and the host staging of theia_hip_ba_create go to the same caches, so that a pipeline that
 * solves problem after problem does not pay hipMalloc / hipFree and page faults each time.  This returns both caches
 * to the runtime.  All RANSAC kernels of
 * the process run on one library-owned stream; calls from several host threads are safe and overlap their host work. */
void theia_hip_release_scratch(void);

#ifdef __cplusplus
}
#endif
#endif /* THEIA_HIP_H_ */
