/*
 * gsx.h — C ABI of the MI355X-native sparse nonlinear-least-squares backend.
 *
 * One shared library (libgsx.so, built by hipcc for gfx950) exports exactly the
 * entry points below.  Plain pointers and sizes only: no C++ types, no torch
 * types, no exceptions across the boundary.  Every function returns a
 * gsx_status (0 = OK).  All floating point is FP64, keys are uint64_t
 * (gtsam::Key, gtsam/base/types.h:97), indices are int32_t.
 *
 * What each entry point replaces in the reference (paths relative to
 * /root/reference/):
 *
 *   gsx_create / gsx_destroy     lowering of NonlinearFactorGraph + Values
 *                                (gtsam/nonlinear/NonlinearFactorGraph.h,
 *                                 gtsam/nonlinear/Values.h:74-79)
 *   gsx_set_ordering             params.ordering / Ordering::Create
 *                                (gtsam/nonlinear/LevenbergMarquardtParams.h:112-117),
 *                                symbolic analysis = EliminationTree ctor
 *                                (gtsam/inference/EliminationTree-inst.h:78-156) +
 *                                JunctionTree ctor (gtsam/inference/JunctionTree-inst.h:51-153)
 *   gsx_compute_ordering         Ordering::Create for the stand-alone harness
 *                                (gtsam/inference/Ordering.h:217-236); NOT ccolamd — own
 *                                minimum-degree / nested-dissection / Schur orderings
 *   gsx_set_values/get_values    Values insert/at (gtsam/nonlinear/Values.h)
 *   gsx_error                    NonlinearFactorGraph::error
 *                                (gtsam/nonlinear/NonlinearFactorGraph.cpp:170-179)
 *   gsx_linearize                NonlinearFactorGraph::linearize
 *                                (gtsam/nonlinear/NonlinearFactorGraph.cpp:239-278)
 *   gsx_get_jacobians            the JacobianFactor [A b] blocks
 *                                (gtsam/linear/JacobianFactor-inl.h:62-100)
 *   gsx_hessian_diagonal         GaussianFactorGraph::hessianDiagonal
 *                                (gtsam/linear/GaussianFactorGraph.cpp:279-287)
 *   gsx_solve                    buildDampedSystem + NonlinearOptimizer::solve
 *                                (gtsam/nonlinear/internal/LevenbergMarquardtState.h:125-156,
 *                                 gtsam/nonlinear/NonlinearOptimizer.cpp:132-179) =
 *                                eliminateMultifrontal(EliminatePreferCholesky) +
 *                                GaussianBayesTree::optimize
 *                                (gtsam/inference/EliminateableFactorGraph-inst.h:123-146,
 *                                 gtsam/linear/HessianFactor.cpp:515-551,
 *                                 gtsam/base/cholesky.cpp:108-159,
 *                                 gtsam/linear/linearAlgorithms-inst.h:49-117)
 *   gsx_linear_error             GaussianFactorGraph::error
 *                                (gtsam/linear/GaussianFactorGraph.cpp:71-78)
 *   gsx_retract                  Values::retract (gtsam/nonlinear/Values.cpp:53-64,99-101)
 *   gsx_lm_optimize / _iterate   LevenbergMarquardtOptimizer::optimize / iterate
 *                                (gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-308,
 *                                 gtsam/nonlinear/NonlinearOptimizer.cpp:62-117,182-231)
 *   gsx_gn_optimize              GaussNewtonOptimizer::iterate
 *                                (gtsam/nonlinear/GaussNewtonOptimizer.cpp:44-66)
 *   gsx_initialize_pose3         InitializePose3::initialize (gtsam/slam/InitializePose3.cpp:296-319) and its
 *                                stages: see "Pose3 initialization" below
 *   gsx_solve_gfg                GaussianFactorGraph::optimize(ordering, EliminatePreferCholesky)
 *                                (gtsam/linear/GaussianFactorGraph.cpp:316-319) — the
 *                                NonlinearOptimizer::solve seam
 *                                (gtsam/nonlinear/NonlinearOptimizer.h:129-130)
 *
 * Threading: a handle is NOT thread-safe; distinct handles are independent.
 * One handle = one device + one HIP stream.  The library fails with
 * GSX_E_NO_DEVICE when no gfx950 device is usable: there is no CPU fallback.
 */
#ifndef GSX_H_
#define GSX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsx_context* gsx_handle;

/* ---- status codes ------------------------------------------------------- */
typedef enum gsx_status {
  GSX_OK = 0,
  GSX_E_INVALID = 1,        /* bad argument / malformed description            */
  GSX_E_NO_DEVICE = 2,      /* no usable gfx950 device / HIP error             */
  GSX_E_BAD_ORDERING = 3,   /* ordering is not a permutation of the variables  */
                            /* (EliminationTree-inst.h:137-141)                */
  GSX_E_INDETERMINATE = 4,  /* IndeterminantLinearSystemException              */
                            /* (gtsam/linear/linearExceptions.h:94-97)         */
  GSX_E_STATE = 5,          /* call sequence error (e.g. solve before linearize)*/
  GSX_E_NOMEM = 6
} gsx_status;

/* ---- variable types (state layout / tangent dim) ------------------------ */
enum {
  GSX_VAR_VECTOR = 0, /* R^d: state d, tangent d (Point2/Point3/generic)       */
  GSX_VAR_POSE2 = 1,  /* state (x,y,theta), tangent (x,y,theta)                */
  GSX_VAR_POSE3 = 2,  /* state R row-major 9 + t 3, tangent (omega3, v3)       */
  GSX_VAR_CAMERA = 3, /* PinholeCamera<Cal3Bundler>: Pose3 state 12 +          */
                      /* (f,k1,k2,u0,v0); tangent (pose 6, f, k1, k2)          */
  GSX_VAR_ROT3 = 4,   /* Rot3: state R row-major 9, tangent omega 3; retract R Expmap(omega), local
                         coordinates Logmap(R1' R2) (gtsam/geometry/Rot3.h:40-47 with GTSAM_ROT3_EXPMAP, the
                         reference's default).  Taken by GSX_F_PRIOR, GSX_F_BETWEEN, GSX_F_ATTITUDE and GSX_F_MAG;
                         the g2o / BAL writers, gsx_initialize_pose3, gsx_lago_*, gsx_triangulate_landmarks and
                         smart factors refuse a problem that holds one (GSX_E_INVALID)                      */
  GSX_VAR_UNIT3 = 5,  /* Unit3, a point on the unit sphere: state the unit vector p (3), tangent 2 in the basis
                         B = p.basis() (gtsam/geometry/Unit3.cpp:72-81, 128-138: b1 = normalize(p x axis), the axis
                         that of the smallest |p_i| with the tie order of CalculateBestAxis, b2 = p x b1).  Retract
                         Unit3::retract (:255-282: normalize(cos(theta) p + sin(theta) / theta B v), theta = |B v|,
                         the theta < epsilon branch included), local coordinates Unit3::localCoordinates
                         (:285-303, with the first-order branch at p . q -> 1 and (pi, 0) at the antipode).  Taken
                         by GSX_F_PRIOR (and GSX_F_LINEAR); not a group: GSX_F_BETWEEN refuses it by name.  A
                         state whose norm differs from 1 by more than 1e-9 is refused (gsx_set_values, a prior's
                         measurement; gsx_update for a new variable): nothing is normalised
                         silently.  (gsx_solve_gfg / gsx_solve_gfg_h hand a GSX_F_LINEAR-only handle zeros: no state is read)                                       */
  GSX_VAR_ESSENTIAL = 6 /* EssentialMatrix (gtsam/geometry/EssentialMatrix.h:92-103): state R row-major 9, then
                         the direction t (3, of unit length as above); tangent omega (3), then the direction's 2.
                         Retract (R Expmap(omega), t.retract(v)), local coordinates (Logmap(R1' R2),
                         t1.localCoordinates(t2)).  E = [t]x R is formed where a kernel needs it, never stored.
                         Taken by GSX_F_PRIOR and the GSX_F_ESSENTIAL* factors; GSX_F_BETWEEN refuses it by name.
                         Like GSX_VAR_ROT3, both types are refused by the writers, the initializers, lago and
                         triangulation                                                                      */
};

/* ---- factor types -------------------------------------------------------- */
enum {
  GSX_F_LINEAR = 0,         /* JacobianFactor given directly: meas = [A b] col-major,
                               rows = f_rows[i]; keys: any number                 */
  GSX_F_PRIOR = 1,          /* PriorFactor<T> (gtsam/nonlinear/PriorFactor.h:98-102);
                               meas = prior value in the variable's state layout  */
  GSX_F_BETWEEN = 2,        /* BetweenFactor<T> (gtsam/slam/BetweenFactor.h:111-124);
                               meas = measured T in state layout; T in
                               {VECTOR, POSE2, POSE3, ROT3}.  On ROT3: e =
                               Logmap(z' R1' R2), A1 = -R2' R1, A2 = I — the identity
                               for the Local derivative, as on POSE3               */
  GSX_F_SFM = 3,            /* GeneralSFMFactor<PinholeCamera<Cal3Bundler>,Point3>
                               (gtsam/slam/GeneralSFMFactor.h:141-177); keys
                               (camera, point); meas = (u,v)                       */
  GSX_F_PROJECTION = 4,     /* GenericProjectionFactor<Pose3,Point3,Cal3_S2>
                               (gtsam/slam/ProjectionFactor.h:138-166) with a fixed
                               calibration; keys (POSE3, VECTOR(3)); meas = (u, v,
                               fx, fy, s, u0, v0), or those 7 followed by
                               body_P_sensor as a Pose3 state (R row-major 9, t 3):
                               19 doubles, the if(body_P_sensor_) branch there — the
                               camera sits at pose.compose(body_P_sensor), the pose
                               Jacobian is the camera's times D compose / D pose =
                               AdjointMap(body_P_sensor^-1) (Pose3.cpp:61-75).
                               Cheirality (default flags; z <= 0 in the SENSOR
                               frame): zero Jacobians and the constant error
                               (2 fx, 2 fx); the sensor form counts it in
                               n_cheirality.  The sensor rotation is taken as given */
  GSX_F_BEARINGRANGE = 5,   /* BearingRangeFactor<Pose2,Point2> (gtsam/sam/
                               BearingRangeFactor.h; Pose2::bearing / range,
                               gtsam/geometry/Pose2.cpp:246-285, Rot2.cpp:119-130);
                               keys (POSE2, VECTOR(2)); meas = (bearing angle,
                               range); error = (wrapped bearing difference,
                               range difference)                                   */
  GSX_F_RANGE = 6,          /* RangeFactor<A1,A2> (gtsam/sam/RangeFactor.h); keys
                               (POSE2, VECTOR(2)), (POSE2, POSE2), (POSE3, VECTOR(3))
                               or (POSE3, POSE3); m = 1; meas = (range); error =
                               range(a1, a2) - z.  RangeFactorWithTransform<A1,A2>
                               (RangeFactor.h:104-150): meas = (range) followed by
                               body_T_sensor in the state layout of the first key —
                               13 doubles for POSE3 (R 9, t 3), 4 for POSE2 (x, y,
                               theta); the range is taken from a1.compose(
                               body_T_sensor), the first key's Jacobian is multiplied
                               by AdjointMap(body_T_sensor^-1), the row of ones
                               below included.  Pose2::range (gtsam/geometry/
                               Pose2.cpp:271-310), Pose3::range (Pose3.cpp:408-431).
                               At a distance <= 1e-10 the derivative of the norm is
                               the row of ones norm2 / norm3 hand out there
                               (Point2.cpp:27-36, Point3.cpp:41-50), not a division
                               by zero                                             */
  GSX_F_BEARING = 7,        /* BearingFactor<Pose2,Point2> (gtsam/sam/BearingFactor.h;
                               Pose2::bearing, Pose2.cpp:246-257); keys (POSE2,
                               VECTOR(2)); m = 1; meas = (bearing angle); error = the
                               wrapped bearing difference: the first row of
                               GSX_F_BEARINGRANGE                                  */
  GSX_F_STEREO = 8,         /* GenericStereoFactor<Pose3,Point3> (gtsam/slam/
                               StereoFactor.h:126-154) with a fixed Cal3_S2Stereo;
                               keys (POSE3, VECTOR(3)); m = 3; meas =
                               (uL, uR, v, fx, fy, s, u0, v0, b), or those 9 followed
                               by body_P_sensor as a Pose3 state: 21 doubles, the
                               if(body_P_sensor_) branch there, as GSX_F_PROJECTION.  StereoCamera::
                               project2 (gtsam/geometry/StereoCamera.cpp:37-79): uL =
                               u0 + fx x/z, uR = u0 + fx (x - b)/z, v = v0 + fy y/z —
                               the skew s is carried but, as there, not used.
                               Cheirality (default flags): z <= 0 in the camera frame
                               gives zero Jacobians and the constant error
                               (2 fx, 2 fx, 2 fx); the sensor form counts it in
                               n_cheirality                                        */
  GSX_F_SFM2 = 9,           /* GeneralSFMFactor2<Cal3_S2> (gtsam/slam/
                               GeneralSFMFactor.h:208-278): the calibration is a
                               variable.  Keys (POSE3, VECTOR(3), VECTOR(5)), the
                               last one Cal3_S2 as (fx, fy, s, u0, v0) — it retracts
                               by vector addition (Cal3_S2.h); m = 2; meas = (u, v);
                               error = PinholeCamera<Cal3_S2>(pose, K).project(point)
                               - z with Dpose, Dpoint and Dcal = [x 0 y 1 0; 0 y 0 0 1]
                               (Cal3_S2.cpp:54-62).  Cheirality (:270-277): zero
                               Jacobians and a ZERO error — not the 2 fx of
                               GSX_F_PROJECTION — counted in n_cheirality          */
  GSX_F_SMART_PROJECTION = 10, /* SmartProjectionPoseFactor<Cal3_S2> (gtsam/slam/SmartProjectionPoseFactor.h,
                               SmartProjectionFactor.h, SmartFactorBase.h): one factor per track.  At every
                               linearization it triangulates the landmark from the current poses (triangulateSafe, DLT,
                               no noise model; the LM refinement with enable_epi), marginalizes it and hands the
                               optimizer a factor on the poses alone.  See "Smart projection factors" below.
                               Keys: nk POSE3 variables, 2 <= nk <= 8 — a LIMIT: 8 is the key limit of the assembly
                               (GSX_F_LINEAR's), and the reference returns a zero factor for a single view where this
                               library returns GSX_E_INVALID.  Rows: m = 2 nk - 3, those of the reference's
                               JacobianFactorSVD.  Noise: GSX_NOISE_ISOTROPIC (one sigma) or GSX_NOISE_UNIT only
                               (SmartFactorBase throws "needs isotropic" otherwise); no robust bit.
                               meas = (fx, fy, s, u0, v0,
                                       rank_tol, enable_epi, landmark_distance_threshold,
                                       dynamic_outlier_rejection_threshold   [SmartProjectionParams::triangulation],
                                       retriangulation_threshold, degeneracy_mode),
                               optionally body_P_sensor as a Pose3 state (12 doubles; told by the length, as with
                               GSX_F_PROJECTION), then 2 nk pixel coordinates in key order.
                               degeneracy_mode: only ZERO_ON_DEGENERACY (1) is taken; IGNORE_DEGENERACY (0) and
                               HANDLE_INFINITY (2) go through backprojectPointAtInfinity and a Unit3 tangent basis and
                               return GSX_E_INVALID — the reference's SmartProjectionRigFactor makes the same restriction.
                               No linearization mode is offered: HESSIAN and JACOBIAN_SVD give the same normal equations
                               at lambda = 0, which is what NonlinearFactorGraph::linearize passes                   */
  GSX_F_TRANSLATION = 11,   /* TranslationFactor (gtsam/sfm/TranslationFactor.h:41-78); keys (VECTOR(3), VECTOR(3)) =
                               (Ta, Tb); m = 3; meas = the 3 doubles of w_aZb.point3(), taken as given (the ABI does not
                               renormalise; the Python Unit3 normalises as the reference's constructor does).  Error =
                               normalize(Tb - Ta) - z; H2 = the 3 x 3 derivative of normalize (gtsam/geometry/
                               Point3.cpp:52-62), H1 = -H2.  Ta == Tb divides by zero exactly as the reference does: no
                               special case — the non-finite block surfaces through the handle's existing non-finite
                               reporting (a failed factorization / GSX_E_INDETERMINATE, a non-finite error)            */
  GSX_F_BILINEAR_TRANSLATION = 12, /* BilinearAngleTranslationFactor (TranslationFactor.h:104-149), BATA; keys (VECTOR(3),
                               VECTOR(3), VECTOR(1)) = (Ta, Tb, scale); m = 3; meas = the same 3 doubles.  Error =
                               |s| (Tb - Ta) - z; H1 = -|s| I, H2 = |s| I, H3 = (Tb - Ta) for s >= 0 — s == 0 takes this
                               branch — else (Ta - Tb)                                                                 */
  /* ---- absolute-measurement factors: one key (GPSFactorArmCalib: two), told apart by key type and length ---- */
  GSX_F_GPS = 13,           /* GPSFactor (gtsam/navigation/GPSFactor.cpp:40-43): key (POSE3); m = 3; meas = nT (3); e =
                               t - nT, H = [0 R].  GPSFactorArm (:85-96): meas = nT (3), bL (3) — told by the length; e =
                               t + R bL - nT, H = [-R [bL]x, R].  GPSFactorArmCalib (:113-128): keys (POSE3, VECTOR(3)),
                               the lever arm a variable; meas = nT (3); H2 = R                                          */
  GSX_F_POSE_TRANSLATION_PRIOR = 14, /* PoseTranslationPrior<POSE> (gtsam/slam/PoseTranslationPrior.h:65-77): key (POSE2),
                               m = 2, meas = (x, y), or (POSE3), m = 3, meas = t (3); e = t - z, H = R in the translation
                               columns, zero elsewhere                                                                  */
  GSX_F_POSE_ROTATION_PRIOR = 15, /* PoseRotationPrior<POSE> (gtsam/slam/PoseRotationPrior.h:81-90): key (POSE2), m = 1,
                               meas = (theta): e = Rot2 local coordinates of (z, R), an angle in (-pi, pi]; or (POSE3),
                               m = 3, meas = R row-major (9): e = Logmap(z' R).  H is the IDENTITY in the rotation
                               columns, as written there — not the derivative of Logmap                                */
  GSX_F_ATTITUDE = 16,      /* Rot3AttitudeFactor / Pose3AttitudeFactor (gtsam/navigation/AttitudeFactor.cpp:26-40,
                               AttitudeFactor.h:136, 212): key (ROT3) or (POSE3); m = 2; meas = nRef (3), bMeasured (3),
                               both of unit length to 1e-9 (GSX_E_INVALID otherwise).  e = B' q with q = normalize(R
                               bMeasured) and B = nRef.basis() (gtsam/geometry/Unit3.cpp:72-141, 199-206), computed by
                               the library once per factor; H = B' (I - q q') (-R [bMeasured]x) in the rotation columns,
                               which is the reference's B' B_q B_q' (-R [b]x) for any basis B_q of q; the translation
                               columns of the POSE3 form are zero                                                       */
  GSX_F_MAG = 17,           /* MagFactor1 (gtsam/navigation/MagFactor.h:121-125): key (ROT3), m = 3; MagPoseFactor<POSE>
                               (MagPoseFactor.h:74-132): key (POSE3), m = 3, or (POSE2), m = 2.  meas = z, nM, bias, m
                               doubles each, PREPARED: nM = scale * direction.normalized(), z and bias rotated by
                               body_P_sensor where there is one (the constructors do that; the Python classes too).
                               e = R' nM + bias - z; H = [R' nM]x in the rotation columns (Rot3::unrotate), on POSE2
                               (q_y, -q_x) in the theta column (Rot2::unrotate)                                         */
  /* ---- two-view geometry (gtsam/slam/EssentialMatrixFactor.h, EssentialMatrixConstraint.cpp).  NOT lowered:
     EssentialMatrixFactor5 (its same-key use lists one variable twice), the Cal3Bundler and Cal3f instantiations of
     EssentialMatrixFactor4, EssentialTransferFactor, and the Pose3 bearing factors on a Unit3 measurement ---- */
  GSX_F_ESSENTIAL = 18,     /* EssentialMatrixFactor (:34-106): key (ESSENTIAL); m = 1; meas = vA (3), vB (3), the
                               homogeneous vectors the factor stores.  e = vA' E vB; H = [vA' E [-vB]x, vA' [-R vB]x B]
                               with B the direction's basis (EssentialMatrix::error, EssentialMatrix.cpp:104-114)       */
  GSX_F_ESSENTIAL_DEPTH = 19, /* EssentialMatrixFactor2 (:112-229): keys (ESSENTIAL, VECTOR(1) inverse depth d); m = 2;
                               meas = dP1 (3), pn (2), f (1).  dP2 = R' (dP1 - d t), e = f (Project(dP2) - pn): d = 0 is
                               the pure homography, dP2.z <= 0 is projected all the same (PinholeBase::Project has no
                               cheirality check).  With cRb (9, row-major) appended — 15 doubles — it is
                               EssentialMatrixFactor3 (:237-317): E is first rotated into the camera frame
                               (EssentialMatrix::rotate, EssentialMatrix.cpp:73-101), DE multiplied by its 5 x 5 block
                               [cRb 0; 0 Bq' cRb B], Bq the basis of the ROTATED direction (Rot3::rotate(Unit3))         */
  GSX_F_ESSENTIAL_CALIB = 20, /* EssentialMatrixFactor4<Cal3_S2> (:334-419): keys (ESSENTIAL, VECTOR(5)), the calibration
                               (fx, fy, s, u0, v0) as for GSX_F_SFM2; m = 1; meas = pA (2), pB (2) in pixels.  e = vA' E vB
                               with v = (Cal3_S2::calibrate(p), 1) (gtsam/geometry/Cal3_S2.cpp:53-69, its calibration
                               Jacobian in HK)                                                                          */
  GSX_F_ESSENTIAL_CONSTRAINT = 21 /* EssentialMatrixConstraint (EssentialMatrixConstraint.cpp:45-77): keys (POSE3, POSE3);
                               m = 5; meas = the measured E as R (9) and its direction (3, of unit length to 1e-9).
                               e = measured.localCoordinates(FromPose3(p1.between(p2))) (EssentialMatrix.cpp:27-45,
                               Unit3.cpp:44-52); the Jacobians are D_hx_1P2 D_between only — the local-coordinates map
                               contributes none, as in the reference.  A zero relative translation gives a non-finite
                               error there and here: it does not trap and surfaces as any other non-finite error does
                               (a failed factorization / GSX_E_INDETERMINATE, a non-finite gsx_error)                   */
};

/* ---- noise model kinds (gtsam/linear/NoiseModel.cpp) --------------------- */
enum {
  GSX_NOISE_UNIT = 0,       /* no parameters                                     */
  GSX_NOISE_ISOTROPIC = 1,  /* 1 parameter: sigma                                */
  GSX_NOISE_DIAGONAL = 2,   /* m parameters: sigmas.  A sigma of exactly 0 makes
                               the row a HARD CONSTRAINT — noiseModel::Constrained::
                               MixedSigmas(sigmas), mu = 1000 (NoiseModel.h:389-500) */
  GSX_NOISE_GAUSSIAN = 3,   /* m*m parameters: upper-triangular sqrt information R,
                               row-major (whitened = R * unwhitened)             */
  GSX_NOISE_CONSTRAINED = 4,/* 2m parameters: sigmas (0 = hard constraint), then the
                               weights mu the violated constraint rows get in the
                               error functions — Constrained::MixedSigmas(mu, sigmas)
                               (NoiseModel.cpp:371-381,438-444).  See "Hard
                               constraints" below.                                */
  /* noiseModel::Robust (gtsam/linear/NoiseModel.cpp:709-735, LossFunctions.cpp): OR one of these onto the base
   * kind above and append ONE parameter (k / c) after the base model's parameters.  Linearization whitens with
   * the base model and then scales [A b] by sqrt(weight(|b|)) (Block reweighting); the factor's error is
   * loss(|whitened e|) instead of |e|^2 / 2. */
  GSX_NOISE_ROBUST_HUBER = 1 << 4,   /* mEstimator::Huber  :179-191 */
  GSX_NOISE_ROBUST_TUKEY = 2 << 4,   /* mEstimator::Tukey  :250-267 */
  GSX_NOISE_ROBUST_CAUCHY = 3 << 4,  /* mEstimator::Cauchy :217-224 */
  GSX_NOISE_BASE_MASK = 15
};

/* ---- Hard constraints ------------------------------------------------------
 * A row of sigma 0 (GSX_NOISE_DIAGONAL / GSX_NOISE_CONSTRAINED) is a hard constraint: the linear step satisfies
 * A_row delta = b_row exactly.  The reference eliminates a clique that holds such a row with EliminateQR and
 * Constrained::QR instead of Cholesky (gtsam/linear/HessianFactor.cpp:538-551, JacobianFactor.cpp:804-842,
 * NoiseModel.cpp:503-620); this library turns the row into a pivot of its clique before the clique's Cholesky
 * (csrc/constraint.hip) — the same step delta, the same LM trace.  What a caller sees:
 *   - gsx_error / gsx_linear_error weigh a violated constraint row by mu, as Constrained::squaredMahalanobisDistance does
 *     (NoiseModel.cpp:438-444; mu = 1000 for GSX_NOISE_DIAGONAL);
 *   - gsx_get_jacobians returns a constraint row scaled by sqrt(mu) (the reference keeps it unwhitened and applies mu in
 *     its error functions); gsx_hessian_diagonal counts it unwhitened, as JacobianFactor::hessianDiagonalAdd does;
 *   - gsx_stats.n_constraint_rows / n_constrained_fronts; a clique that takes constraint rows in is always a blocked front;
 *   - gsx_get_conditional of a clique with constraint pivots gives an EQUIVALENT conditional (a pivot row has unit
 *     diagonal and comes first in its clique's elimination), not the reference's row for row;
 *   - NOT available on such a problem: marginal covariances and Dogleg (GSX_E_STATE), sharding (gsx_set_ordering fails);
 *   - a clique that takes in more constraint rows than it has frontal scalars hands the others on, each with the
 *     variables it still holds, to the clique where the first of them is frontal; rows of one clique with DIFFERENT
 *     supports (excess rows on (a, x) and on (b, y) of a clique {a, b}) are handed on too, each until it reaches its
 *     own first variable.  How many rows a clique may hand on is planned from the variables the factors hold, assuming
 *     that r rows holding a variable of d scalars give min(r, d) pivots;
 *   - what is refused: a constraint row that leaves FEWER pivots than that plan — its entries in its clique's frontal
 *     variables all vanish NUMERICALLY although its factor holds them, or rows that are dependent within a variable's
 *     columns (a rank-deficient constraint Jacobian) — and still says something about the separator is reported as
 *     GSX_E_INDETERMINATE by the solve; the reference passes such a row on to the parent clique.  A row that reduces
 *     to 0 = d (redundant or inconsistent, nothing left in any column) is dropped, as the reference drops it. */

/* ---- ordering kinds for gsx_compute_ordering ----------------------------- */
enum {
  GSX_ORDER_NATURAL = 0,    /* ascending key                                      */
  GSX_ORDER_MINDEGREE = 1,  /* own approximate-minimum-degree (host)              */
  GSX_ORDER_ND = 2,         /* own nested dissection (BFS level-set separators)   */
  GSX_ORDER_SCHUR = 3,      /* VECTOR(3) landmarks first, then the rest by
                               minimum degree on the reduced graph                */
  GSX_ORDER_SCHUR_ND = 4    /* landmarks first, the rest by nested dissection of
                               the reduced graph (shallow tree; METIS analogue)   */
};

/*
 * Immutable problem structure.  Variables are listed in ASCENDING KEY ORDER
 * (the iteration order of gtsam::Values); everything else refers to variables
 * by their index in this list.  Factors are listed in graph order.
 */
typedef struct gsx_problem_desc {
  int32_t n_vars;
  const uint64_t* var_keys;   /* [n_vars] strictly ascending                     */
  const int32_t* var_types;   /* [n_vars] GSX_VAR_*                              */
  const int32_t* var_dims;    /* [n_vars] tangent dim (checked for typed vars)   */

  int32_t n_factors;
  const int32_t* f_type;      /* [n_factors] GSX_F_*                             */
  const int32_t* f_rows;      /* [n_factors] residual dim m                      */
  const int32_t* f_key_ptr;   /* [n_factors+1] CSR into f_vars                   */
  const int32_t* f_vars;      /* variable indices                                */
  const int64_t* f_meas_ptr;  /* [n_factors+1] CSR into meas                     */
  const double* meas;
  const int32_t* f_noise_kind;/* [n_factors] GSX_NOISE_*                         */
  const int64_t* f_noise_ptr; /* [n_factors+1] CSR into noise                    */
  const double* noise;
} gsx_problem_desc;

/* LevenbergMarquardtParams (gtsam/nonlinear/LevenbergMarquardtParams.h:61-98) +
 * NonlinearOptimizerParams (gtsam/nonlinear/NonlinearOptimizerParams.h:42-108). */
typedef struct gsx_lm_params {
  int32_t max_iterations;        /* 100 (legacy) / 50 (ceres)                  */
  double relative_error_tol;     /* 1e-5 / 1e-6                                */
  double absolute_error_tol;     /* 1e-5 / 0                                   */
  double error_tol;              /* 0                                          */
  double lambda_initial;         /* 1e-5 / 1e-4                                */
  double lambda_factor;          /* 10 / 2                                     */
  double lambda_upper_bound;     /* 1e5 / 1e32                                 */
  double lambda_lower_bound;     /* 0 / 1e-16                                  */
  double min_model_fidelity;     /* 1e-3                                       */
  int32_t diagonal_damping;      /* 0 / 1                                      */
  int32_t use_fixed_lambda_factor; /* 1 / 0                                    */
  double min_diagonal;           /* 1e-6                                       */
  double max_diagonal;           /* 1e32                                       */
  int32_t verbosity;             /* 0 silent, 1 SUMMARY lines to stdout        */
} gsx_lm_params;

/* Result + per-inner-iteration trace (the CSV the reference's logFile holds:
 * LevenbergMarquardtOptimizer.cpp:104-118). */
typedef struct gsx_lm_result {
  double initial_error;
  double final_error;
  double final_lambda;
  int32_t iterations;            /* outer (accepted) iterations                */
  int32_t inner_iterations;      /* tryLambda calls                            */
  int32_t n_solve_failures;      /* indeterminate systems met on the way       */
  int32_t trace_len;             /* entries written to the trace arrays        */
  /* caller-owned, each [trace_cap] or NULL */
  int32_t trace_cap;
  double* trace_error;           /* error after the inner iteration            */
  double* trace_lambda;          /* lambda tried                               */
  int32_t* trace_accepted;       /* 1 accepted, 0 rejected, -1 solve failed    */
  int32_t pcg_iterations;        /* PCG iterations of all solves of the run; written ONLY by a handle whose linear
                                    solver is GSX_SOLVER_PCG (callers built before the field existed never set one) */
} gsx_lm_result;

/* Symbolic-analysis and timing counters (gsx_get_stats). */
typedef struct gsx_stats {
  int64_t n_fronts;              /* Bayes-tree cliques                         */
  int64_t n_levels;              /* height of the assembly tree                */
  int64_t max_front_dim;         /* max frontal scalar dim                     */
  int64_t max_front_rows;        /* max frontal + separator scalar dim         */
  int64_t n_small_fronts;        /* fronts eliminated in LDS                   */
  int64_t n_big_fronts;          /* fronts eliminated by the blocked path      */
  double factor_flops;           /* sum f^3/3 + f^2 (s+1) + f (s+1)^2          */
  double front_bytes;            /* sum 8 (f+s+1)^2                            */
  double lpanel_bytes;           /* sum 8 f (f+s+1)  (back-substitution reads) */
  double jacobian_bytes;         /* bytes of all [A b] blocks                  */
  double hessian_bytes;          /* bytes of the block-sparse H panels         */
  double total_dim;              /* scalar dimension of the system             */
  /* accumulated device times (ms, HIP events on the handle's stream) and call
   * counts since the last gsx_reset_stats, named like the reference's gttic
   * labels (gtsam/base/timing.h) */
  double ms_linearize, ms_assemble_hessian, ms_factorize, ms_backsolve,
      ms_linear_error, ms_retract, ms_error;
  int64_t n_linearize, n_factorize, n_backsolve, n_error;
  int64_t n_cheirality;          /* SFM / SFM2 / sensor-form factors in their cheirality branch in the last linearize */
  double amalgamation_relax;     /* the amalgamation in effect (the library's choice under GSX_AMALGAMATION_AUTO) */
  int64_t amalgamation_max_frontal_dim;
  int64_t n_medium_fronts;       /* of the LDS fronts: frontal panel in LDS, trailing block in HBM */
  int64_t n_tree_fronts;         /* fronts eliminated dependency-driven, one launch per tier, instead of level by level */
  int64_t n_upper_levels;        /* launch rounds of the fronts that are neither: levelled among themselves (longest chain) */
  int64_t n_constraint_rows;     /* hard-constraint (zero-sigma) rows of the graph */
  int64_t n_constrained_fronts;  /* fronts that take constraint rows in (always blocked; constraint pivots before Cholesky) */
  int64_t n_pcg_iterations;      /* PCG iterations since the last gsx_reset_stats (gsx_solve_pcg and the drivers of a PCG handle) */
  int64_t n_pcg_solves;          /* ... and the solves they belong to */
  int64_t n_smart_invalid;       /* smart factors whose last linearize found no valid point (an all-zero block) */
  int64_t n_smart_retriangulated;/* smart factors the last linearize or error evaluation actually re-triangulated */
} gsx_stats;

/* ---- on-disk formats (host only) -------------------------
 * Native readers of the files the reference's drivers start from, lowered to a
 * gsx_problem_desc + packed initial Values owned by an opaque gsx_dataset.
 *   gsx_read_g2o   readG2o / parse3DFactors: gtsam/slam/dataset.cpp:216-296,505-633
 *                  (2-D), :756-863 (3-D, information permuted from (t,R) to (R,t));
 *                  noise = Gaussian::Information (gtsam/linear/NoiseModel.cpp:98-112);
 *                  + the anchoring prior of examples/Pose2SLAMExample_g2o.cpp:65-67 /
 *                  Pose3SLAMExample_g2o.cpp:42-48, appended last
 *   gsx_read_bal   SfmData::FromBalFile gtsam/sfm/SfmData.cpp:189-245 + openGL2gtsam
 *                  :79-85; graph of examples/SFMExample_bal.cpp:55-68 (add_priors != 0
 *                  appends its two priors)
 *                  3-D also takes TORO's VERTEX3 / EDGE3 (roll pitch yaw, information as written: :741-764,
 *                  :829-840); poses of a 3-D file that have no VERTEX line are chained from the successive odometry
 *                  edges starting at the origin, as the reference's MATLAB loader does for such files
 *                  (matlab/+gtsam/load3D.m:21-53; examples/Data/sphere2500.txt)
 *   gsx_load2d     load2D gtsam/slam/dataset.cpp:505-570: TORO / "graph" 2-D files — VERTEX2|VERTEX_SE2|VERTEX,
 *                  VERTEX_XY landmarks (keys L(j)), EDGE2|EDGE|EDGE_SE2|ODOMETRY between factors, BR / LANDMARK
 *                  bearing-range factors (:452-496); undeclared variables are created from the odometry / the first
 *                  sighting (:540-563); no prior is added.  noise_format as enum NoiseFormat (dataset.h:65-71, AUTO
 *                  guesses GRAPH or COV, :219-231); smart != 0 lets a diagonal matrix become a Diagonal / Isotropic /
 *                  Unit model (NoiseModel.cpp:98-131); kernel 0/1/2 = none / Huber(1.345) / Tukey(4.6851) (:276-292);
 *                  model_sigmas (3 doubles or NULL) replaces the models of the file (:348-349); max_index as there
 *                  (0 = all).  The sampler (addNoise) is not offered.
 * The pointers handed out by gsx_dataset_get stay valid until gsx_dataset_free. */
enum { GSX_NOISE_FORMAT_G2O = 0, GSX_NOISE_FORMAT_TORO = 1, GSX_NOISE_FORMAT_GRAPH = 2, GSX_NOISE_FORMAT_COV = 3,
       GSX_NOISE_FORMAT_AUTO = 4 };
typedef struct gsx_dataset gsx_dataset;
gsx_status gsx_read_g2o(const char* path, int32_t is3d, gsx_dataset** out);
gsx_status gsx_load2d(const char* path, const double* model_sigmas, int64_t max_index, int32_t smart,
                      int32_t noise_format, int32_t kernel, gsx_dataset** out);
gsx_status gsx_read_bal(const char* path, int32_t add_priors, gsx_dataset** out);
gsx_status gsx_dataset_get(const gsx_dataset* d, gsx_problem_desc* desc, const double** values, int64_t* n_values);
void gsx_dataset_free(gsx_dataset* d);
/* writeG2o (gtsam/slam/dataset.cpp:636-735): the Pose2 / Pose3 variables and the between factors of a problem with the
 * given packed Values, in g2o format (17 significant digits). */
gsx_status gsx_write_g2o(const gsx_problem_desc* desc, const double* values, int64_t n_values, const char* path);
/* save2D (gtsam/slam/dataset.cpp:587-617): VERTEX2 lines for the Pose2 values; for every BetweenFactor<Pose2> an EDGE2
 * line with the keys swapped and the measurement inverted, carrying the information of the ONE Diagonal model handed in
 * (3 sigmas) in TORO order — as the reference, which ignores the factors' own models there. */
gsx_status gsx_save2d(const gsx_problem_desc* desc, const double* values, int64_t n_values, const double* model_sigmas,
                      const char* path);
/* writeBAL / writeBALfromValues (gtsam/sfm/SfmData.cpp:249-377): cameras and points of `values`, the observations of the
 * GSX_F_SFM factors grouped by point; poses back in the OpenGL convention (gtsam2openGL :88-99), rotations as Rodrigues
 * vectors, measurements (u, -v); 17 significant digits. */
gsx_status gsx_write_bal(const gsx_problem_desc* desc, const double* values, int64_t n_values, const char* path);

/* ---- lifecycle ------------------------------------------------------------ */
gsx_status gsx_create(const gsx_problem_desc* desc, int32_t device, gsx_handle* out);
gsx_status gsx_destroy(gsx_handle h);
const char* gsx_last_error(gsx_handle h);          /* human-readable, may be "".  h == NULL: the line of the
                                                      calling thread's last call that HAS no handle — a refused
                                                      gsx_create, and every call that takes a description without
                                                      one (the g2o / BAL / save2d writers, gsx_pose3_* and
                                                      gsx_initialize_pose3, gsx_lago_*, gsx_triangulation_tracks,
                                                      gsx_triangulate_landmarks).  Each of them clears the line on
                                                      entry, so "" after one that went through or that failed
                                                      without a line; the pointer is valid until the thread's next
                                                      such call */
const char* gsx_version(void);
int32_t gsx_device_count(void);                    /* 0 when no GPU is visible  */

/* ---- ordering / symbolic analysis (host only; works without a GPU) -------- */
gsx_status gsx_set_ordering(gsx_handle h, const uint64_t* keys, int32_t n);
gsx_status gsx_compute_ordering(gsx_handle h, int32_t kind, uint64_t* keys_out);
/* Relaxed clique amalgamation, applied by the NEXT gsx_set_ordering.  relax = 0 builds exactly the
 * reference's Bayes tree: a child cluster is merged into its parent only when that adds no structural zero
 * (gtsam/inference/JunctionTree-inst.h:120-149).  relax > 0 also merges a child when the explicit zeros padded
 * into its columns are at most relax x its own conditional's size and the merged frontal dimension stays
 * <= max_frontal_dim: fewer, larger cliques, i.e. fewer levels and kernel launches on the latency-bound chains of
 * the elimination tree.  The solution is unchanged (zeros are factored as zeros); only gsx_get_tree differs.
 * relax = GSX_AMALGAMATION_AUTO (the default of a new handle; max_frontal_dim ignored): the symbolic analysis picks
 * (relax, max_frontal_dim) itself from a cost model of the level schedule — levels, pivot chains, padded flops —
 * and reports its choice in gsx_stats.  Every reference clique still survives whole inside one of the library's. */
#define GSX_AMALGAMATION_AUTO (-1.0)
gsx_status gsx_set_amalgamation(gsx_handle h, double relax, int32_t max_frontal_dim);
/* ---- one problem over the GPUs of a node -------------------------------------------------------
 * The reference has no distributed solver; the seam is the same as everywhere else in this header — the handle
 * stands in for NonlinearOptimizer::solve()/iterate() — and the partition is the multifrontal one: subtrees of the
 * Bayes tree are independent until their Schur complements meet in a common ancestor
 * (gtsam/inference/ClusterTree-inst.h:256-265), and the solve hands only x_S down
 * (gtsam/linear/linearAlgorithms-inst.h:60-62).
 *
 * One process per GPU; every rank creates its handle from the SAME problem, values and ordering and calls
 * gsx_set_shard before gsx_set_ordering.  The next gsx_set_ordering then splits the tree into a CAP (the top fronts,
 * whose subtrees are too heavy to give to one rank) and the forest below it, dealt to the ranks by cost.  A rank
 * linearizes the factors of its subtrees, assembles and eliminates their fronts, and adds its share into the cap
 * fronts; ONE sum all-reduce of the cap's contiguous arena block per factorization completes them, after which every
 * rank factors and back-substitutes the cap alike (identical bits in, identical bits out) and solves its own
 * subtrees.  Errors and status counters are summed the same way before the host reads them, so the LM policy takes
 * the same decisions on every rank.  A rank keeps only its own variables (and the cap's) up to date between
 * iterations; gsx_get_values and gsx_solve(delta_out) complete the vector with one more all-reduce.
 *
 * allreduce(user, device_buffer, count): in-place SUM of `count` doubles of device memory over all ranks, complete
 * (device-visible) when it returns; non-zero return = failure.  The library synchronizes its own stream before the
 * call.  With torch.distributed this is dist.all_reduce on a tensor aliasing the pointer (backend "nccl" = RCCL over
 * xGMI); a C++ host would call ncclAllReduce.  In a sharded handle EVERY entry point is collective: all ranks call it
 * in the same order.  gsx_dogleg_optimize and gsx_marginal_covariance are not available on a sharded handle
 * (GSX_E_STATE).  world = 1 (the default) is the single-GPU path, bit for bit. */
typedef int32_t (*gsx_allreduce_fn)(void* user, double* device_buffer, int64_t count);
gsx_status gsx_set_shard(gsx_handle h, int32_t rank, int32_t world, gsx_allreduce_fn allreduce, void* user);
typedef struct gsx_shard_info {
  int32_t rank, world;
  int32_t n_cap_fronts;          /* fronts of the cap (processed by every rank)            */
  int32_t n_own_fronts;          /* fronts of this rank's subtrees                         */
  int32_t cap_level0;            /* first level of the cap in the schedule, -1: no cap     */
  int32_t n_own_factors;         /* factors this rank linearizes                           */
  int64_t cap_doubles;           /* size of the per-factorization all-reduce               */
  double cap_flops, own_flops, total_flops;  /* elimination flop estimates: cap, own subtrees, whole tree */
} gsx_shard_info;
/* partition of the current ordering: front_owner[n_fronts] = owning rank or -1 (cap), factor_owned[n_factors] = 1
 * when this rank linearizes the factor; either array may be NULL */
gsx_status gsx_get_shard(gsx_handle h, gsx_shard_info* info, int32_t* front_owner, int32_t* factor_owned);
/* A device buffer the library allocated itself (hipMalloc) that holds nothing between calls: what a host probes its
 * all-reduce on before trusting it with the cap (the hazard is a collective library reducing IN PLACE on memory it did
 * not allocate; gtsam_petercdev_amd/distributed.py: checked_allreduce).  *count doubles at *device_ptr; the host may
 * overwrite them freely between gsx calls. */
gsx_status gsx_scratch_buffer(gsx_handle h, double** device_ptr, int64_t* count);
/* how each front of the current tree is eliminated: bits 0-1 = 0 leaf kernel (panel only), 1 whole front in LDS,
 * 2 blocked path in HBM, 3 medium (frontal panel in LDS, trailing block in HBM); bit 2 = tree front (dependency-driven
 * launch); bit 3 = lean leaf (no Schur complement stored: its blocked parent's gather forms it) */
gsx_status gsx_get_front_classes(gsx_handle h, int32_t* classes);
/* The extend-add plan of the current tree, read-only (host side; answers on a handle without a device): how the
 * contributions of the children reach the blocked fronts.  A segment is one wave's work: up to 64 consecutive sources
 * of one destination block.  Pass NULL arrays to query the counts, then fill:
 *   segments[11 * i ..]  group (the upper level whose launch runs it, -1: the side group of lean leaves), task (one per
 *                        destination block and group), destination front, variable of the block's rows (-1: the
 *                        right-hand side), variable of its columns (indices as in gsx_get_tree), rows dB, columns dA,
 *                        1 for a diagonal block, scratch slot (-1: the sum is added straight into the front), first
 *                        source, one past the last source
 *   sources[2 * s ..]    child front, and F > 0 for a lean leaf (the product form of its n x F panel) or 0 for a stored
 *                        Schur-complement block
 *   combines[4 * m ..]   group, task, first scratch slot, number of slots: the tasks of more than one segment, whose
 *                        partial sums the combine pass adds in slot order */
gsx_status gsx_get_gather_plan(gsx_handle h, int32_t* n_segments, int64_t* n_sources, int32_t* n_combines,
                               int64_t* segments, int32_t* sources, int32_t* combines);
/* Which kernel assembles the H panel (J'J, J'b) of every variable of the current tree, read-only and host side (answers
 * on a handle without a device, and never touches one).  Arrays of n_vars entries indexed as in gsx_get_tree; any may be
 * NULL:
 *   classes[v]      GSX_H_TILE   2..64 terms, every factor at most 8 rows and 16 columns with the rhs: one matrix-core
 *                                product per factor, a wave per panel, four panels a workgroup
 *                   GSX_H_LIGHT  panel of at most 6144 doubles, fewer than 96 terms: one wave, one LDS copy
 *                   GSX_H_HEAVY  panel of at most 1536 doubles, 96 terms or more: four waves, an LDS copy each, summed
 *                                in wave order
 *                   GSX_H_HUGE   panel above 6144 doubles: one wave straight into global memory
 *                   GSX_H_STAR   dimension at most 7, every factor binary (three terms) with a later-eliminated partner
 *                                of its own, all factors of one shape
 *                   GSX_H_DIAG   no later neighbour, dimension at most 15, 64 terms (32 factors) or more: matrix cores,
 *                                four waves
 *                   -1           the variable belongs to another rank's subtree (gsx_set_shard)
 *                   (a term = one block product of one factor: own block, one per later neighbour in the factor, rhs)
 *   group[v]        index of the variable's launch group (panels of like size share a launch), -1 with class -1
 *   position[v]     its place in the group's variable list
 *   bundle[v], bundle_size[v]   a star variable: the bundle (one wave) it shares with up to four neighbours of its
 *                   shape, and how many variables the bundle holds; -1 and 0 when the star group runs unbundled (one
 *                   variable has more than 64 factors) and for every other class
 *   *fused_diag_star   1 when the star bundles and the diag group run in one launch.  A handle that eliminates star
 *                   leaves straight from [A b] (the default when the tree has some; not a handle created under
 *                   GSX_FUSED_STAR=0 — like every schedule switch it is read by gsx_create and kept for the handle's
 *                   life — and not a handle without a device) launches the two apart: 0. */
enum { GSX_H_TILE = 0, GSX_H_LIGHT = 1, GSX_H_HEAVY = 2, GSX_H_HUGE = 3, GSX_H_STAR = 4, GSX_H_DIAG = 5 };
gsx_status gsx_get_hessian_groups(gsx_handle h, int32_t* classes, int32_t* group, int32_t* position, int32_t* bundle,
                                  int32_t* bundle_size, int32_t* fused_diag_star);
/* The H panel of variable `key` as the device assembled it from the current [A b] blocks: *rows x *dim doubles,
 * column-major (entry (i, j) at out[i + j * *rows]); rows = the variable's own scalars, then those of its
 * later-eliminated neighbours in elimination order, then the right-hand side; entry (i, j) = sum over the variable's
 * factors of column i of the row's block times column j of the variable's block (the last row: b' A).  row_var[i],
 * row_scalar[i] name the variable (index as in gsx_get_tree; -1: the right-hand side) and the scalar of row i; both may
 * be NULL.  out = NULL queries *rows and *dim only (host side).  Like gsx_hessian_diagonal the call assembles stale
 * panels first, those of the star leaves included, which the factorization otherwise forms in registers and never
 * stores.  GSX_E_STATE before gsx_linearize and for a variable of another rank's subtree; on a sharded handle a cap
 * variable's panel holds this rank's terms only. */
gsx_status gsx_get_hessian_panel(gsx_handle h, uint64_t key, int32_t* rows, int32_t* dim, double* out, int32_t* row_var,
                                 int32_t* row_scalar);
gsx_status gsx_get_ordering(gsx_handle h, uint64_t* keys_out);
/* Bayes-tree structure for parity checks: per front the frontal / separator
 * variable indices (CSR) and the parent front (-1 = root).  Pass NULL arrays to
 * query sizes (*n_fronts, *n_sep_total = length of sep_vars). */
gsx_status gsx_get_tree(gsx_handle h, int32_t* n_fronts, int64_t* n_sep_total, int32_t* parent,
                        int32_t* frontal_ptr, int32_t* frontal_vars,
                        int32_t* sep_ptr, int32_t* sep_vars);

/* ---- state ----------------------------------------------------------------- */
int64_t gsx_state_size(gsx_handle h);              /* doubles in packed Values  */
int64_t gsx_tangent_size(gsx_handle h);            /* doubles in packed delta   */
int64_t gsx_jacobian_size(gsx_handle h);           /* doubles in all [A b]      */
gsx_status gsx_set_values(gsx_handle h, const double* packed, int64_t n);
gsx_status gsx_get_values(gsx_handle h, double* packed, int64_t n);

/* ---- the hot path, step by step -------------------------------------------- */
gsx_status gsx_error(gsx_handle h, double* out);
gsx_status gsx_linearize(gsx_handle h);
/* [A b] of every factor, graph order, each dense column-major m x (sum d + 1) */
gsx_status gsx_get_jacobians(gsx_handle h, double* out, int64_t n);
gsx_status gsx_hessian_diagonal(gsx_handle h, double* out, int64_t n);
/* Damped solve (J'J + lambda D) delta = J'b with D = I or clamp(diag J'J).
 * delta_out may be NULL (delta stays on the device for gsx_retract).
 * On GSX_E_INDETERMINATE *bad_key holds a frontal key of a failing clique. */
gsx_status gsx_solve(gsx_handle h, double lambda, int32_t diagonal_damping,
                     double min_diagonal, double max_diagonal, double* delta_out,
                     int64_t n, uint64_t* bad_key);
/* 0.5 * sum |A_i delta - b_i|^2 on the UNDAMPED linear graph, at 0 and at the
 * delta of the last gsx_solve. */
gsx_status gsx_linear_error(gsx_handle h, double* err_at_zero, double* err_at_delta);
/* trial = values (+) delta (device delta of the last solve when delta==NULL);
 * *trial_error (may be NULL) = graph error at trial; commit != 0 makes trial
 * the current values. */
gsx_status gsx_retract(gsx_handle h, const double* delta, int64_t n, int32_t commit,
                       double* trial_error);

/* ---- optimizers ------------------------------------------------------------- */
void gsx_lm_params_legacy(gsx_lm_params* p);       /* SetLegacyDefaults          */
void gsx_lm_params_ceres(gsx_lm_params* p);        /* SetCeresDefaults           */
gsx_status gsx_lm_optimize(gsx_handle h, const gsx_lm_params* p, gsx_lm_result* r);
/* one outer iteration (LevenbergMarquardtOptimizer::iterate); the LM state
 * (lambda, factor, error) lives in the handle; reset by gsx_lm_reset. */
gsx_status gsx_lm_reset(gsx_handle h, const gsx_lm_params* p);
gsx_status gsx_lm_iterate(gsx_handle h, const gsx_lm_params* p, double* error,
                          double* lambda);
/* The trust policy alone, as a pure host function (csrc/lm_policy.cpp; usable without a GPU): what one damped trial means
 * for the controller.  Inputs: whether the damped system could be factored, the quadratic model's cost at zero and at the
 * step (undamped linearized graph), the true cost at the retracted point.  `state` is updated in place.  Decision-equivalent
 * to LevenbergMarquardtOptimizer::tryLambda (gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-270) +
 * LevenbergMarquardtState::increaseLambda / decreaseLambda (gtsam/nonlinear/internal/LevenbergMarquardtState.h:70-94);
 * gsx_lm_optimize / gsx_lm_iterate call exactly this function. */
typedef struct gsx_lm_state {
  double lambda;                 /* damping weight of the next trial            */
  double factor;                 /* its growth multiplier                       */
  double cost;                   /* nonlinear cost at the current values        */
  int32_t outer_iterations;      /* accepted steps                              */
  int32_t inner_iterations;      /* trials that changed the controller          */
} gsx_lm_state;
enum { GSX_LM_TAKE = 1,          /* step accepted: commit the trial values, relinearize           */
       GSX_LM_RETRY = 0,         /* step rejected: same linearization, larger damping             */
       GSX_LM_SETTLE = 2,        /* change below the relative tolerance: stop searching lambda    */
       GSX_LM_GIVE_UP = 3 };     /* damping passed lambda_upper_bound                             */
typedef struct gsx_lm_decision {
  int32_t verdict;               /* GSX_LM_*                                    */
  int32_t solved;                /* the damped system was factored              */
  double gain_ratio;             /* actual / predicted decrease (0 when not formed) */
  double cost_change;            /* cost(now) - cost(trial)                     */
  double trial_cost;             /* +inf when the trial cost was not consulted  */
  double lambda_tried;
} gsx_lm_decision;
gsx_status gsx_lm_decide(const gsx_lm_params* p, gsx_lm_state* state, int32_t solved, double model_at_zero,
                         double model_at_step, double trial_cost, gsx_lm_decision* out);
/* One LM trial without the accept/reject policy — the numeric body of LevenbergMarquardtOptimizer::tryLambda
 * (gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp:121-230), preceded when relinearize != 0 by the linearization
 * iterate() does (:252-262): damped solve, linearized error at 0 and at delta, retract into the trial values (the
 * current values stay), nonlinear error there — with ONE host synchronisation, as inside gsx_lm_optimize.
 * GSX_E_INDETERMINATE when the damped system cannot be factored. */
gsx_status gsx_lm_trial(gsx_handle h, int32_t relinearize, double lambda, int32_t diagonal_damping,
                        double min_diagonal, double max_diagonal, double* linear_error_0,
                        double* linear_error_delta, double* trial_error);
gsx_status gsx_gn_optimize(gsx_handle h, int32_t max_iterations, double relative_error_tol,
                           double absolute_error_tol, double error_tol, gsx_lm_result* r);
/* DoglegOptimizer (gtsam/nonlinear/DoglegOptimizer.cpp:84-121; DoglegOptimizerImpl::Iterate in
 * ONE_STEP_PER_ITERATION mode, DoglegOptimizerImpl.h:137-252) on the same kernels.  The result's
 * final_lambda / trace_lambda carry the trust-region radius delta.  DoglegParams::deltaInitial = 1.0. */
gsx_status gsx_dogleg_optimize(gsx_handle h, double delta_initial, int32_t max_iterations, double relative_error_tol,
                               double absolute_error_tol, double error_tol, gsx_lm_result* result);
/* Marginals::marginalCovariance(key) (gtsam/nonlinear/Marginals.cpp:107-136): the dA x dA block of H^-1 of the current
 * linearization in the variable's tangent space (column-major), from the undamped factorization on the device. */
gsx_status gsx_marginal_covariance(gsx_handle h, uint64_t key, double* out, int64_t n_out);
/* Marginals::jointMarginalCovariance(variables) (gtsam/nonlinear/Marginals.cpp:138-189): the joint covariance of up to 64
 * variables, D x D row-major with D = sum of their dimensions, blocks in the order of `keys` (the reference returns
 * them sorted by key: pass sorted keys for the same layout). */
gsx_status gsx_joint_marginal_covariance(gsx_handle h, const uint64_t* keys, int32_t n_keys, double* out, int64_t n_out);
/* Marginal covariances of MANY variables in one top-down pass over the undamped factorization (selected inversion: each
 * clique's block of H^-1 from its parent's, every clique of a level in parallel; the reference shares the same work through
 * the cached separator marginals of its Bayes tree, gtsam/inference/BayesTreeCliqueBase-inst.h).
 * gsx_marginal_blocks_size: the doubles gsx_marginal_covariances writes for these keys, the sum of d_v * d_v
 * (keys == NULL: every variable; n_keys is then ignored).  -1 for a NULL handle, a negative n_keys, an unknown key or a key
 * listed twice (the cases gsx_marginal_covariances answers with GSX_E_INVALID).  Needs no device.
 * gsx_marginal_covariances: the d_v x d_v blocks of H^-1 (column-major, tangent space, current linearization) of the listed
 * variables, one after the other in the order of `keys`; keys == NULL: every variable in ascending key order.  For a key
 * list only the cliques on the listed variables' paths to the root are visited; the blocks are the same bits as those of
 * the all-variables call.  No limit on n_keys or on the dimension of a variable.  GSX_E_INVALID: unknown or repeated key,
 * n_out != gsx_marginal_blocks_size; GSX_E_STATE: sharded handle, hard constraints; GSX_E_INDETERMINATE: the undamped
 * system cannot be factored; GSX_E_NOMEM: the covariance arena (one (n - 1) x (n + F - 1) block per clique that is not
 * a leaf-kernel clique, about the size of the front arena) does not fit; GSX_E_NO_DEVICE without a GPU. */
int64_t    gsx_marginal_blocks_size(gsx_handle h, const uint64_t* keys, int32_t n_keys);
gsx_status gsx_marginal_covariances(gsx_handle h, const uint64_t* keys, int32_t n_keys, double* out, int64_t n_out);

/* ---- partial relinearization / re-elimination on a fixed graph (first step) ----------------------
 * The numeric core of an iSAM2 update (gtsam/nonlinear/ISAM2.cpp:419-484: relinearize the factors of the variables
 * whose linearization point moved; :725-783: re-eliminate the part of the Bayes tree that contains them) on a FIXED
 * structure: graph, ordering and Bayes tree stay as they are; the factorization and every untouched subtree's Schur
 * complement stay resident in HBM.  Given the moved variables (`keys`; `states` = their new packed states one after the
 * other in that order, or NULL when the handle's values are already current) the call re-linearizes only the factors
 * touching them, re-assembles only the H panels of those factors' variables, and re-eliminates only the cliques holding
 * those variables and their ancestors.  The result is bit-identical to a full gsx_linearize + gsx_solve(lambda = 0)
 * factorization at the same values.  Needs the resident undamped factorization of the current linearization
 * (GSX_E_STATE otherwise); follow with gsx_solve(h, 0, ...) — which then only back-substitutes — or the marginal queries.
 * When most of the tree is dirty anyway the call takes the full path (same bits; the stats then report everything).
 * Adding / removing factors and variables: gsx_update below; the partial ("wildfire") back-substitution:
 * gsx_backsubstitute_wildfire. */
typedef struct gsx_partial_stats {
  int32_t n_factors_relinearized, n_panels_reassembled, n_fronts_reeliminated, n_fronts;
} gsx_partial_stats;
gsx_status gsx_relinearize_partial(gsx_handle h, const uint64_t* keys, int32_t n_keys, const double* states,
                                   int64_t n_states, gsx_partial_stats* out);
/* ---- ISAM2's partial ("wildfire") back-substitution --------------------------------------------------------------------
 * DeltaImpl::UpdateGaussNewtonDelta (gtsam/nonlinear/ISAM2-impl.cpp:48-77) -> optimizeWildfireNonRecursive
 * (gtsam/nonlinear/ISAM2Clique.cpp:261-287) on the resident undamped factorization: starting at the roots, a clique is
 * back-substituted when it was re-eliminated since the handle's last complete solution ("replaced": the cliques redone
 * by gsx_relinearize_partial, or all of them after a full factorization) or when one of its separator variables changed
 * (ISAM2Clique::isDirty, :68-90); its new frontal solution is kept — and its frontal variables count as changed — when
 * the clique was replaced or the solution moved by at least `threshold` in the infinity norm, and is put back to the old
 * values otherwise (valuesChanged / restoreFromOriginals, :175-201); children are visited only through a dirty parent.
 * threshold <= 0, or no complete undamped solution resident yet (gsx_solve with lambda = 0 leaves one, and so does
 * this call): every clique is back-substituted, as the reference does.  delta_out (tangent order of gsx_solve) may be
 * NULL; n_vars_solved = the reference's lastBacksubVariableCount (frontal variables of the cliques back-substituted).
 * A front of a relaxed tree (gsx_set_amalgamation) is visited or skipped as a whole, so the reference's clique-by-clique
 * pattern is reproduced exactly at relax = 0.  The dirty rule is evaluated at the top of the back-substitution kernels
 * (a clean clique's workgroup returns at once); one small bookkeeping launch follows every level.  Needs the resident
 * undamped factorization (GSX_E_STATE otherwise); not on a sharded handle. */
gsx_status gsx_backsubstitute_wildfire(gsx_handle h, double threshold, double* delta_out, int64_t n,
                                       int64_t* n_vars_solved, uint64_t* bad_key);

/* ---- structural update of a live handle: ISAM2::update(newFactors, newTheta, removeFactorIndices) ------------------------
 * (gtsam/nonlinear/ISAM2.cpp:395-484; the reference then detaches the affected part of the Bayes tree, re-orders it with
 * constrained COLAMD and re-eliminates it, ISAM2.cpp:117-362.)
 * `desc` describes the WHOLE graph after the update: the variables and factors that stay plus the new ones, in any
 * position.  factor_origin[i] = index, in the handle's current graph, of new factor i, or -1 for a factor that is new;
 * current factors that no entry names are removed.  A variable is kept when its key exists on both sides (type and
 * dimension must agree); new_values = the states of the NEW variables, packed in ascending-key order.
 * Semantics (iSAM2's): kept variables keep their current linearization point and kept factors their current [A b]
 * (copied on the device, not re-linearized); only the new factors are linearized.  Elimination order: the unaffected
 * variables keep their relative order, the affected ones — the variables of added / removed factors and the new
 * variables — are moved to the end, least-connected first (the constrained ordering of ISAM2.cpp:265-299, with a static
 * degree rule in place of CCOLAMD); the amalgamation setting of the current tree is kept; gsx_set_ordering afterwards
 * replaces the ordering like on any handle.
 * What is NOT incremental: the symbolic analysis is redone for the whole graph on the host (O(graph), not O(affected)),
 * and the next solve re-eliminates the whole tree on the device (milliseconds; gsx_relinearize_partial remains
 * available afterwards for moved variables).  The stats say what the update cost.  Not on a sharded handle. */
typedef struct gsx_update_stats {
  int32_t n_vars_added, n_vars_removed, n_factors_added, n_factors_removed, n_vars_affected, n_fronts;
  double host_symbolic_s;        /* ordering + symbolic analysis + upload of the tables */
  double device_s;               /* copies + linearization of the new factors (stream time, synchronised) */
} gsx_update_stats;
gsx_status gsx_update(gsx_handle h, const gsx_problem_desc* desc, const int32_t* factor_origin, const double* new_values,
                      int64_t n_new_values, gsx_update_stats* out);

/* DoglegOptimizerImpl::ComputeDoglegPoint (DoglegOptimizerImpl.cpp:26-86) on plain vectors (host). */
gsx_status gsx_dogleg_point(double delta, const double* dx_u, const double* dx_n, int64_t n, double* out);

/* ---- factors the backend does not know (seam S5: NonlinearFactor::linearize, gtsam/nonlinear/NonlinearFactor.h:145-146) ----
 * A graph may carry GSX_F_LINEAR slots for factor types outside the table above: the caller linearizes those on the CPU
 * at every new linearization point (factor->linearize(values) -> JacobianFactor) and refreshes their [A b] blocks in
 * place with this call — values = the factors' blocks one after the other, each m x (sum d + 1) column-major exactly as
 * `meas` at gsx_create (the slot's noise model is folded in here, as at creation).  gsx_linearize leaves these blocks
 * alone; the Hessian panels are re-assembled at the next solve.  gsx_error counts 0 for such a slot: the caller adds
 * its factors' nonlinear error itself. */
gsx_status gsx_set_block_jacobians(gsx_handle h, int32_t first_factor, int32_t n_factors, const double* values,
                                   int64_t n_values);
/* [R S d] of clique `front` (numbering of gsx_get_tree) from the factorization resident after a solve — the
 * GaussianConditional the reference's elimination stores in the Bayes-tree clique (R() / S() / d(),
 * gtsam/linear/GaussianConditional.h:243-252; BayesTreeCliqueBase-inst.h:27-31): n_frontal x n_cols column-major, the
 * columns in the order frontal variables, separator variables (both as gsx_get_tree lists them), rhs.  With the
 * reference's cliques (gsx_set_amalgamation(h, 0, .)) it is the reference's conditional entry for entry; out = NULL
 * queries the sizes. */
gsx_status gsx_get_conditional(gsx_handle h, int32_t front, int32_t* n_frontal, int32_t* n_cols, double* out,
                               int64_t n_out);

/* ---- the iterative linear solver: NonlinearOptimizerParams::linearSolverType = Iterative with PCGSolverParameters ------
 * (gtsam/nonlinear/NonlinearOptimizer.cpp:154-162: PCGSolver(*pcg).optimize(gfg) on the damped graph.)
 * preconditionedConjugateGradient (gtsam/linear/ConjugateGradientSolver.h:109-171) on the device for
 * A = J'J + lambda D, b = J'b, initial estimate zero, matrix-free over the [A b] blocks (csrc/pcg.hip), with
 * BlockJacobiPreconditioner (gtsam/linear/Preconditioner.cpp:87-176) or DummyPreconditioner (the identity).  The
 * subgraph preconditioner and SubgraphSolver are not offered.  A variable's tangent dimension may be at most 32, with
 * either preconditioner (GSX_E_INVALID from the solve beyond).
 * The loop is the reference's, condition for condition:
 *   for (k = 1; k <= max_iterations && (gamma > threshold || k <= min_iterations); k++), threshold =
 *   max(epsilon_abs, epsilon_rel^2 gamma_0), and at k % reset == 0 a restart from the true residual (reset >= 1).
 * gsx_pcg_stats.iterations counts the loop bodies executed: gamma after `iterations` bodies is gamma_final (the
 * reference's own counter stands one higher when its loop ends).  converged = gamma_final <= threshold; running into
 * max_iterations is not an error — the estimate is returned with converged = 0, as the reference returns it.
 * GSX_E_INDETERMINATE: a diagonal block has no Cholesky factor (*bad_key = its variable), or p'Ap is non-positive or
 * non-finite while gamma > threshold (*bad_key untouched).
 * gamma_0 = 0 (linearized at a stationary point) is NOT special-cased, because the reference does not: with
 * min_iterations >= 1 the first body computes alpha = 0 / 0, and the estimate returned is all NaN, status GSX_OK,
 * gamma_final NaN, converged 0; with min_iterations = 0 no body runs and the estimate is zero. */
enum { GSX_PRECOND_DUMMY = 0, GSX_PRECOND_BLOCK_JACOBI = 1 };
enum { GSX_SOLVER_MULTIFRONTAL = 0, GSX_SOLVER_PCG = 1 };
typedef struct gsx_pcg_params {
  int32_t max_iterations;        /* 500   ConjugateGradientSolver.h:47                                   */
  int32_t min_iterations;        /* 1     :46                                                            */
  int32_t reset;                 /* 501   :48                                                            */
  double epsilon_rel;            /* 1e-3  :49                                                            */
  double epsilon_abs;            /* 1e-3  :50                                                            */
  int32_t preconditioner;        /* GSX_PRECOND_*: the reference's PCGSolverParameters has no default
                                    (a null pointer); the default here is GSX_PRECOND_BLOCK_JACOBI     */
} gsx_pcg_params;
typedef struct gsx_pcg_stats {
  int32_t iterations;            /* loop bodies executed                                                 */
  int32_t converged;             /* gamma_final <= threshold                                             */
  double gamma_initial, gamma_final, threshold;
} gsx_pcg_stats;
void gsx_pcg_params_default(gsx_pcg_params* p);
/* The damped solve of gsx_solve by PCG on a linearized handle; D = I or clamp(diag J'J, min_diagonal, max_diagonal)
 * as there.  Builds no fronts and leaves the factorization arena alone.  delta_out (may be NULL), stats_out (may be
 * NULL), bad_key (may be NULL); delta stays on the device for gsx_retract / gsx_linear_error.  GSX_E_STATE: not
 * linearized, sharded handle, hard constraints (the step there is a KKT solve). */
gsx_status gsx_solve_pcg(gsx_handle h, double lambda, int32_t diagonal_damping, double min_diagonal, double max_diagonal,
                         const gsx_pcg_params* params, double* delta_out, int64_t n, gsx_pcg_stats* stats_out,
                         uint64_t* bad_key);
/* Which linear solver gsx_lm_optimize / gsx_lm_iterate / gsx_lm_trial / gsx_gn_optimize take their step from.  kind =
 * GSX_SOLVER_MULTIFRONTAL (the default of a new handle; params ignored) or GSX_SOLVER_PCG (params = NULL: the defaults).
 * A PCG handle evaluates the two linearized errors of a trial directly on [A b] (the model-decrease identity holds for an
 * exact solve only), adds the iterations of every solve into gsx_lm_result.pcg_iterations / gsx_stats.n_pcg_iterations,
 * and treats GSX_E_INDETERMINATE from the solve like a failed factorization.  GSX_E_STATE: PCG on a sharded handle or on
 * a problem with hard constraints; gsx_dogleg_optimize on a PCG handle.  The marginal and conditional queries need the
 * direct factorization exactly as before, whatever the solver kind. */
gsx_status gsx_set_linear_solver(gsx_handle h, int32_t kind, const gsx_pcg_params* params);

/* ---- the linear seam (NonlinearOptimizer::solve override) ------------------- */
/* desc must contain only GSX_F_LINEAR factors and GSX_VAR_VECTOR variables;
 * ordering may be NULL (own minimum degree).  delta_out in variable-index order. */
gsx_status gsx_solve_gfg(const gsx_problem_desc* desc, const uint64_t* ordering,
                         int32_t device, double* delta_out, int64_t n, uint64_t* bad_key);
/* The same seam with the structure kept: NonlinearOptimizer::solve (gtsam/nonlinear/NonlinearOptimizer.h:129-130) is
 * called once per LM trial on graphs of ONE structure (same keys, dims, ordering; only the numbers and the damping
 * priors' sigmas change).  Create the handle once (gsx_create on the GSX_F_LINEAR description + gsx_set_ordering: the
 * symbolic analysis and every device table are built once), then per call hand over only the [A b] blocks of all
 * factors, one after the other as in `meas` (blocks = NULL: solve what the handle holds).  delta_out as above. */
gsx_status gsx_solve_gfg_h(gsx_handle h, const double* blocks, int64_t n_blocks, double* delta_out, int64_t n,
                           uint64_t* bad_key);

/* ---- Pose3 initialization: InitializePose3 (gtsam/slam/InitializePose3.{h,cpp}, gtsam/slam/InitializePose.h) --------------
 * The initial guess a Pose3 pose graph needs, in the reference's three stages: (1) chordal relaxation — one linear
 * least-squares solve over relaxed rotation matrices, every 3 x 3 block then projected onto SO(3) (Rot3::ClosestTo);
 * (2) optionally the Tron-Vidal Riemannian gradient iterations on the rotations; (3) Gauss-Newton on the full poses from
 * those rotations and zero translations (one iteration by default).
 * These calls take a description, not a handle: they build their own internal handles (direct solver, one device) and free
 * them before returning.
 * What is used of `desc`: GSX_F_BETWEEN on two POSE3 variables and GSX_F_PRIOR on a POSE3 variable; every other factor is
 * ignored, as buildPoseGraph drops it (InitializePose.h:36-52).  A prior becomes a between factor from the ANCHOR (key
 * 99999999, initialize::kAnchorKey) with the prior's noise; a variable of `desc` with that key: GSX_E_INVALID.
 * The rotation weight of a factor is the first entry of whiten(e_0) under its noise model, which the reference takes for a
 * precision (InitializePose3.cpp:48-51, :62): 1 (Unit), 1 / sigma (Isotropic), 1 / sigma_0 (Diagonal / Constrained; 1 when
 * sigma_0 = 0, Constrained::whiten), R(0, 0) (Gaussian).  A robust model counts as its BASE model: a deliberate deviation —
 * the reference's Robust::whitenInPlace also reweights (NoiseModel.h:711-712, WhitenSystem), so its precisions[0] under
 * Huber over sigma_0 is sqrt(weight(1 / sigma_0)) / sigma_0, a value that depends on the loss's k and not on the data.
 * A factor of weight 0 (an infinite sigma, Isotropic::Precision(6, 0)) contributes nothing to the relaxed system nor to the
 * Gauss-Newton graph; it stays an edge of the gradient iterations, which never look at the noise.  Limit: a Diagonal /
 * Constrained model with sigma_0 infinite and other sigmas finite is dropped from the Gauss-Newton graph as a whole as well,
 * where the reference would keep its other five rows (gsx_create takes no infinite sigma); only Isotropic::Precision(6, 0)
 * is a factor that truly vanishes.
 * Rotation arrays (rot_out, rot) hold 9 doubles, row-major, per POSE3 variable of `desc`, in the order of `desc`.
 * values_out is packed like gsx_get_values for `desc`.  The reference returns only the poses its pose graph holds; here a
 * variable that is not POSE3, or a POSE3 variable no used factor holds, is copied from `given` by gsx_initialize_pose3
 * (GSX_E_INVALID when there is one and given == NULL) and left as the caller filled it by gsx_pose3_compute_poses;
 * gsx_pose3_orientations_chordal writes the identity for such a pose, gsx_pose3_orientations_gradient the rotation of
 * `given`.
 * GSX_E_INVALID (before any device is touched): malformed description, anchor-key collision, wrong n_out / n_rot /
 * n_given, use_gradient without `given`.  GSX_E_NO_DEVICE: no usable device (every call but gsx_pose3_init_structure).
 * GSX_E_INDETERMINATE: some pose is not joined to the anchor by factors of non-zero weight (no prior: the relaxed system
 * is rank deficient and the reference throws IndeterminantLinearSystemException), or a factorization failed. */
typedef struct gsx_init_pose3_params {
  int32_t use_gradient;             /* 0: chordal (default) ; 1: computeOrientationsGradient            */
  int32_t max_gradient_iterations;  /* 10000 (InitializePose3.h default)                               */
  int32_t set_ref_frame;            /* 1                                                                */
  int32_t single_iter;              /* 1: computePoses does one GN iteration                            */
} gsx_init_pose3_params;
void gsx_init_pose3_params_default(gsx_init_pose3_params* p);
/* InitializePose3::initialize (InitializePose3.cpp:296-319); p == NULL: the defaults; gradient_iterations (may be NULL):
 * the gradient iterations executed, 0 for chordal */
gsx_status gsx_initialize_pose3(const gsx_problem_desc* desc, const double* given, int64_t n_given,
                                const gsx_init_pose3_params* p, int32_t device,
                                double* values_out, int64_t n_out, int32_t* gradient_iterations);
/* buildPose3graph + computeOrientationsChordal (:37-114).  The relaxed 9-vector of a pose splits into the three rows of
 * its rotation and the system into three identical ones over 3-dimensional variables that differ in the anchor prior's
 * right-hand side (e_1, e_2, e_3) only: one internal handle of 3 x 7 GSX_F_LINEAR blocks [-w I, w Rij | 0] written on the
 * device, one symbolic analysis, three solves, one projection kernel. */
gsx_status gsx_pose3_orientations_chordal(const gsx_problem_desc* desc, int32_t device, double* rot_out, int64_t n_out);
/* computeOrientationsGradient (:117-218, 256-275) from the rotations of `given` (packed Values of desc).  Two launches per
 * iteration (gradient of every node from the old rotations, then the update by the full exponential map), no host
 * synchronisation inside a batch of 32 iterations; stops after iteration `it` when it > 20 and the largest gradient norm
 * is below 5e-3.  *iterations (may be NULL) = iterations executed.  The output is R^-1, or Rref R^-1 with set_ref_frame. */
gsx_status gsx_pose3_orientations_gradient(const gsx_problem_desc* desc, const double* given, int64_t n_given,
                                           int32_t max_iter, int32_t set_ref_frame, int32_t device,
                                           double* rot_out, int64_t n_out, int32_t* iterations);
/* initialize::computePoses<Pose3> (InitializePose.h:57-97): Gauss-Newton (gsx_gn_optimize; 1 iteration, or its defaults
 * 100 / 1e-5 / 1e-5 / 0 when single_iter == 0) on the pose graph + the anchor + a Unit prior on the anchor, from
 * (rot, zero translation); the anchor is dropped from the result. */
gsx_status gsx_pose3_compute_poses(const gsx_problem_desc* desc, const double* rot, int64_t n_rot, int32_t single_iter,
                                   int32_t device, double* values_out, int64_t n_out);
/* Rot3::ClosestTo on n matrices (SO3.cpp:202-208), row-major in and out: U diag(1, 1, det(U V')) V' by one-sided Jacobi
 * rotations in registers (no M'M is formed) and two polishing passes (csrc/init_math.h), one thread per matrix — the projection kernel of the chordal stage.  The
 * answer is unique only when sigma_2 + sigma_3 > 0 (det > 0) or sigma_2 > sigma_3 (det < 0). */
gsx_status gsx_closest_rotations(const double* m, int64_t n, int32_t device, double* r_out);
/* host only, needs no device: the pose graph of buildPoseGraph<Pose3> (InitializePose.h:36-52) and the adjacency of
 * createSymbolicGraph (InitializePose3.cpp:221-253).  Nodes: the POSE3 variables of desc in its order (0 .. P-1), the anchor
 * = P.  Edges in factor order, a prior as an edge from the anchor: edge_from / edge_to [*n_edges] (call once with NULL
 * arrays for *n_edges); adj_ptr [P + 2], adj [2 * n_edges] = the edges at each node in factor order; adj_cap = the
 * capacity of adj (GSX_E_INVALID when too small).  Any array may be NULL. */
gsx_status gsx_pose3_init_structure(const gsx_problem_desc* desc, int32_t* n_edges, int32_t* edge_from, int32_t* edge_to,
                                    int32_t* adj_ptr, int32_t* adj, int64_t adj_cap);
/* Stage times (ms) of the LAST initializer call of the process (not thread-safe; for tools/init_probe.py), n = 8:
 * [0] host: lowering + ordering + symbolic analysis + upload of the relaxed system; [1] chordal_blocks_kernel; [2] the three
 * relaxed solves; [3] closest_rotation_kernel; [4] host: the same for the anchor graph; [5] pose_states_kernel +
 * gsx_gn_optimize; [6] the gradient iterations; [7] the number of gradient iterations executed.  [1]-[3], [5], [6] are HIP
 * events on the internal handle's stream; a stage that did not run is 0. */
gsx_status gsx_pose3_init_timings(double* out_ms, int32_t n);

/* ---- Pose2 initialization: lago (gtsam/slam/lago.{h,cpp}, gtsam/slam/InitializePose.h) -------------------------------------
 * Linear approximation for graph optimization: (1) a spanning tree of the pose graph, (2) the cumulative orientation of
 * every pose along the tree, which removes the 2 k pi wrap-around of every loop-closing edge (chord), (3) one linear
 * least-squares solve in the orientations, (4) one in the full poses.  The tree is built on the host; everything from (2) on
 * runs on the device, the two solves on internal handles (direct solver, one device) that the call builds and frees.
 * What is used of `desc`: GSX_F_BETWEEN on two POSE2 variables and GSX_F_PRIOR on a POSE2 variable; every other factor is
 * ignored (a prior on a VECTOR(1) orientation included), as buildPoseGraph drops it (InitializePose.h:36-52).  A prior
 * becomes an edge from the ANCHOR (key 99999999) with the prior's noise; a variable of `desc` with that key:
 * GSX_E_INVALID.  The measured angle is measured().theta(): kept as stored when inside (-pi, pi], else atan2(sin, cos).
 * Noise: the reference needs a noiseModel::Diagonal (lago.cpp:142-162, :344-348): GSX_NOISE_UNIT / ISOTROPIC / DIAGONAL /
 * CONSTRAINED are taken, GSX_NOISE_GAUSSIAN or any robust kind on a used factor is GSX_E_INVALID (the reference throws
 * invalid_argument), and so is a sigma that is not positive (a stated limit: the reference would carry a constrained row).
 * Nodes: the POSE2 variables of `desc` in its order (0 .. P-1), the anchor = P; edges: the used factors in factor order.
 * The tree: use_odometric_path != 0: findOdometricPath (lago.cpp:202-226) — the first edge between consecutive keys gives a
 * node its parent, the smallest key seen is attached to the anchor, an edge from the anchor is never consecutive;
 * else findMinimumSpanningTree (:229-260) — Kruskal with unit weights in factor order, then the reference's stack-driven
 * walk from the anchor.  GSX_E_INVALID where the reference's tree.at(key) throws: a used pose without a tree entry (a key
 * gap on the odometric path; a pose not joined to the anchor in MST mode, e.g. no prior).  On the odometric path the pose
 * attached to the anchor may carry no prior (the reference's deltaThetaMap.at throws there): the orientation system has no
 * row that fixes its gauge and the numeric calls return GSX_E_INDETERMINATE; so does a failed factorization.
 * The anchor's orientation prior has sigma 0 in the reference (:43-44, :196-197); here theta_anchor = 0 is substituted
 * before the solve (the same solution): the orientation system has one scalar variable per used pose and an edge from the
 * anchor is a unary row.  The pose system has the used poses and the anchor as 3-dimensional variables and the anchor's
 * prior Variances(1e-6, 1e-6, 1e-8) (:45-46, :355).
 * values_out is packed like gsx_get_values for `desc`; the angle of a POSE2 state is written as Pose2(x, y, theta).theta()
 * returns it, in (-pi, pi].  A variable that is not POSE2, or a POSE2 variable no used factor holds, is copied from `given`
 * (GSX_E_INVALID when there is one and given == NULL).  GSX_E_NO_DEVICE: no usable device (every call but
 * gsx_lago_structure); every GSX_E_INVALID above comes before a device is touched. */
/* lago::initialize(graph, useOdometricPath) (lago.cpp:375-388); given may be NULL (see above) */
gsx_status gsx_lago_initialize(const gsx_problem_desc* desc, int32_t use_odometric_path, const double* given,
                               int64_t n_given, int32_t device, double* values_out, int64_t n_out);
/* lago::initializeOrientations (:297-305): one double per POSE2 variable of desc, in its order, NOT wrapped (the
 * reference's VectorValues); 0 for a pose no used factor holds.  n_out = the number of POSE2 variables. */
gsx_status gsx_lago_initialize_orientations(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t device,
                                            double* theta_out, int64_t n_out);
/* lago::initialize(graph, initialGuess) (:391-409): the odometric tree; x and y of every pose are those of `given`, bit
 * for bit, theta is lago's. */
gsx_status gsx_lago_initialize_with_guess(const gsx_problem_desc* desc, const double* given, int64_t n_given, int32_t device,
                                          double* values_out, int64_t n_out);
/* host only, needs no device: the pose graph, the tree and the split of getSymbolicGraph (:101-138).  edge_from / edge_to
 * [*n_edges] (call once with every array NULL for *n_edges; the tree is then not built); parent [P + 1]: the parent node,
 * the anchor its own, -1 for a pose without a tree entry; delta [P + 1]: the signed deltaTheta of the edge parent -> node,
 * inserted once (a duplicate does not overwrite it), 0 without one; tree_ids [*n_tree] and chord_ids [*n_edges - *n_tree]:
 * edge indices, each list in factor order (room for *n_edges each is enough); *max_depth: edges on the longest path from a
 * pose to the anchor.  Any pointer may be NULL. */
gsx_status gsx_lago_structure(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t* n_edges, int32_t* edge_from,
                              int32_t* edge_to, int32_t* parent, double* delta, int32_t* n_tree, int32_t* tree_ids,
                              int32_t* chord_ids, int32_t* max_depth);
/* lago::computeThetasToRoot (:56-98) on a forest of n nodes given by parent links (a root: parent[i] == i, its delta is
 * ignored): out[i] = the sum of delta over the path from i to its root.  Pointer jumping: ceil(log2(max depth + 1)) launches
 * enqueued back to back, double-buffered.  The summation order differs from the reference's walk: per node
 * |out - reference| <= depth * 2^-53 * sum |delta| over its path.  GSX_E_INVALID: a link out of range or a cycle. */
gsx_status gsx_lago_thetas_to_root(const int32_t* parent, const double* delta, int64_t n, int32_t device, double* out);
/* the regularized deltaTheta of every edge, in edge order (buildLinearOrientationGraph, :165-199): a tree edge keeps its
 * measurement, a chord takes dtheta - 2 pi round((dtheta + theta_root[key1] - theta_root[key2]) / 2 pi).  n_out = n_edges. */
gsx_status gsx_lago_regularized_measurements(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t device,
                                             double* out, int64_t n_out);
/* Stage times (ms) of the LAST lago call of the process (not thread-safe; for tools/lago_probe.py), n = 8: [0] host:
 * lowering + ordering + symbolic analysis + upload of the orientation system; [1] the lago_theta_to_root_kernel rounds;
 * [2] lago_orientation_blocks_kernel; [3] the orientation solve; [4] host: as [0] for the pose system; [5]
 * lago_pose_blocks_kernel; [6] the pose solve; [7] lago_compose_kernel.  [1]-[3], [5]-[7] are HIP events on the internal
 * handles' streams; a stage that did not run is 0. */
gsx_status gsx_lago_timings(double* out_ms, int32_t n);

/* ---- Landmark triangulation (gtsam/geometry/triangulation.{h,cpp}) -----------------------------------------------------------
 * triangulatePoint3 (DLT or LOST, optionally refined by LM on the one Point3) and triangulateSafe for MANY tracks at once: a
 * track is the list of (camera, pixel) observations of one landmark; every track is independent work for one lane (fewer than
 * 64 observations) or one wave of the device (csrc/triangulate.hip; the per-track arithmetic is csrc/triangulate_math.h).
 * Cameras: GSX_CAMERA_POSE3_CAL3_S2 — a Pose3 state (R row-major 9, t 3) per camera and Cal3_S2 calibrations (fx, fy, s, u0,
 * v0), ONE shared (n_calibrations = 1) or one per camera (n_calibrations = n_cameras): PinholePose / PinholeCamera<Cal3_S2>;
 * GSX_CAMERA_CAL3BUNDLER — the 17-double state of a GSX_VAR_CAMERA variable per camera (calibrations ignored):
 * PinholeCamera<Cal3Bundler>, whose measurements are undistorted as undistortMeasurementInternal does (triangulation.h:
 * 260-268; Cal3Bundler::calibrate's fixed-point loop, at most 10 rounds, tol 1e-5, Cal3Bundler.cpp:93-128).  Cal3DS2, fisheye,
 * unified, spherical and stereo cameras are not taken.
 * DLT (triangulateHomogeneousDLT, triangulation.cpp:27-56; DLT, base/Matrix.cpp:556-574): the rows p.x P2 - P0, p.y P2 - P1
 * are streamed into a 4 x 4 triangle by Givens rotations and that triangle gets a one-sided Jacobi SVD — A'A is never formed;
 * rank = singular values above rank_tol (absolute), rank < 3 is underconstrained.  LOST (triangulateLOST, :86-147): the same
 * streaming reduction of [A b], then a column-pivoted QR of the 3 x 3 with ColPivHouseholderQR's RELATIVE rank rule (pivots
 * above rank_tol x the largest).  Refinement (triangulateNonlinear -> optimize, :177-195): LM with lambdaInitial 1,
 * lambdaFactor 10, maxIterations 100, absoluteErrorTol 1.0 on TriangulationFactors (gtsam/slam/TriangulationFactor.h:122-136:
 * behind the camera a zero Jacobian and the error 2 fx (1, 1)), the decisions of gsx_lm_decide, inside the kernel.
 * Status per track, TriangulationResult::Status (triangulation.h:644) with the cheirality checks on: a track with fewer than 2
 * observations or an underconstrained system is DEGENERATE; a final point with transformTo(point).z <= 0 in some camera is
 * BEHIND_CAMERA; with safe != 0 then triangulateSafe's loop (:719-745): FAR_POINT, OUTLIER.  CALIBRATION_FAILED is the
 * reference's runtime_error of Cal3Bundler::calibrate.  Limits: a homogeneous solution with v[3] == 0 is DEGENERATE (the
 * reference hands out a non-finite point); LOST under a robust model uses the base model's sigmas (the reference's
 * Robust::sigmas throws).  A track that is not VALID leaves NaN in its point. */
enum { GSX_TRI_VALID = 0, GSX_TRI_DEGENERATE = 1, GSX_TRI_BEHIND_CAMERA = 2, GSX_TRI_OUTLIER = 3, GSX_TRI_FAR_POINT = 4,
       GSX_TRI_CALIBRATION_FAILED = 5 };
enum { GSX_CAMERA_POSE3_CAL3_S2 = 0, GSX_CAMERA_CAL3BUNDLER = 1 };
/* TriangulationParameters (triangulation.h:562-607) + the arguments of triangulatePoint3 (:424-430) */
typedef struct gsx_triangulation_params {
  double rank_tol;                 /* 1e-9 (triangulatePoint3); TriangulationParameters' own default is 1.0                */
  int32_t optimize;                /* 0; enableEPI: refine by LM                                                          */
  int32_t use_lost;                /* 0                                                                                   */
  int32_t noise_kind;              /* -1: no model — unwhitened factors, LOST sigma 1e-4 (:439); else GSX_NOISE_UNIT /
                                      ISOTROPIC / DIAGONAL / GAUSSIAN of dimension 2, robust bits allowed.
                                      GSX_NOISE_CONSTRAINED or a sigma that is not positive: GSX_E_INVALID, the reference's
                                      factor does not support them (TriangulationFactor.h:144)                            */
  double noise[5];                 /* the model's parameters as in gsx_problem_desc.noise, then the robust parameter      */
  double landmark_distance_threshold;            /* -1; <= 0: off                                                         */
  double dynamic_outlier_rejection_threshold;    /* -1; <= 0: off; compared with the LARGEST reprojection error norm      */
  int32_t safe;                    /* 0: triangulatePoint3 — only the underconstrained and cheirality outcomes;
                                      1: triangulateSafe                                                                  */
} gsx_triangulation_params;
void gsx_triangulation_params_default(gsx_triangulation_params* p);
/* triangulatePoint3 / triangulateSafe on n_tracks tracks.  track_ptr [n_tracks + 1] is a CSR into obs_camera (camera index)
 * and obs_xy (2 doubles per observation).  Writes points_out [3 n_tracks] and status_out [n_tracks]; lm_counts_out (may be
 * NULL) [2 n_tracks]: the accepted LM iterations and the trials that changed the controller, 0 without refinement.  params
 * == NULL: the defaults.  Zero tracks: GSX_OK.  GSX_E_INVALID (before a device is touched): a camera index out of range, a
 * malformed CSR, a refused noise model.  GSX_E_NO_DEVICE without a usable device. */
gsx_status gsx_triangulate(int32_t camera_kind, const double* cameras, int32_t n_cameras, const double* calibrations,
                           int32_t n_calibrations, const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_camera,
                           const double* obs_xy, const gsx_triangulation_params* params, int32_t device, double* points_out,
                           int32_t* status_out, int32_t* lm_counts_out);
/* host only, needs no device: the tracks of a problem description.  The GSX_F_SFM and GSX_F_PROJECTION factors are grouped
 * per landmark (their second key); landmarks in the order of desc, the observations of a landmark in factor order; every
 * other factor type is ignored.  landmark_vars [*n_landmarks] variable indices, track_ptr [*n_landmarks + 1], obs_factor
 * [*n_observations] factor indices; call once with NULL arrays for the sizes.  GSX_E_INVALID: a landmark seen by both camera
 * kinds, a malformed factor. */
gsx_status gsx_triangulation_tracks(const gsx_problem_desc* desc, int32_t* n_landmarks, int64_t* n_observations,
                                    int32_t* landmark_vars, int64_t* track_ptr, int32_t* obs_factor);
/* The practical entry: triangulate every landmark of a problem from the cameras in `values` (packed like gsx_get_values).
 * GSX_F_SFM observations use the GSX_VAR_CAMERA variable; GSX_F_PROJECTION observations the POSE3 variable, the factor's
 * calibration and, where present, its body_P_sensor (composed into the pose on the device).  values_out = values with the
 * VALID landmarks overwritten; a landmark that fails keeps its input value.  status_out: one entry per landmark in the order
 * of gsx_triangulation_tracks (room for n_vars entries always suffices); *n_landmarks_out (may be NULL) their number. */
gsx_status gsx_triangulate_landmarks(const gsx_problem_desc* desc, const double* values, int64_t n_values,
                                     const gsx_triangulation_params* params, int32_t device, double* values_out,
                                     int32_t* status_out, int32_t* n_landmarks_out);
/* Stage times (ms) of the LAST triangulation call of the process (not thread-safe; for tools/triangulate_probe.py), n = 5:
 * [0] host: sorting the tracks into the two classes; [1] triangulate_cameras_kernel; [2] triangulate_short_kernel; [3]
 * triangulate_long_kernel; [4] the whole call on the host clock, transfers included.  [1]-[3] are HIP events. */
gsx_status gsx_triangulate_timings(double* out_ms, int32_t n);

/* ---- Smart projection factors (GSX_F_SMART_PROJECTION) ------------------------------------------------------------------------
 * Linearization (csrc/smart_math.h, csrc/smart.hip): with a VALID point, per view F_i (2 x 6: PinholePose's projection
 * Jacobian with respect to the pose, times the compose Jacobian of SmartFactorBase.h:225-236 with body_P_sensor), E_i (2 x 3)
 * and b_i = z_i - h_i, all whitened by 1 / sigma; then three Householder reflectors of E (2 nk x 3) are applied to [F b] and
 * rows 3 .. 2 nk - 1 are the factor's block A = Q_2'[F b].  Any orthonormal basis Q_2 of the left null space of E gives the
 * reference's F'F - F'E (E'E)^-1 E'F with its gradient and constant term, so the block is comparable with the reference
 * through [A b]'[A b] only, never entry by entry.  Without a valid point: the all-zero block and the error 0
 * (SmartProjectionFactor.h:214-220, :427-429).  The error is totalReprojectionError: 0.5 |whitened (h - z)|^2 over all 2 nk
 * rows at the triangulated point — not 0.5 |b|^2 of the projected block; the two differ in the reference as well.
 * The re-triangulation cache (decideIfTriangulate, SmartProjectionFactor.h:127-165) lives in the handle, per factor: the
 * camera poses of the last triangulation, its point and its status.  It is empty after gsx_create and after gsx_update.
 * Every call that evaluates a smart factor consults and updates it in stream order — gsx_linearize, gsx_error, the trial
 * error of gsx_retract, gsx_lm_trial, the drivers, gsx_relinearize_partial — and re-triangulates only when some camera pose
 * differs from the cached one by more than retriangulation_threshold in an entry of R or t (Pose3::equals).  With a
 * threshold of 0 only bit-identical poses reuse the cached point, which is the point a new triangulation would give.
 * Limit: a cached point that is no longer in front of every camera at the current poses (the reference throws
 * CheiralityException there) gives the all-zero block / the error 0, counted in n_smart_invalid.
 * A sharded handle with a smart factor in its graph: GSX_E_STATE from gsx_set_ordering.
 * gsx_smart_points: SmartProjectionFactor::point() of every smart factor in graph order — the point of its last
 * triangulation (NaN unless VALID) in points_out [3 n] and its GSX_TRI_* status, or -1 when it was never triangulated, in
 * status_out [n]; either array may be NULL.  n must be the number of smart factors of the graph (GSX_E_INVALID otherwise;
 * n = 0 with no smart factor is GSX_OK). */
gsx_status gsx_smart_points(gsx_handle h, double* points_out, int32_t* status_out, int64_t n);

/* ---- Translation averaging: 1dSfM (gtsam/sfm/MFAS.{h,cpp}, gtsam/sfm/TranslationRecovery.{h,cpp}) ----------------------------
 * MFAS (minimum feedback arc set, MFAS.cpp:36-171) for n_dirs projection directions at once over one edge set
 * (csrc/mfas.hip): one workgroup per direction, the node sums in LDS.
 *   edges: n_edges unordered pairs (key1[i], key2[i]); a pair given twice in the same order keeps the LAST entry (the map
 *     assignment of MFAS.cpp:119); a pair present in both orders, or key1[i] == key2[i], is GSX_E_INVALID (absWeightOfEdge
 *     :85-91 cannot tell the two orders apart).
 *   weights: either edge_dirs (3 per edge) and proj_dirs (3 per direction): w[d][e] = edge_dirs[e] . proj_dirs[d]
 *     (:118-121, summed x, y, z in that order without fused multiply-add), or, with edge_dirs == NULL, `weights`
 *     [n_dirs x n_edges] given (the MFAS(edgeWeights) constructor).  The entry of a superseded duplicate is ignored.
 *   out_mean[e] = sum over d, in order of d, of out_weights[d][e] / n_dirs (python/gtsam/examples/
 *     TranslationAveragingExample.py:84-87); out_weights [n_dirs x n_edges] or NULL; out_ordering [n_dirs x n_nodes] keys or
 *     NULL, n_nodes = the distinct keys of the edges.  A superseded duplicate gets its successor's values.
 * The ordering: the reference removes "the first root in unordered_map order", which is unspecified.  Any order among the
 * roots (in-weight sum < 1e-8) gives the same outlier weights apart from edges with |w| < 1e-8, so out_ordering is *a* valid
 * MFAS ordering, defined here as: the root of the lowest key first; without a root the node of the largest (out + 1) /
 * (in + 1), the lowest key on an exact tie.  No atomics: two runs give the same bits.
 * LIMIT: at most GSX_MFAS_MAX_NODES = 8192 distinct keys — two doubles and a flag byte of LDS per node, 136 KiB of the
 * 160 KiB of a gfx950 workgroup — and n_dirs x n_edges below 2^31.  Above:
 * GSX_E_INVALID with a line on stderr, never a skipped launch.  Every GSX_E_INVALID of the arguments comes before a device
 * is touched; the launcher's own LDS check (dynamic + static LDS of the kernel against 160 KiB) follows the device check and
 * cannot fire within the node limit.
 * The launch takes min(n_dirs, CUs x resident workgroups per CU) workgroups, each striding over the directions.  The
 * environment variable GSX_MFAS_MAX_GRID (a positive integer, read at every call) caps that number: a tuning and test
 * knob — the outputs are the same bits at any grid. */
#define GSX_MFAS_MAX_NODES 8192
gsx_status gsx_mfas_outlier_weights(const uint64_t* key1, const uint64_t* key2, int64_t n_edges,
                                    const double* edge_dirs, const double* proj_dirs, const double* weights,
                                    int32_t n_dirs, int32_t device, double* out_mean, double* out_weights,
                                    uint64_t* out_ordering);
/* Stage times (ms) of the LAST MFAS call of the process (not thread-safe; for tools/translation_probe.py), n = 4: [0] host:
 * key ranking, duplicate handling, CSR; [1] mfas_kernel; [2] mfas_mean_kernel; [3] the whole call on the host clock,
 * transfers included.  [1]-[2] are HIP events. */
gsx_status gsx_mfas_timings(double* out_ms, int32_t n);

/* TranslationRecovery (TranslationRecovery.cpp:49-228).  The measurements: n_unit direction edges (keys, 3 doubles each —
 * taken as given — and a noise model each: GSX_NOISE_* kind and a CSR of parameters sized for m = 3), `scale`, n_between
 * BinaryMeasurement<Point3> edges in the same layout, and n_given initial translations (keys + 3 doubles each). */
typedef struct gsx_translation_input {
  int64_t n_unit;
  const uint64_t *unit_key1, *unit_key2;
  const double* unit_dirs;            /* [3 n_unit] */
  const int32_t* unit_noise_kind;     /* [n_unit] */
  const int64_t* unit_noise_ptr;      /* [n_unit + 1] CSR into unit_noise */
  const double* unit_noise;
  double scale;
  int64_t n_between;
  const uint64_t *between_key1, *between_key2;
  const double* between_meas;         /* [3 n_between] */
  const int32_t* between_noise_kind;
  const int64_t* between_noise_ptr;
  const double* between_noise;
  int64_t n_given;
  const uint64_t* given_keys;
  const double* given_values;         /* [3 n_given] */
} gsx_translation_input;
typedef struct gsx_translation_params {
  gsx_lm_params lm;            /* default: gsx_lm_params_legacy (TranslationRecovery() default-constructs LevenbergMarquardtParams) */
  int32_t use_bilinear;        /* BATA: one VECTOR(1) scale variable Symbol('S', i) per kept edge, initial value 1 */
  uint32_t seed;               /* std::mt19937 seed of the random initial values; default 42 (TranslationRecovery.cpp:42) */
  double prior_sigma;          /* isotropic sigma of the origin prior; default 0.01 (TranslationRecovery.h:111-112) */
} gsx_translation_params;
void gsx_translation_params_default(gsx_translation_params* p);
/* Host only, needs no device: the graph and initial values TranslationRecovery::run builds (csrc/translation_graph.cpp).
 *   - zero edges merged: union-find over the unit edges whose direction has every component within 1e-9 of 0
 *     (Unit3::equals against Unit3(0, 0, 0), :49-60); every edge of both lists is rewritten onto the representatives and
 *     dropped when its ends coincide (:65-76).  The representative of a set is the root DSFMap gives it: union by rank,
 *     the root of key1 on a tie (gtsam/base/DSFMap.h:87-102).
 *   - factors in edge order: GSX_F_TRANSLATION, or with use_bilinear GSX_F_BILINEAR_TRANSLATION with the scale variable
 *     Symbol('S', i) = ('S' << 56 | i), i counting the KEPT edges (buildGraph, :99-117);
 *   - priors (addPrior, :119-143): GSX_F_PRIOR at the origin on the first kept edge's key1 (Isotropic prior_sigma); without
 *     between edges a GSX_F_PRIOR scale * z on that edge's key2 with that edge's noise; otherwise one GSX_F_BETWEEN on
 *     VECTOR(3) per kept between edge;
 *   - initial values (initializeRandomly, :145-181): in first-appearance order over the kept unit edges, then the kept between
 *     edges, each key takes its given value or three draws of std::uniform_real_distribution<double>(-1, 1) from
 *     std::mt19937(seed); scale variables start at 1.  A FRESH generator is made per call: the reference's static generator
 *     gives this stream on its first call in a process and continues it on later ones.
 *   - no kept edge of either list: no factors, one origin value per set of the union-find (:216-223).
 * The result is a gsx_dataset, read with gsx_dataset_get and released with gsx_dataset_free; variables in ascending key order.  merged_keys /
 * merged_into (each with room for 2 n_unit entries, or NULL): every key of a merged set that is not its representative, and
 * that representative; *n_merged their number. */
gsx_status gsx_translation_recovery_problem(const gsx_translation_input* in, const gsx_translation_params* p, gsx_dataset** out,
                                            uint64_t* merged_keys, uint64_t* merged_into, int64_t* n_merged);
/* TranslationRecovery::run (:191-228): the description above on an ordinary handle, gsx_lm_optimize with p->lm, and the
 * values read back — no solver code of its own.  keys_out / translations_out (3 per key): the translation variables in
 * ascending key order followed by the merged keys, each with its representative's result (addSameTranslationNodes, :80-97);
 * room for 2 (n_unit + n_between) keys always suffices; *n_out their number.  r (may be NULL): the LM result; without a kept
 * edge no handle is created, no device is needed and r is zeroed. */
gsx_status gsx_translation_recovery(const gsx_translation_input* in, const gsx_translation_params* p, int32_t device,
                                    uint64_t* keys_out, double* translations_out, int64_t* n_out, gsx_lm_result* r);

/* ---- dense kernel exposed for unit parity (gtsam/base/cholesky.cpp:108-159) -- */
/* In-place partial Cholesky of an n x n column-major symmetric matrix (upper
 * triangle significant, like the reference): on return the first nfrontal rows
 * hold [R S], the trailing block holds C - S'S (upper).  *ok = 0 when the
 * reference would have reported failure. */
gsx_status gsx_cholesky_partial(double* abc, int32_t n, int32_t nfrontal, int32_t device,
                                int32_t* ok);

/* ---- stats / stream ---------------------------------------------------------- */
gsx_status gsx_get_stats(gsx_handle h, gsx_stats* out);
gsx_status gsx_reset_stats(gsx_handle h);
gsx_status gsx_synchronize(gsx_handle h);
/* level -1 (default): no timers — the ms_* / n_* fields of gsx_stats stay 0; level 0: HIP-event timers around the phases
 * (an event record costs ~5 us of stream time, ~70 us per LM iteration); level 1: additionally every factor_small /
 * factor_big launch (and one stream only).  bench.py times with -1 and reads the phase times from a level-0 pass. */
gsx_status gsx_set_profiling(gsx_handle h, int32_t level);
/* average duration (ms) of the named kernel class over launches since the last
 * gsx_reset_stats, measured with HIP events on the handle's stream; names:
 * "linearize", "assemble_hessian", "factor_leaf", "factor_small", "factor_big", "backsolve",
 * "linear_error", "retract", "error". *launches (may be NULL) = count. */
gsx_status gsx_kernel_time(gsx_handle h, const char* name, double* avg_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GSX_H_ */
