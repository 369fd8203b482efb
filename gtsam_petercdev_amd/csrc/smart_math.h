// smart_math.h — the arithmetic of ONE SmartProjectionPoseFactor<Cal3_S2> (smart.hip), on top of triangulate_math.h and, like
// it, compiled for the device and for a plain host program (tests/native/smart_native.cpp runs it on the CPU).
// Reference: gtsam/slam/SmartProjectionPoseFactor.h, SmartProjectionFactor.h, SmartFactorBase.h,
// gtsam/geometry/CalibratedCamera.cpp:27-46 (Dpose, Dpoint), Cal3_S2.cpp:54-62, Pose3.cpp:169-171 (equals).
// Matrices are row-major unless said otherwise.  Nothing here allocates; the loops over views and rows have compile-time
// bounds with a run-time guard, so that a device lane keeps its arrays in registers.
#pragma once
#include "triangulate_math.h"

namespace gsx {
namespace smart {

constexpr int kMaxViews = 8;              // the key limit of the assembly (GSX_F_LINEAR's)
constexpr int kMaxRows = 2 * kMaxViews;   // rows of [F b] before the landmark is marginalized
constexpr int kMaxCols = 6 * kMaxViews + 1;
// meas = (fx, fy, s, u0, v0, rank_tol, enable_epi, landmark_distance_threshold, dynamic_outlier_rejection_threshold,
//         retriangulation_threshold, degeneracy_mode) [+ body_P_sensor 12] + 2 nk pixels
enum { M_K = 0, M_RANK_TOL = 5, M_ENABLE_EPI = 6, M_LANDMARK_DISTANCE = 7, M_OUTLIER = 8, M_RETRIANGULATION = 9,
       M_DEGENERACY = 10, kHead = 11 };
enum { ZERO_ON_DEGENERACY = 1 };          // DegeneracyMode (SmartFactorParams.h): IGNORE 0, ZERO_ON 1, HANDLE_INFINITY 2
constexpr int kNever = -1;                // status of a factor that was never triangulated (an empty cache)

GSX_HD bool has_sensor(long long nmeas, int nk) { return nmeas == kHead + 12 + 2 * nk; }
GSX_HD const double* sensor_of(const double* meas, long long nmeas, int nk) { return has_sensor(nmeas, nk) ? meas + kHead : nullptr; }
GSX_HD const double* pixels_of(const double* meas, long long nmeas, int nk) { return meas + kHead + (has_sensor(nmeas, nk) ? 12 : 0); }

// SmartProjectionParams::triangulation handed to gtsam::triangulateSafe (SmartProjectionFactor.h:181-182): DLT, no noise model
GSX_HD void triangulation_params(const double* meas, trim::Params& P) {
  P.rank_tol = meas[M_RANK_TOL];
  P.optimize = meas[M_ENABLE_EPI] != 0.0;
  P.use_lost = 0;
  P.safe = 1;
  P.lost_sigma = 1e-4;
  P.landmark_distance_threshold = meas[M_LANDMARK_DISTANCE];
  P.outlier_threshold = meas[M_OUTLIER];
  P.noise.kind = trim::N_UNIT;
  for (int i = 0; i < 5; ++i) P.noise.p[i] = 0.0;
}

// the camera of one view: pose.compose(body_P_sensor) with the factor's calibration (SmartProjectionPoseFactor::cameras)
GSX_HD void view_camera(const double* pose, const double* meas, const double* sensor, trim::Camera& c) {
  double in[trim::kCameraInDoubles];
  for (int i = 0; i < 12; ++i) in[i] = pose[i];
  for (int i = 0; i < 5; ++i) in[12 + i] = meas[M_K + i];
  trim::prepare_camera(trim::CAM_POSE3, in, sensor, c);
}

// fpEqual(a, b, tol, false) (gtsam/base/Vector.cpp:42-77; its DOUBLE_MIN_NORMAL is 1 + the smallest normal = 1.0)
GSX_HD bool fp_equal(double a, double b, double tol) {
  if (isnan(a) || isnan(b)) return isnan(a) && isnan(b);
  if (isinf(a) || isinf(b)) return isinf(a) && isinf(b);
  return fabs(a - b) <= tol;
}
// Pose3::equals(pose, tol): every entry of R and of t.  cached: R 9, t 3
GSX_HD bool pose_equals(const trim::Camera& c, const double* cached, double tol) {
  bool eq = true;
  for (int i = 0; i < 9; ++i) eq = eq && fp_equal(c.R[i], cached[i], tol);
  for (int i = 0; i < 3; ++i) eq = eq && fp_equal(c.t[i], cached[9 + i], tol);
  return eq;
}
// decideIfTriangulate (SmartProjectionFactor.h:127-165): true = re-triangulate; the cache is then overwritten
GSX_HD bool decide_retriangulate(const trim::Camera* cams, int nk, double tol, int cached_status, double* cache) {
  bool retriangulate = cached_status == kNever;
  if (!retriangulate)
    for (int i = 0; i < nk; ++i)
      if (!pose_equals(cams[i], cache + 12 * i, tol)) {
        retriangulate = true;
        break;
      }
  if (retriangulate)
    for (int i = 0; i < nk; ++i) {
      for (int k = 0; k < 9; ++k) cache[12 * i + k] = cams[i].R[k];
      for (int k = 0; k < 3; ++k) cache[12 * i + 9 + k] = cams[i].t[k];
    }
  return retriangulate;
}

// gtsam::triangulateSafe on the factor's cameras; a factor of fewer than two views is DEGENERATE (:176-177)
GSX_HD int triangulate(const trim::Camera* cams, const double* z, int nk, const trim::Params& P, double* point) {
  const int32_t ident[kMaxViews] = {0, 1, 2, 3, 4, 5, 6, 7};
  int counts[2];
  return trim::triangulate_track(cams, ident, z, nk, P, point, counts);
}

// One view at the point p: e = h - z and, when F is given, F (2 x 6: PinholePose::project2's Dpose, times the compose
// Jacobian AdjointMap(body_P_sensor^-1) with a sensor, SmartFactorBase.h:221-237) and E (2 x 3: Dpoint), all unwhitened.
// false: the point is not in front of the camera (the reference throws CheiralityException).
GSX_HD bool view_eval(const trim::Camera& c, const double* sensor, const double* p, const double* z, double* e, double* F,
                      double* E) {
  const double dx = p[0] - c.t[0], dy = p[1] - c.t[1], dz = p[2] - c.t[2];
  const double qx = c.R[0] * dx + c.R[3] * dy + c.R[6] * dz;
  const double qy = c.R[1] * dx + c.R[4] * dy + c.R[7] * dz;
  const double qz = c.R[2] * dx + c.R[5] * dy + c.R[8] * dz;
  if (!(qz > 0.0)) return false;
  const double d = 1.0 / qz, u = qx * d, v = qy * d;
  const double fx = c.K[0], fy = c.K[1], s = c.K[2];
  e[0] = fx * u + s * v + c.K[3] - z[0];
  e[1] = fy * v + c.K[4] - z[1];
  if (!F) return true;
  // Dpn_pose (CalibratedCamera.cpp:27-34), then Dpi_pn = [fx s; 0 fy]
  const double r0[6] = {u * v, -1.0 - u * u, v, -d, 0.0, d * u};
  const double r1[6] = {1.0 + v * v, -u * v, -u, 0.0, -d, d * v};
  for (int k = 0; k < 6; ++k) {
    F[k] = fx * r0[k] + s * r1[k];
    F[6 + k] = fy * r1[k];
  }
  if (sensor)   // row h <- h AdjointMap(S^-1) = (R h_w + t x (R h_v), R h_v)
    for (int r = 0; r < 2; ++r) {
      double* h = F + 6 * r;
      double rv[3], rw[3];
      for (int i = 0; i < 3; ++i) {
        rv[i] = sensor[3 * i] * h[3] + sensor[3 * i + 1] * h[4] + sensor[3 * i + 2] * h[5];
        rw[i] = sensor[3 * i] * h[0] + sensor[3 * i + 1] * h[1] + sensor[3 * i + 2] * h[2];
      }
      const double* t = sensor + 9;
      h[0] = rw[0] + (t[1] * rv[2] - t[2] * rv[1]);
      h[1] = rw[1] + (t[2] * rv[0] - t[0] * rv[2]);
      h[2] = rw[2] + (t[0] * rv[1] - t[1] * rv[0]);
      h[3] = rv[0]; h[4] = rv[1]; h[5] = rv[2];
    }
  for (int j = 0; j < 3; ++j) {   // Dpn_point = d [R(:,0)' - u R(:,2)'; R(:,1)' - v R(:,2)'] (:37-46)
    const double a0 = d * (c.R[3 * j] - u * c.R[3 * j + 2]), a1 = d * (c.R[3 * j + 1] - v * c.R[3 * j + 2]);
    E[j] = fx * a0 + s * a1;
    E[3 + j] = fy * a1;
  }
  return true;
}

// The whitened E (2 nk x 3, rows beyond 2 nk zero) and column `col` of the whitened [F b] (2 nk rows): col < 6 nk is
// column col % 6 of view col / 6 (two non-zero rows), col == 6 nk is b = z - h.  Every column sees the same E, so a wave
// whose lanes each build one column runs this in lock step.  false: some view fails the cheirality test.
GSX_HD bool build_column(const trim::Camera* cams, const double* sensor, const double* z, int nk, const double* p,
                         double inv_sigma, int col, double* E, double* x) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < kMaxViews; ++i) {
    double e[2] = {0.0, 0.0}, F[12], Ei[6];
    for (int k = 0; k < 12; ++k) F[k] = 0.0;
    for (int k = 0; k < 6; ++k) Ei[k] = 0.0;
    if (i < nk) ok = view_eval(cams[i], sensor, p, z + 2 * i, e, F, Ei) && ok;
    double x0 = 0.0, x1 = 0.0;
    if (col == 6 * nk) { x0 = -e[0]; x1 = -e[1]; }
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (col == 6 * i + k) { x0 = F[k]; x1 = F[6 + k]; }
    const bool live = i < nk;
    x[2 * i] = live ? x0 * inv_sigma : 0.0;
    x[2 * i + 1] = live ? x1 * inv_sigma : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      E[6 * i + k] = live ? Ei[k] * inv_sigma : 0.0;
      E[6 * i + 3 + k] = live ? Ei[3 + k] * inv_sigma : 0.0;
    }
  }
  return ok;
}

// Three Householder reflectors of E (rows x 3): on return column k of E holds v_k in rows k .. rows - 1 and beta[k] =
// 2 / v_k'v_k (0: the column was already zero below and on the diagonal, the reflector is the identity).  Q = H_0 H_1 H_2;
// rows 3 .. rows - 1 of Q'[F b] are Q_2'[F b], Q_2 an orthonormal basis of the left null space of E.
GSX_HD void reflectors(double* E, int rows, double* beta) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double sigma = 0.0;
#pragma unroll
    for (int r = k + 1; r < kMaxRows; ++r)
      if (r < rows) sigma += E[3 * r + k] * E[3 * r + k];
    const double x0 = E[3 * k + k];
    const double norm = sqrt(x0 * x0 + sigma);
    const double alpha = x0 >= 0.0 ? -norm : norm;
    const double v0 = x0 - alpha;
    const double vtv = v0 * v0 + sigma;
    beta[k] = vtv > 0.0 ? 2.0 / vtv : 0.0;
    E[3 * k + k] = v0;
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int r = k; r < kMaxRows; ++r)
        if (r < rows) s += E[3 * r + k] * E[3 * r + j];
      s *= beta[k];
#pragma unroll
      for (int r = k; r < kMaxRows; ++r)
        if (r < rows) E[3 * r + j] -= s * E[3 * r + k];
    }
  }
}
// x <- Q'x for one column of `rows` entries
GSX_HD void apply_reflectors(const double* E, const double* beta, int rows, double* x) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
#pragma unroll
    for (int r = k; r < kMaxRows; ++r)
      if (r < rows) s += E[3 * r + k] * x[r];
    s *= beta[k];
#pragma unroll
    for (int r = k; r < kMaxRows; ++r)
      if (r < rows) x[r] -= s * E[3 * r + k];
  }
}

// Column `col` of the factor's [A b] = Q_2'[F b] (2 nk - 3 rows) at the point p into out[0 .. 2 nk - 3): what one lane of
// the linearize kernel computes.  false (out untouched): a view fails the cheirality test.
GSX_HD bool block_column(const trim::Camera* cams, const double* sensor, const double* z, int nk, const double* p,
                         double inv_sigma, int col, double* x) {
  double E[3 * kMaxRows], beta[3];
  if (!build_column(cams, sensor, z, nk, p, inv_sigma, col, E, x)) return false;
  reflectors(E, 2 * nk, beta);
  apply_reflectors(E, beta, 2 * nk, x);
  return true;
}

// totalReprojectionError (SmartFactorBase.h:301-306) at p: 0.5 |whitened (h - z)|^2 over all 2 nk rows.  A view that fails
// the cheirality test makes the factor count 0 (*ok = false).
GSX_HD double reprojection_error(const trim::Camera* cams, const double* z, int nk, const double* p, double inv_sigma,
                                 bool* ok) {
  double total = 0.0;
  *ok = true;
  for (int i = 0; i < nk; ++i) {
    double e[2];
    if (!view_eval(cams[i], nullptr, p, z + 2 * i, e, nullptr, nullptr)) {
      *ok = false;
      return 0.0;
    }
    total += (e[0] * inv_sigma) * (e[0] * inv_sigma) + (e[1] * inv_sigma) * (e[1] * inv_sigma);
  }
  return 0.5 * total;
}

}  // namespace smart
}  // namespace gsx
