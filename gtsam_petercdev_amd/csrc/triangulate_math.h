// triangulate_math.h — everything that is arithmetic on ONE track of the batched triangulation (triangulate.hip), written
// so that the very same functions compile for the device and for a plain host program (tests/native/triangulate_native.cpp
// runs them on the CPU).  Reference: gtsam/geometry/triangulation.{h,cpp}, gtsam/slam/TriangulationFactor.h,
// gtsam/geometry/Cal3Bundler.cpp, gtsam/base/Matrix.cpp:556-574 (DLT), gtsam/nonlinear/LevenbergMarquardtOptimizer.cpp.
// Matrices are row-major.  No function here allocates, and none indexes a local array by a run-time value.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef GSX_HD
#define GSX_HD __host__ __device__ inline
#endif
#else
#ifndef GSX_HD
#define GSX_HD inline
#endif
#endif

namespace gsx {
namespace trim {

// TriangulationResult::Status (triangulation.h:644) + the Cal3Bundler::calibrate failure (Cal3Bundler.cpp:120-123)
enum { ST_VALID = 0, ST_DEGENERATE = 1, ST_BEHIND_CAMERA = 2, ST_OUTLIER = 3, ST_FAR_POINT = 4, ST_CALIBRATION_FAILED = 5 };
enum { CAM_POSE3 = 0, CAM_BUNDLER = 1 };
// noise kinds: the values of include/gsx.h (GSX_NOISE_*), restated so that the header stands alone
enum { N_UNIT = 0, N_ISOTROPIC = 1, N_DIAGONAL = 2, N_GAUSSIAN = 3, N_BASE_MASK = 15 };

constexpr int kCameraInDoubles = 17;   // R 9, t 3, then (fx, fy, s, u0, v0) or (f, k1, k2, u0, v0)
constexpr int kCameraDoubles = 32;     // the prepared record below, padded to 256 B

// A prepared camera: P = K [R' | -R' t] (cameraProjectionMatrix, PinholeCamera.h:316-318), the pose wTc, the pinhole part
// of the calibration (createPinholeCalibration, triangulation.h:252-256) and the radial terms (0 for Cal3_S2).
struct Camera {
  double P[12];
  double R[9];
  double t[3];
  double K[5];   // fx, fy, s, u0, v0
  double k1, k2;
  double pad;
};

struct Noise {
  int kind;        // GSX_NOISE_* of dimension 2, robust bits included
  double p[5];     // sigma | sigmas 2 | R 4 (upper triangular, row-major), then the robust parameter
};

struct Params {
  double rank_tol;
  int optimize, use_lost, safe;
  double lost_sigma;                 // mean of the model's sigmas, 1e-4 without a model (triangulation.h:439)
  double landmark_distance_threshold, outlier_threshold;   // <= 0: off
  Noise noise;
};

// ---- camera preparation ----------------------------------------------------------------------------------------------
// in: kCameraInDoubles; sensor: body_P_sensor as a Pose3 state (R 9, t 3) or NULL — the camera sits at pose.compose(sensor)
GSX_HD void prepare_camera(int kind, const double* in, const double* sensor, Camera& c) {
  if (sensor) {   // Pose3::compose: R = Ra Rb, t = ta + Ra tb
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j)
        c.R[3 * i + j] = in[3 * i] * sensor[j] + in[3 * i + 1] * sensor[3 + j] + in[3 * i + 2] * sensor[6 + j];
      c.t[i] = in[9 + i] + in[3 * i] * sensor[9] + in[3 * i + 1] * sensor[10] + in[3 * i + 2] * sensor[11];
    }
  } else {
    for (int i = 0; i < 9; ++i) c.R[i] = in[i];
    for (int i = 0; i < 3; ++i) c.t[i] = in[9 + i];
  }
  if (kind == CAM_BUNDLER) {   // Cal3Bundler::K(): [f 0 u0; 0 f v0; 0 0 1]
    c.K[0] = in[12]; c.K[1] = in[12]; c.K[2] = 0.0; c.K[3] = in[15]; c.K[4] = in[16];
    c.k1 = in[13]; c.k2 = in[14];
  } else {
    for (int i = 0; i < 5; ++i) c.K[i] = in[12 + i];
    c.k1 = 0.0; c.k2 = 0.0;
  }
  c.pad = 0.0;
  // E = [R' | -R' t] (Pose3::inverse), P = K E
  double E[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) E[4 * i + j] = c.R[3 * j + i];
    E[4 * i + 3] = -(c.R[i] * c.t[0] + c.R[3 + i] * c.t[1] + c.R[6 + i] * c.t[2]);
  }
  for (int j = 0; j < 4; ++j) {
    c.P[j] = c.K[0] * E[j] + c.K[2] * E[4 + j] + c.K[3] * E[8 + j];
    c.P[4 + j] = c.K[1] * E[4 + j] + c.K[4] * E[8 + j];
    c.P[8 + j] = E[8 + j];
  }
}

// uncalibrate of the camera's full model on intrinsic coordinates (Cal3Bundler.cpp:64-90, Cal3_S2.cpp:54-62); Dp 2x2 or NULL
GSX_HD void uncalibrate(const Camera& c, double x, double y, double* pi, double* Dp) {
  const double r = x * x + y * y;
  const double g = 1. + (c.k1 + c.k2 * r) * r;
  const double u = g * x, v = g * y;
  pi[0] = c.K[0] * u + c.K[2] * v + c.K[3];
  pi[1] = c.K[1] * v + c.K[4];
  if (Dp) {
    const double a = 2. * (c.k1 + 2. * c.k2 * r);
    const double d00 = g + a * x * x, d01 = a * x * y, d11 = g + a * y * y;
    Dp[0] = c.K[0] * d00 + c.K[2] * d01; Dp[1] = c.K[0] * d01 + c.K[2] * d11;
    Dp[2] = c.K[1] * d01;                Dp[3] = c.K[1] * d11;
  }
}

// calibrate: pixel -> intrinsic coordinates.  Cal3_S2::calibrate (Cal3_S2.cpp:64-75) when there is no distortion, else
// Cal3Bundler::calibrate's fixed-point loop (Cal3Bundler.cpp:93-128): at most 10 rounds, tol_ = 1e-5 on the pixel distance.
// Returns false where the reference throws "fails to converge".
GSX_HD bool calibrate(const Camera& c, const double* z, double* pn) {
  const double inv_fy_dv = (z[1] - c.K[4]) / c.K[1];
  const double px0 = (z[0] - c.K[3] - c.K[2] * inv_fy_dv) / c.K[0], py0 = inv_fy_dv;
  if (c.k1 == 0.0 && c.k2 == 0.0) {
    pn[0] = px0; pn[1] = py0;
    return true;
  }
  double px = px0, py = py0;
  for (int iteration = 0; iteration < 10; ++iteration) {
    const double rr = px * px + py * py;
    const double g = 1 + c.k1 * rr + c.k2 * rr * rr;
    pn[0] = px0 / g; pn[1] = py0 / g;
    double pi[2];
    uncalibrate(c, pn[0], pn[1], pi, nullptr);
    const double dx = pi[0] - z[0], dy = pi[1] - z[1];
    if (sqrt(dx * dx + dy * dy) <= 1e-5) return true;
    px = pn[0]; py = pn[1];
  }
  return false;
}

// transformTo(point).z (Pose3.cpp:380-397)
GSX_HD double depth(const Camera& c, const double* p) {
  return c.R[2] * (p[0] - c.t[0]) + c.R[5] * (p[1] - c.t[1]) + c.R[8] * (p[2] - c.t[2]);
}

// PinholeCamera::project2(point, {}, Dpoint) (CalibratedCamera.cpp:27-46,116-135 + uncalibrate).  false on cheirality
// (z <= 0; the oracle is built with GTSAM_THROW_CHEIRALITY_EXCEPTION).  H 2x3 or NULL.
GSX_HD bool project(const Camera& c, const double* p, double* pi, double* H) {
  const double dx = p[0] - c.t[0], dy = p[1] - c.t[1], dz = p[2] - c.t[2];
  const double qx = c.R[0] * dx + c.R[3] * dy + c.R[6] * dz;
  const double qy = c.R[1] * dx + c.R[4] * dy + c.R[7] * dz;
  const double qz = c.R[2] * dx + c.R[5] * dy + c.R[8] * dz;
  if (!(qz > 0.0)) return false;
  const double d = 1.0 / qz, u = qx * d, v = qy * d;
  double Dp[4];
  uncalibrate(c, u, v, pi, H ? Dp : nullptr);
  if (H) {
    // Dpn_point = d [R0' - u R2' ; R1' - v R2'] with Rk' = column k of R (Dpoint, CalibratedCamera.cpp:41-46)
    for (int j = 0; j < 3; ++j) {
      const double a0 = d * (c.R[3 * j] - u * c.R[3 * j + 2]), a1 = d * (c.R[3 * j + 1] - v * c.R[3 * j + 2]);
      H[j] = Dp[0] * a0 + Dp[1] * a1;
      H[3 + j] = Dp[2] * a0 + Dp[3] * a1;
    }
  }
  return true;
}

// ---- the streaming triangular factor -------------------------------------------------------------------------------------
// T holds the upper triangle of a 4 x 4 R, row by row: (0,0..3) (1,1..3) (2,2..3) (3,3).  For DLT it is the R of A (2m x 4);
// for LOST that of [A b] (2m x 3 | 1): its leading 3 x 3 is the R of A, its last column Q'b.
GSX_HD constexpr int tri(int i, int j) { return 4 * i - (i * (i - 1)) / 2 + (j - i); }

GSX_HD void tri_zero(double* T) {
  for (int i = 0; i < 10; ++i) T[i] = 0.0;
}

// one row into R by 4 Givens rotations (the row is destroyed); `first` = leading entries of the row known to be zero
GSX_HD void tri_insert(double* T, double* row, int first = 0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    if (k < first) continue;
    const double a = T[tri(k, k)], b = row[k];
    if (b == 0.0) continue;
    const double r = sqrt(a * a + b * b);
    const double cs = a / r, sn = b / r;
    T[tri(k, k)] = r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = k + 1; j < 4; ++j) {
      const double tj = T[tri(k, j)], rj = row[j];
      T[tri(k, j)] = cs * tj + sn * rj;
      row[j] = cs * rj - sn * tj;
    }
  }
}

// TSQR merge: stack another triangle under this one and re-triangularise
GSX_HD void tri_merge(double* T, const double* other) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 4; ++i) {
    double row[4] = {0.0, 0.0, 0.0, 0.0};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = i; j < 4; ++j) row[j] = other[tri(i, j)];
    tri_insert(T, row, i);
  }
}

// the two DLT rows of one observation: p.x P2 - P0, p.y P2 - P1 on the undistorted measurement (triangulation.cpp:48-49,
// undistortMeasurementInternal triangulation.h:260-268).  rows: 2 x 4.  Returns ST_VALID or ST_CALIBRATION_FAILED.
GSX_HD int dlt_rows(const Camera& c, const double* z, double* rows) {
  double u = z[0], v = z[1];
  if (c.k1 != 0.0 || c.k2 != 0.0) {
    double pn[2];
    if (!calibrate(c, z, pn)) return ST_CALIBRATION_FAILED;
    u = c.K[0] * pn[0] + c.K[2] * pn[1] + c.K[3];   // Cal3_S2::uncalibrate of the pinhole part
    v = c.K[1] * pn[1] + c.K[4];
  }
  for (int j = 0; j < 4; ++j) {
    rows[j] = u * c.P[8 + j] - c.P[j];
    rows[4 + j] = v * c.P[8 + j] - c.P[4 + j];
  }
  return ST_VALID;
}

GSX_HD void rotate(const Camera& c, const double* v, double* out) {
  for (int i = 0; i < 3; ++i) out[i] = c.R[3 * i] * v[0] + c.R[3 * i + 1] * v[1] + c.R[3 * i + 2] * v[2];
}
GSX_HD double cross_norm(const double* a, const double* b) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  return sqrt(x * x + y * y + z * z);
}

// the two LOST rows [A | b] of observation i of a track (triangulation.cpp:97-139): partner j = (i + 1) % m, and the search
// over k = 2 .. m - 1 when num_i == 0 || den_i == 0.  cams: the camera table; oc / oz: the track's camera indices / pixels.
// Returns ST_VALID, ST_DEGENERATE (no usable partner) or ST_CALIBRATION_FAILED.
GSX_HD int lost_rows(const Camera* cams, const int32_t* oc, const double* oz, int m, int i, double sigma, double* rows) {
  const Camera& ci = cams[oc[i]];
  double zi[3], zj[3];
  zi[2] = 1.0; zj[2] = 1.0;
  if (!calibrate(ci, oz + 2 * i, zi)) return ST_CALIBRATION_FAILED;
  double wZi[3], wZj[3], d_ij[3];
  rotate(ci, zi, wZi);
  double num_i = 0.0, den_i = 0.0;
  bool success = false;
  for (int k = 1; k < m; ++k) {
    const int j = (i + k) % m;
    const Camera& cj = cams[oc[j]];
    if (!calibrate(cj, oz + 2 * j, zj)) return ST_CALIBRATION_FAILED;
    for (int a = 0; a < 3; ++a) d_ij[a] = cj.t[a] - ci.t[a];
    rotate(cj, zj, wZj);
    num_i = cross_norm(wZi, wZj);
    den_i = cross_norm(d_ij, wZj);
    // the first partner is taken unless num == 0 || den == 0 (:112); the search wants both > 0 (:122)
    if (k == 1 ? !(num_i == 0 || den_i == 0) : (num_i > 0 && den_i > 0)) {
      success = true;
      break;
    }
  }
  if (!success) return ST_DEGENERATE;
  const double q = num_i / (sigma * den_i);
  // q [0 -1 y; 1 0 -x] R'   (skewSymmetric(z).topLeftCorner(2, 3) with z = (x, y, 1))
  double b0 = 0.0, b1 = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double r0 = ci.R[3 * a], r1 = ci.R[3 * a + 1], r2 = ci.R[3 * a + 2];   // row a of R = column a of R'
    rows[a] = q * (-r1 + zi[1] * r2);
    rows[4 + a] = q * (r0 - zi[0] * r2);
    b0 += rows[a] * ci.t[a];
    b1 += rows[4 + a] * ci.t[a];
  }
  rows[3] = b0;
  rows[7] = b1;
  return ST_VALID;
}

// ---- DLT: one-sided Jacobi SVD of the 4 x 4 triangle --------------------------------------------------------------------------
// Its singular values and right singular vectors are A's.  rank = singular values above rank_tol, absolute (Matrix.cpp:
// 566-569); the point is v[0:3] / v[3] of the right vector of the smallest one (triangulation.cpp:153-156).  sv (may be NULL):
// the four singular values, unsorted.
GSX_HD int dlt_finish(const double* T, double rank_tol, double* point, double* sv) {
  double G[16], V[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      G[4 * i + j] = j >= i ? T[tri(i, j)] : 0.0;
      V[4 * i + j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int p = 0; p < 3; ++p) {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < 4; ++i) {
          alpha += G[4 * i + p] * G[4 * i + p];
          beta += G[4 * i + q] * G[4 * i + q];
          gamma += G[4 * i + p] * G[4 * i + q];
        }
        if (gamma == 0.0 || fabs(gamma) <= 1.1102230246251565e-16 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < 4; ++i) {
          const double gp = G[4 * i + p], gq = G[4 * i + q];
          G[4 * i + p] = cs * gp - sn * gq;
          G[4 * i + q] = sn * gp + cs * gq;
          const double vp = V[4 * i + p], vq = V[4 * i + q];
          V[4 * i + p] = cs * vp - sn * vq;
          V[4 * i + q] = sn * vp + cs * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double s[4];
  for (int j = 0; j < 4; ++j) {
    double n = 0;
    for (int i = 0; i < 4; ++i) n += G[4 * i + j] * G[4 * i + j];
    s[j] = sqrt(n);
  }
  int rank = 0;
  for (int j = 0; j < 4; ++j) rank += s[j] > rank_tol ? 1 : 0;
  if (sv)
    for (int j = 0; j < 4; ++j) sv[j] = s[j];
  if (rank < 3) return ST_DEGENERATE;
  // the column of the smallest singular value, chosen by selects (no run-time index)
  double smin = s[0], v0 = V[0], v1 = V[4], v2 = V[8], v3 = V[12];
  for (int j = 1; j < 4; ++j) {
    const bool less = s[j] < smin;
    smin = less ? s[j] : smin;
    v0 = less ? V[j] : v0;
    v1 = less ? V[4 + j] : v1;
    v2 = less ? V[8 + j] : v2;
    v3 = less ? V[12 + j] : v3;
  }
  point[0] = v0 / v3; point[1] = v1 / v3; point[2] = v2 / v3;
  return ST_VALID;
}

// ---- LOST: column-pivoted QR of the leading 3 x 3 of the triangle, right-hand side carried along ---------------------------------
// ColPivHouseholderQR's rank rule (Eigen: pivots above threshold x the largest pivot, setThreshold(rank_tol),
// triangulation.cpp:141-146): relative.  The column-pivoted factorisation of R has the pivots of that of A.
// pivots (may be NULL): the three |pivots|.
GSX_HD int lost_finish(const double* T, double rank_tol, double* point, double* pivots) {
  // columns as separate scalars so that swaps are selects
  double c0[3] = {T[tri(0, 0)], 0.0, 0.0}, c1[3] = {T[tri(0, 1)], T[tri(1, 1)], 0.0},
         c2[3] = {T[tri(0, 2)], T[tri(1, 2)], T[tri(2, 2)]}, d[3] = {T[tri(0, 3)], T[tri(1, 3)], T[tri(2, 3)]};
  int i0 = 0, i1 = 1, i2 = 2;   // the original column held by c0 / c1 / c2
#define GSX_SWAP_COL(A, B, IA, IB)             \
  do {                                         \
    for (int r_ = 0; r_ < 3; ++r_) {           \
      const double t_ = A[r_];                 \
      A[r_] = B[r_];                           \
      B[r_] = t_;                              \
    }                                          \
    const int ti_ = IA;                        \
    IA = IB;                                   \
    IB = ti_;                                  \
  } while (0)
  // rotate rows (a, b) so that column C's entry b vanishes
#define GSX_ROW_GIVENS(C, a, b)                                  \
  do {                                                           \
    const double x_ = C[a], y_ = C[b];                           \
    if (y_ != 0.0) {                                             \
      const double r_ = sqrt(x_ * x_ + y_ * y_), cs_ = x_ / r_, sn_ = y_ / r_; \
      double u_, w_;                                             \
      u_ = c0[a]; w_ = c0[b]; c0[a] = cs_ * u_ + sn_ * w_; c0[b] = cs_ * w_ - sn_ * u_; \
      u_ = c1[a]; w_ = c1[b]; c1[a] = cs_ * u_ + sn_ * w_; c1[b] = cs_ * w_ - sn_ * u_; \
      u_ = c2[a]; w_ = c2[b]; c2[a] = cs_ * u_ + sn_ * w_; c2[b] = cs_ * w_ - sn_ * u_; \
      u_ = d[a];  w_ = d[b];  d[a] = cs_ * u_ + sn_ * w_;  d[b] = cs_ * w_ - sn_ * u_;  \
    }                                                            \
  } while (0)
  double n0 = c0[0] * c0[0], n1 = c1[0] * c1[0] + c1[1] * c1[1], n2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
  if (n1 > n0 && n1 >= n2) GSX_SWAP_COL(c0, c1, i0, i1);
  else if (n2 > n0 && n2 > n1) GSX_SWAP_COL(c0, c2, i0, i2);
  GSX_ROW_GIVENS(c0, 1, 2);
  GSX_ROW_GIVENS(c0, 0, 1);
  n1 = c1[1] * c1[1] + c1[2] * c1[2];
  n2 = c2[1] * c2[1] + c2[2] * c2[2];
  if (n2 > n1) GSX_SWAP_COL(c1, c2, i1, i2);
  GSX_ROW_GIVENS(c1, 1, 2);
#undef GSX_SWAP_COL
#undef GSX_ROW_GIVENS
  const double p0 = fabs(c0[0]), p1 = fabs(c1[1]), p2 = fabs(c2[2]);
  if (pivots) { pivots[0] = p0; pivots[1] = p1; pivots[2] = p2; }
  const double pmax = fmax(p0, fmax(p1, p2));
  const int rank = (p0 > rank_tol * pmax ? 1 : 0) + (p1 > rank_tol * pmax ? 1 : 0) + (p2 > rank_tol * pmax ? 1 : 0);
  if (rank < 3) return ST_DEGENERATE;
  const double y2 = d[2] / c2[2];
  const double y1 = (d[1] - c2[1] * y2) / c1[1];
  const double y0 = (d[0] - c1[0] * y1 - c2[0] * y2) / c0[0];
  // x[perm] = y, by selects
  point[0] = i0 == 0 ? y0 : (i1 == 0 ? y1 : y2);
  point[1] = i0 == 1 ? y0 : (i1 == 1 ? y1 : y2);
  point[2] = i0 == 2 ? y0 : (i1 == 2 ? y1 : y2);
  return ST_VALID;
}

// ---- noise (gtsam/linear/NoiseModel.cpp, LossFunctions.cpp) ---------------------------------------------------------------------
GSX_HD int noise_base_params(int base) { return base == N_UNIT ? 0 : (base == N_ISOTROPIC ? 1 : (base == N_DIAGONAL ? 2 : 4)); }
GSX_HD double robust_weight(int loss, double k, double dist) {   // LossFunctions.cpp:179-191, 250-267, 217-224
  const double a = fabs(dist);
  if (loss == 1) return (a <= k) ? 1.0 : k / a;
  if (loss == 2) {
    if (a > k) return 0.0;
    const double t = 1.0 - dist * dist / (k * k);
    return t * t;
  }
  return (k * k) / (k * k + dist * dist);
}
GSX_HD double robust_loss(int loss, double k, double dist) {
  const double a = fabs(dist);
  if (loss == 1) return (a <= k) ? dist * dist / 2 : k * (a - k / 2);
  if (loss == 2) {
    if (a > k) return k * k / 6.0;
    const double t = 1.0 - dist * dist / (k * k);
    return k * k * (1 - t * t * t) / 6.0;
  }
  return k * k * log1p(dist * dist / (k * k)) * 0.5;
}
// whiten a 2-vector or the 2 rows of a 2 x 3 matrix in place with the base model
GSX_HD void whiten2(const Noise& n, double& a, double& b) {
  const int base = n.kind & N_BASE_MASK;
  if (base == N_ISOTROPIC) { a /= n.p[0]; b /= n.p[0]; }
  else if (base == N_DIAGONAL) { a /= n.p[0]; b /= n.p[1]; }
  else if (base == N_GAUSSIAN) { a = n.p[0] * a + n.p[1] * b; b = n.p[3] * b; }
}

// error vector h(x) - z and Jacobian of one TriangulationFactor (TriangulationFactor.h:122-136): behind the camera the
// Jacobian is zero and the error 2 fx (1, 1)
GSX_HD void factor_eval(const Camera& c, const double* z, const double* p, double* e, double* H) {
  double pi[2];
  if (project(c, p, pi, H)) {
    e[0] = pi[0] - z[0]; e[1] = pi[1] - z[1];
  } else {
    e[0] = 2.0 * c.K[0]; e[1] = 2.0 * c.K[0];
    if (H)
      for (int i = 0; i < 6; ++i) H[i] = 0.0;
  }
}

// NonlinearFactorGraph::error of the track at p: sum of 0.5 |whitened e|^2, or of loss(|whitened e|) under a robust model
GSX_HD double track_error(const Camera* cams, const int32_t* oc, const double* oz, int m, const Noise& n, const double* p) {
  const int loss = n.kind >> 4;
  const double k = n.p[noise_base_params(n.kind & N_BASE_MASK)];
  double total = 0.0;
  for (int i = 0; i < m; ++i) {
    double e[2];
    factor_eval(cams[oc[i]], oz + 2 * i, p, e, nullptr);
    whiten2(n, e[0], e[1]);
    const double sq = e[0] * e[0] + e[1] * e[1];
    total += loss ? robust_loss(loss, k, sqrt(sq)) : 0.5 * sq;
  }
  return total;
}

// 3 x 3 Cholesky solve of (H + lambda I) x = g; H as (00, 01, 02, 11, 12, 22).  false when not positive definite.
GSX_HD bool solve_damped3(const double* H, double lambda, const double* g, double* x) {
  const double a00 = H[0] + lambda, a01 = H[1], a02 = H[2], a11 = H[3] + lambda, a12 = H[4], a22 = H[5] + lambda;
  if (!(a00 > 0.0)) return false;
  const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
  const double s11 = a11 - l10 * l10;
  if (!(s11 > 0.0)) return false;
  const double l11 = sqrt(s11), l21 = (a12 - l20 * l10) / l11;
  const double s22 = a22 - l20 * l20 - l21 * l21;
  if (!(s22 > 0.0)) return false;
  const double l22 = sqrt(s22);
  const double y0 = g[0] / l00, y1 = (g[1] - l10 * y0) / l11, y2 = (g[2] - l20 * y0 - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
  return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// checkConvergence (NonlinearOptimizer.cpp:182-231) with relativeErrorTol 1e-5, absoluteErrorTol 1.0, errorTol 0
GSX_HD bool check_convergence(double current_error, double new_error) {
  if (new_error <= 0.0) return true;
  const double absolute_decrease = current_error - new_error;
  const double relative_decrease = absolute_decrease / current_error;
  return relative_decrease <= 1e-5 || absolute_decrease <= 1.0;
}

// triangulateNonlinear -> optimize (triangulation.cpp:177-195): LM on one Point3 with lambdaInitial 1, lambdaFactor 10,
// maxIterations 100, absoluteErrorTol 1.0, relativeErrorTol 1e-5, errorTol 0, lambdaUpperBound 1e5, lambdaLowerBound 0,
// minModelFidelity 1e-3, fixed lambda schedule, no diagonal damping.  The trial decisions are those of csrc/lm_policy.cpp
// (gsx_lm_decide) restated for one 3 x 3 system; the outer loop is NonlinearOptimizer::defaultOptimize (:62-117).
// counts[0] = outer (accepted) iterations, counts[1] = trials that changed the controller.
GSX_HD void refine(const Camera* cams, const int32_t* oc, const double* oz, int m, const Noise& n, double* p, int* counts) {
  const int loss = n.kind >> 4;
  const double rk = n.p[noise_base_params(n.kind & N_BASE_MASK)];
  double lambda = 1.0;
  const double factor = 10.0;
  int iterations = 0, trials = 0;
  double cost = track_error(cams, oc, oz, m, n, p);
  counts[0] = 0; counts[1] = 0;
  if (cost <= 0.0) return;
  double new_error = cost, current_error;
  do {
    current_error = new_error;
    // linearize: A = whitened H, b = -whitened e, both scaled by sqrt(weight(|b|)) under a robust model
    double Hs[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, f0 = 0.0;
    for (int i = 0; i < m; ++i) {
      double e[2], J[6];
      factor_eval(cams[oc[i]], oz + 2 * i, p, e, J);
      double b0 = -e[0], b1 = -e[1];
      whiten2(n, b0, b1);
      whiten2(n, J[0], J[3]); whiten2(n, J[1], J[4]); whiten2(n, J[2], J[5]);
      if (loss) {
        const double w = sqrt(robust_weight(loss, rk, sqrt(b0 * b0 + b1 * b1)));
        b0 *= w; b1 *= w;
        for (int a = 0; a < 6; ++a) J[a] *= w;
      }
      Hs[0] += J[0] * J[0] + J[3] * J[3]; Hs[1] += J[0] * J[1] + J[3] * J[4]; Hs[2] += J[0] * J[2] + J[3] * J[5];
      Hs[3] += J[1] * J[1] + J[4] * J[4]; Hs[4] += J[1] * J[2] + J[4] * J[5]; Hs[5] += J[2] * J[2] + J[5] * J[5];
      g[0] += J[0] * b0 + J[3] * b1; g[1] += J[1] * b0 + J[4] * b1; g[2] += J[2] * b0 + J[5] * b1;
      f0 += 0.5 * (b0 * b0 + b1 * b1);
    }
    // iterate(): keep increasing lambda until a trial ends the search
    for (;;) {
      double dx[3];
      const bool solved = solve_damped3(Hs, lambda, g, dx);
      bool take = false, settle = false;
      double trial[3] = {p[0], p[1], p[2]}, trial_cost = cost;
      if (solved) {
        const double Hd0 = Hs[0] * dx[0] + Hs[1] * dx[1] + Hs[2] * dx[2], Hd1 = Hs[1] * dx[0] + Hs[3] * dx[1] + Hs[4] * dx[2],
                     Hd2 = Hs[2] * dx[0] + Hs[4] * dx[1] + Hs[5] * dx[2];
        // model(0) - model(dx) on the undamped system = g.dx - dx'H dx / 2
        const double predicted = (g[0] * dx[0] + g[1] * dx[1] + g[2] * dx[2]) - 0.5 * (dx[0] * Hd0 + dx[1] * Hd1 + dx[2] * Hd2);
        if (predicted >= 0.0) {
          for (int a = 0; a < 3; ++a) trial[a] = p[a] + dx[a];
          trial_cost = track_error(cams, oc, oz, m, n, trial);
          const double cost_change = cost - trial_cost;
          if (predicted > 2.220446049250313e-16 * f0) take = cost_change / predicted > 1e-3;
          settle = fabs(cost_change) < 1e-5 * cost;
        }
      }
      if (take) {
        lambda = fmax(0.0, lambda / factor);
        for (int a = 0; a < 3; ++a) p[a] = trial[a];
        cost = trial_cost;
        ++iterations; ++trials;
        break;
      }
      if (settle) break;
      lambda *= factor;
      ++trials;
      if (lambda >= 1e5) break;   // giving up: cannot decrease the error with maximum lambda
    }
    new_error = cost;
  } while (iterations < 100 && !check_convergence(current_error, new_error) && isfinite(current_error));
  counts[0] = iterations; counts[1] = trials;
}

// ---- the checks, in the reference's order ----------------------------------------------------------------------------------------
// triangulatePoint3's cheirality loop (triangulation.h:540-546), then with safe != 0 triangulateSafe's loop (:719-745)
GSX_HD int check_point(const Camera* cams, const int32_t* oc, const double* oz, int m, const Params& P, const double* p) {
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return ST_DEGENERATE;   // v[3] == 0: a point at infinity
  for (int i = 0; i < m; ++i)
    if (depth(cams[oc[i]], p) <= 0) return ST_BEHIND_CAMERA;
  if (!P.safe) return ST_VALID;
  double max_reproj = 0.0;
  for (int i = 0; i < m; ++i) {
    const Camera& c = cams[oc[i]];
    if (P.landmark_distance_threshold > 0) {
      const double dx = p[0] - c.t[0], dy = p[1] - c.t[1], dz = p[2] - c.t[2];
      if (sqrt(dx * dx + dy * dy + dz * dz) > P.landmark_distance_threshold) return ST_FAR_POINT;
    }
    if (P.outlier_threshold > 0) {
      double pi[2];
      if (project(c, p, pi, nullptr)) {
        const double ex = pi[0] - oz[2 * i], ey = pi[1] - oz[2 * i + 1];
        max_reproj = fmax(max_reproj, sqrt(ex * ex + ey * ey));
      }
    }
  }
  if (P.outlier_threshold > 0 && max_reproj > P.outlier_threshold) return ST_OUTLIER;
  return ST_VALID;
}

// after the linear stage: refinement, checks, NaN in a point that is not VALID
GSX_HD int finish_track(const Camera* cams, const int32_t* oc, const double* oz, int m, const Params& P, int status,
                        double* point, int* counts) {
  counts[0] = 0; counts[1] = 0;
  if (status == ST_VALID && !(isfinite(point[0]) && isfinite(point[1]) && isfinite(point[2]))) status = ST_DEGENERATE;
  if (status == ST_VALID && P.optimize) refine(cams, oc, oz, m, P.noise, point, counts);
  if (status == ST_VALID) status = check_point(cams, oc, oz, m, P, point);
  if (status != ST_VALID) point[0] = point[1] = point[2] = NAN;
  return status;
}

// the rows of observation i into the triangle; returns the row status
GSX_HD int accumulate_observation(const Camera* cams, const int32_t* oc, const double* oz, int m, int i, const Params& P,
                                  double* T) {
  double rows[8];
  const int st = P.use_lost ? lost_rows(cams, oc, oz, m, i, P.lost_sigma, rows) : dlt_rows(cams[oc[i]], oz + 2 * i, rows);
  if (st != ST_VALID) return st;
  tri_insert(T, rows);
  tri_insert(T, rows + 4);
  return ST_VALID;
}

GSX_HD int linear_finish(const double* T, const Params& P, double* point) {
  return P.use_lost ? lost_finish(T, P.rank_tol, point, nullptr) : dlt_finish(T, P.rank_tol, point, nullptr);
}

// one whole track, serially: what one lane of the short-track kernel and the host program run.  oc / oz point at the track's
// first observation.  A calibration failure outranks an underconstrained system (the reference calibrates every
// measurement before it builds the system).
GSX_HD int triangulate_track(const Camera* cams, const int32_t* oc, const double* oz, int m, const Params& P, double* point,
                             int* counts) {
  counts[0] = 0; counts[1] = 0;
  point[0] = point[1] = point[2] = NAN;
  if (m < 2) return ST_DEGENERATE;
  double T[10];
  tri_zero(T);
  int status = ST_VALID;
  for (int i = 0; i < m; ++i) {
    const int st = accumulate_observation(cams, oc, oz, m, i, P, T);
    status = st > status ? st : status;
  }
  if (status == ST_VALID) status = linear_finish(T, P, point);
  return finish_track(cams, oc, oz, m, P, status, point, counts);
}

}  // namespace trim
}  // namespace gsx
