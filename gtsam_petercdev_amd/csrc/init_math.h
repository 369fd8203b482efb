// init_math.h — the per-rotation arithmetic of the Pose3 initializer (initialize.hip), written so that the very same
// functions compile for the device and for a plain host program (tests/native/init_sanitize.cpp runs them on the CPU).
// 3 x 3 matrices are double[9], row-major.  Reference: gtsam/slam/InitializePose3.cpp, gtsam/geometry/SO3.cpp.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GSX_HD __host__ __device__ inline
#else
#define GSX_HD inline
#endif

namespace gsx {
namespace initm {

GSX_HD void mat_mul(const double* A, const double* B, double* C) {          // C = A B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
GSX_HD void mat_tmul(const double* A, const double* B, double* C) {         // C = A' B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
GSX_HD void mat_transpose(const double* A, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * j + i];
}
GSX_HD void mat_identity(double* C) {
  for (int i = 0; i < 9; ++i) C[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// SO3::Expmap — ExpmapFunctor (gtsam/geometry/SO3.cpp:61-95): I + A W + B W W, Taylor branch at theta^2 <= eps
GSX_HD void so3_exp(const double* w, double* R) {
  const double x = w[0], y = w[1], z = w[2];
  const double theta2 = x * x + y * y + z * z;
  double A, B;
  if (theta2 <= 2.220446049250313e-16) {
    A = 1.0 - theta2 * (1.0 / 6.0);
    B = 0.5 - theta2 * (1.0 / 24.0);
  } else {
    const double theta = sqrt(theta2);
    A = sin(theta) / theta;
    const double s2 = sin(theta / 2.0);
    B = 2.0 * s2 * s2 / theta2;
  }
  // W = [w]x ; W W = w w' - theta2 I
  R[0] = 1.0 + B * (x * x - theta2); R[1] = -A * z + B * (x * y);        R[2] = A * y + B * (x * z);
  R[3] = A * z + B * (x * y);        R[4] = 1.0 + B * (y * y - theta2); R[5] = -A * x + B * (y * z);
  R[6] = -A * y + B * (x * z);       R[7] = A * x + B * (y * z);        R[8] = 1.0 + B * (z * z - theta2);
}

// SO3::Logmap (gtsam/geometry/SO3.cpp:299-375), branch for branch
GSX_HD void so3_log(const double* R, double* omega) {
  const double R11 = R[0], R12 = R[1], R13 = R[2], R21 = R[3], R22 = R[4], R23 = R[5], R31 = R[6], R32 = R[7], R33 = R[8];
  const double tr = R11 + R22 + R33;
  const double kPi = 3.14159265358979323846;
  if (tr + 1.0 < 1e-3) {
    if (R33 > R22 && R33 > R11) {
      const double W = R21 - R12, Q1 = 2.0 + 2.0 * R33, Q2 = R31 + R13, Q3 = R23 + R32;
      const double r = sqrt(Q1), one_over_r = 1 / r, norm = sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W);
      const double sgn_w = W < 0 ? -1.0 : 1.0, mag = kPi - (2 * sgn_w * W) / norm, scale = 0.5 * one_over_r * mag;
      omega[0] = sgn_w * scale * Q2; omega[1] = sgn_w * scale * Q3; omega[2] = sgn_w * scale * Q1;
    } else if (R22 > R11) {
      const double W = R13 - R31, Q1 = 2.0 + 2.0 * R22, Q2 = R23 + R32, Q3 = R12 + R21;
      const double r = sqrt(Q1), one_over_r = 1 / r, norm = sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W);
      const double sgn_w = W < 0 ? -1.0 : 1.0, mag = kPi - (2 * sgn_w * W) / norm, scale = 0.5 * one_over_r * mag;
      omega[0] = sgn_w * scale * Q3; omega[1] = sgn_w * scale * Q1; omega[2] = sgn_w * scale * Q2;
    } else {
      const double W = R32 - R23, Q1 = 2.0 + 2.0 * R11, Q2 = R12 + R21, Q3 = R31 + R13;
      const double r = sqrt(Q1), one_over_r = 1 / r, norm = sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W);
      const double sgn_w = W < 0 ? -1.0 : 1.0, mag = kPi - (2 * sgn_w * W) / norm, scale = 0.5 * one_over_r * mag;
      omega[0] = sgn_w * scale * Q1; omega[1] = sgn_w * scale * Q2; omega[2] = sgn_w * scale * Q3;
    }
  } else {
    double magnitude;
    const double tr_3 = tr - 3.0;
    if (tr_3 < -1e-6) {
      const double theta = acos((tr - 1.0) / 2.0);
      magnitude = theta / (2.0 * sin(theta));
    } else {
      magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0;
    }
    omega[0] = magnitude * (R32 - R23); omega[1] = magnitude * (R13 - R31); omega[2] = magnitude * (R21 - R12);
  }
}

// InitializePose3::gradientTron (InitializePose3.cpp:256-275): the th != th perturbation branch and the th > 1e-5 cut as
// written there
GSX_HD void gradient_tron(const double* R1, const double* R2, double a, double b, double* g) {
  double Q[9], l[3];
  mat_tmul(R1, R2, Q);  // R1.between(R2)
  so3_log(Q, l);
  double th = sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
  if (th != th) {
    const double pw[3] = {0.01, 0.01, 0.01};
    double E[9], R1p[9];
    so3_exp(pw, E);
    mat_mul(R1, E, R1p);
    mat_tmul(R1p, R2, Q);
    so3_log(Q, l);
    th = sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
  }
  if (th > 1e-5 && th == th) {
    l[0] = l[0] / th; l[1] = l[1] / th; l[2] = l[2] / th;
  } else {
    l[0] = l[1] = l[2] = 0.0;
    th = 0.0;
  }
  const double fdot = a * b * th * exp(-b * th);
  g[0] = fdot * l[0]; g[1] = fdot * l[1]; g[2] = fdot * l[2];
}

// sum of six products to about twice the working precision (two-product by fma, two-sum): the skew part of R' M is a
// difference of nearly equal sums, and the polish below is only as good as this residual
GSX_HD double dot6(const double* a, const double* b) {
  double s = 0.0, c = 0.0;
  for (int i = 0; i < 6; ++i) {
    const double p = a[i] * b[i];
    const double e = fma(a[i], b[i], -p);
    const double t = s + p;
    const double z = t - s;
    c += ((s - (t - z)) + (p - z)) + e;
    s = t;
  }
  return s + c;
}

// Rot3::ClosestTo (gtsam/geometry/SO3.cpp:202-208): U diag(1, 1, det(U V')) V' of M = U S V'.
// One-sided Jacobi rotations on the columns of M (A V = U S, no M'M is formed) until every pair of columns is orthogonal to
// working precision.  With the two dominant pairs (u1, v1), (u2, v2) the answer is
//     u1 v1' + u2 v2' + (u1 x u2)(v1 x v2)',
// because u1 x u2 = det(U) u3 and v1 x v2 = det(V) v3: the third pair — the one a tiny singular value defines badly — and
// the determinant never have to be formed.  Two passes of two cheap corrections follow: a Newton-Schulz step, which
// takes the loss of orthogonality from eps to eps^2, and a Newton step on the stationarity condition "R' M symmetric" (the
// rotation w with (tr(S) I - S) w = vee(S - S'), S = R' M), which removes the rotation error the sweeps left; the second
// pass works on the rounding of the first.
GSX_HD void closest_rotation(const double* M, double* R) {
  double a[9], v[9];
  double scale = 0.0;
  for (int i = 0; i < 9; ++i) scale = fmax(scale, fabs(M[i]));
  if (!(scale > 0.0) || !(scale < 1.7e308)) {  // zero or non-finite input: no closest rotation; hand back what Eigen's
    for (int i = 0; i < 9; ++i) R[i] = (scale == 0.0) ? ((i % 4 == 0) ? 1.0 : 0.0) : NAN;  // SVD of 0 gives (U = V = I)
    return;
  }
  for (int i = 0; i < 9; ++i) a[i] = M[i] / scale;
  mat_identity(v);
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double alpha = a[p] * a[p] + a[3 + p] * a[3 + p] + a[6 + p] * a[6 + p];
        const double beta = a[q] * a[q] + a[3 + q] * a[3 + q] + a[6 + q] * a[6 + q];
        const double gamma = a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];
        if (gamma == 0.0 || fabs(gamma) <= 1.1102230246251565e-16 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double ap = a[3 * r + p], aq = a[3 * r + q];
          a[3 * r + p] = c * ap - s * aq;
          a[3 * r + q] = s * ap + c * aq;
          const double vp = v[3 * r + p], vq = v[3 * r + q];
          v[3 * r + p] = c * vp - s * vq;
          v[3 * r + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double n2[3];
  for (int c = 0; c < 3; ++c) n2[c] = a[c] * a[c] + a[3 + c] * a[3 + c] + a[6 + c] * a[6 + c];
  int i3 = 0;
  if (n2[1] < n2[i3]) i3 = 1;
  if (n2[2] < n2[i3]) i3 = 2;
  const int i1 = (i3 + 1) % 3, i2 = (i3 + 2) % 3;  // (the order of the two dominant pairs does not matter)
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
  const double s1 = sqrt(n2[i1]);
  for (int r = 0; r < 3; ++r) { u1[r] = a[3 * r + i1] / s1; u2[r] = a[3 * r + i2]; v1[r] = v[3 * r + i1]; v2[r] = v[3 * r + i2]; }
  const double d12 = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
  for (int r = 0; r < 3; ++r) u2[r] -= d12 * u1[r];
  const double s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  for (int r = 0; r < 3; ++r) u2[r] /= s2;
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1]; v3[1] = v1[2] * v2[0] - v1[0] * v2[2]; v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
  double R0[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R0[3 * i + j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
  for (int pass = 0; pass < 2; ++pass) {
    // Newton-Schulz: R <- R (3 I - R'R) / 2
    double G[9], T[9];
    mat_tmul(R0, R0, G);
    for (int i = 0; i < 9; ++i) G[i] = ((i % 4 == 0) ? 1.5 : 0.0) - 0.5 * G[i];
    mat_mul(R0, G, T);
    for (int i = 0; i < 9; ++i) R0[i] = T[i];
    // S = R' (M / scale); its skew part to twice the precision
    double S[9], Mn[9];
    for (int i = 0; i < 9; ++i) Mn[i] = M[i] / scale;
    mat_tmul(R0, Mn, S);
    double k[3];
    {
      // vee(S - S'): (S21 - S12, S02 - S20, S10 - S01), S_ij = sum_r R0[r][i] Mn[r][j]
      const int ii[3] = {2, 0, 1}, jj[3] = {1, 2, 0};
      for (int e = 0; e < 3; ++e) {
        double x[6], y[6];
        for (int r = 0; r < 3; ++r) {
          x[r] = R0[3 * r + ii[e]];     y[r] = Mn[3 * r + jj[e]];
          x[3 + r] = -R0[3 * r + jj[e]]; y[3 + r] = Mn[3 * r + ii[e]];
        }
        k[e] = dot6(x, y);
      }
    }
    const double trS = S[0] + S[4] + S[8];
    double H[9];  // tr(S) I - sym(S)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) H[3 * i + j] = ((i == j) ? trS : 0.0) - 0.5 * (S[3 * i + j] + S[3 * j + i]);
    // w = H^-1 k by the adjugate (H is symmetric, its eigenvalues are the pairwise sums of the signed singular values)
    const double c00 = H[4] * H[8] - H[5] * H[7], c01 = H[5] * H[6] - H[3] * H[8], c02 = H[3] * H[7] - H[4] * H[6];
    const double det = H[0] * c00 + H[1] * c01 + H[2] * c02;
    if (!(fabs(det) > 0.0)) break;
    const double c11 = H[0] * H[8] - H[2] * H[6], c12 = H[1] * H[6] - H[0] * H[7], c22 = H[0] * H[4] - H[1] * H[3];
    double w[3];
    w[0] = (c00 * k[0] + c01 * k[1] + c02 * k[2]) / det;
    w[1] = (c01 * k[0] + c11 * k[1] + c12 * k[2]) / det;
    w[2] = (c02 * k[0] + c12 * k[1] + c22 * k[2]) / det;
    if (!(fabs(w[0]) + fabs(w[1]) + fabs(w[2]) < 1e-3)) break;  // not a small correction: the input has no unique answer
    double E[9];
    so3_exp(w, E);
    mat_mul(R0, E, T);
    for (int i = 0; i < 9; ++i) R0[i] = T[i];
  }
  for (int i = 0; i < 9; ++i) R[i] = R0[i];
}

}  // namespace initm
}  // namespace gsx
