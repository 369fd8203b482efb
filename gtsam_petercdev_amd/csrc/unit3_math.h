// unit3_math.h — Unit3 (a point on the unit sphere, tangent 2) for host and device alike: the tangent basis and both
// charts, one definition each.  problem.cpp computes the attitude factor's basis with it once per factor and checks states
// with it; the kernels retract, take local coordinates and build the epipolar Jacobians with it.
//   basis              gtsam/geometry/Unit3.cpp:72-81, 128-138
//   retract            Unit3.cpp:255-282 (the theta < epsilon branch and the renormalisation of FromPoint3 included)
//   localCoordinates   Unit3.cpp:285-303 (the first-order branch at x -> 1 and the antipodal answer (pi, 0) included)
#pragma once
#include <cmath>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define GSX_U3_HD __host__ __device__ __forceinline__
#else
#define GSX_U3_HD inline
#endif

namespace gsx {

// b1 = normalize(n x axis) with the axis of the smallest |n_i| (ties go to the earlier axis, as the chain of <= in
// CalculateBestAxis), b2 = n x b1.  B row-major 3 x 2.
GSX_U3_HD void unit3_basis(const double* n, double* B) {
  const double mx = ::fabs(n[0]), my = ::fabs(n[1]), mz = ::fabs(n[2]);
  double a[3] = {0, 0, 0};
  if (mx <= my && mx <= mz) a[0] = 1;
  else if (my <= mx && my <= mz) a[1] = 1;
  else a[2] = 1;
  double b1[3] = {n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]};
  const double nrm = ::sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
  for (int r = 0; r < 3; ++r) b1[r] /= nrm;
  const double b2[3] = {n[1] * b1[2] - n[2] * b1[1], n[2] * b1[0] - n[0] * b1[2], n[0] * b1[1] - n[1] * b1[0]};
  for (int r = 0; r < 3; ++r) {
    B[2 * r] = b1[r];
    B[2 * r + 1] = b2[r];
  }
}

// q = p.retract(v): xi = B v, q = normalize(cos(theta) p + sin(theta) / theta xi), theta = |xi|; below machine epsilon
// normalize(cos(theta) p + xi)
GSX_U3_HD void unit3_retract(const double* p, const double* v, double* q) {
  double B[6], xi[3];
  unit3_basis(p, B);
  for (int r = 0; r < 3; ++r) xi[r] = B[2 * r] * v[0] + B[2 * r + 1] * v[1];
  const double theta = ::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  const double c = ::cos(theta);
  const double st = theta < 2.220446049250313e-16 ? 1.0 : ::sin(theta) / theta;
  double u[3];
  for (int r = 0; r < 3; ++r) u[r] = c * p[r] + xi[r] * st;
  const double nrm = ::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int r = 0; r < 3; ++r) q[r] = u[r] / nrm;
}

// out = p.localCoordinates(q): B' (y (q - x p)) with x = p . q and y = acos(x) / sqrt(1 - x^2)
GSX_U3_HD void unit3_local(const double* p, const double* q, double* out) {
  // the two branches below hang on the last bit of x and z: no contraction into FMAs here, so that host and device decide
  // alike, and as the plain products and sums of the reference do
#pragma clang fp contract(off)
  const double x = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
  const double z = 1 - x * x;
  double y;
  if (z < 2.220446049250313e-16) {
    if (x > 0) {
      y = 1.0 - (x - 1.0) / 3.0;
    } else {
      out[0] = 3.14159265358979323846;
      out[1] = 0.0;
      return;
    }
  } else {
    y = ::acos(x) / ::sqrt(z);
  }
  double B[6];
  unit3_basis(p, B);
  out[0] = out[1] = 0.0;
  for (int r = 0; r < 3; ++r) {
    const double w = q[r] - x * p[r];
    out[0] += (B[2 * r] * y) * w;
    out[1] += (B[2 * r + 1] * y) * w;
  }
}

// | |u| - 1 | within the tolerance a direction handed in must meet (that of GSX_F_ATTITUDE's directions)
GSX_U3_HD bool unit3_is_unit(const double* u) { return ::fabs(::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= 1e-9; }

}  // namespace gsx
