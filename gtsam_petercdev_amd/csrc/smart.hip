// smart.hip — SmartProjectionPoseFactor<Cal3_S2> on the device (gfx950, wave64): GSX_F_SMART_PROJECTION.
//
//   smart_triangulate_kernel   pass one of linearize AND of the error: one lane per factor.  Prepares the cameras
//                              pose (+) body_P_sensor, consults the re-triangulation cache (decideIfTriangulate,
//                              gtsam/slam/SmartProjectionFactor.h:127-165), triangulates when a camera moved by more than
//                              the threshold (triangulateSafe, the short-track path of triangulate_math.h) and leaves
//                              cameras, point and status in the handle's SmartDev tables.
//   smart_linearize_kernel     pass two of linearize: one wave per factor, one lane per column of [F b] (6 nk + 1 <= 49).
//                              A lane holds its column of 2 nk <= 16 rows in registers; the three Householder reflectors
//                              of E are the same in every lane, so applying them is lane-local, and rows 3 .. 2 nk - 1 go
//                              straight into the factor's [A b] slot: A = Q_2'[F b], Q_2 an orthonormal basis of the left
//                              null space of E.  (E'E)^-1 is never formed and no SVD is run.
//   smart_error_kernel         pass two of the error: one lane per factor, 0.5 |whitened (h - z)|^2 over all 2 nk rows at
//                              the cached point (totalReprojectionError), then the block reduction.
//
// A factor without a valid point writes the all-zero block and counts 0 in the error (ZERO_ON_DEGENERACY,
// SmartProjectionFactor.h:214-220, :427-429).  The per-factor arithmetic is csrc/smart_math.h.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "smart_math.h"
#include "wave_util.h"

namespace gsx {

namespace {

struct SmartFactor {   // what the three kernels read of one factor before they touch the state
  int nk, kp, slot;
  const double *meas, *sensor, *z;
  double inv_sigma;
};
__device__ __forceinline__ SmartFactor load_factor(const DevProblem& P, const SmartDev& S, int f) {
  SmartFactor F;
  F.kp = P.f_key_ptr[f];
  F.nk = P.f_key_ptr[f + 1] - F.kp;
  F.slot = S.slot[f];
  F.meas = P.meas + P.f_meas_off[f];
  const long long nmeas = P.f_meas_off[f + 1] - P.f_meas_off[f];
  F.sensor = smart::sensor_of(F.meas, nmeas, F.nk);
  F.z = smart::pixels_of(F.meas, nmeas, F.nk);
  F.inv_sigma = (P.f_noise_kind[f] & GSX_NOISE_BASE_MASK) == GSX_NOISE_ISOTROPIC ? 1.0 / P.noise[P.f_noise_off[f]] : 1.0;
  return F;
}

__global__ void __launch_bounds__(64) smart_triangulate_kernel(DevProblem P, const int* list, int n, const double* values,
                                                               SmartDev S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SmartFactor F = load_factor(P, S, list[i]);
  trim::Camera* cams = reinterpret_cast<trim::Camera*>(S.cams) + (size_t)F.slot * smart::kMaxViews;
  for (int k = 0; k < F.nk; ++k)
    smart::view_camera(values + P.var_state_off[P.f_vars[F.kp + k]], F.meas, F.sensor, cams[k]);
  double* cache = S.cache + (size_t)F.slot * 12 * smart::kMaxViews;
  if (!smart::decide_retriangulate(cams, F.nk, F.meas[smart::M_RETRIANGULATION], S.status[F.slot], cache)) return;
  trim::Params prm;
  smart::triangulation_params(F.meas, prm);
  double point[3];
  const int status = smart::triangulate(cams, F.z, F.nk, prm, point);
  S.point[3 * F.slot] = point[0];
  S.point[3 * F.slot + 1] = point[1];
  S.point[3 * F.slot + 2] = point[2];
  S.status[F.slot] = status;
  atomicAdd(&S.counters[1], 1);
}

constexpr int kWavesPerBlock = 4;
__global__ void __launch_bounds__(64 * kWavesPerBlock) smart_linearize_kernel(DevProblem P, const int* list, int n,
                                                                                SmartDev S, double* jac) {
  const int i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;   // (wave-uniform)
  const int f = list[i];
  const SmartFactor F = load_factor(P, S, f);
  const int m = 2 * F.nk - 3, ncols = 6 * F.nk + 1;
  const int col = lane < ncols ? lane : ncols - 1;   // the idle lanes shadow the last column and store nothing
  const trim::Camera* cams = reinterpret_cast<const trim::Camera*>(S.cams) + (size_t)F.slot * smart::kMaxViews;
  double x[smart::kMaxRows];
  bool ok = S.status[F.slot] == trim::ST_VALID;
  if (ok) {
    const double p[3] = {S.point[3 * F.slot], S.point[3 * F.slot + 1], S.point[3 * F.slot + 2]};
    ok = smart::block_column(cams, F.sensor, F.z, F.nk, p, F.inv_sigma, col, x);
  }
  if (!ok && lane == 0) atomicAdd(&S.counters[0], 1);
  if (lane >= ncols) return;
  double* out = jac + P.f_jac_off[f] + (size_t)col * m;
#pragma unroll
  for (int r = 3; r < smart::kMaxRows; ++r)
    if (r - 3 < m) out[r - 3] = ok ? x[r] : 0.0;
}

__global__ void __launch_bounds__(256) smart_error_kernel(DevProblem P, const int* list, int n, SmartDev S, double* partials) {
  __shared__ double ws[4];
  double acc = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const SmartFactor F = load_factor(P, S, list[i]);
    if (S.status[F.slot] != trim::ST_VALID) continue;
    const trim::Camera* cams = reinterpret_cast<const trim::Camera*>(S.cams) + (size_t)F.slot * smart::kMaxViews;
    const double p[3] = {S.point[3 * F.slot], S.point[3 * F.slot + 1], S.point[3 * F.slot + 2]};
    bool ok;
    acc += smart::reprojection_error(cams, F.z, F.nk, p, F.inv_sigma, &ok);
  }
  // fixed summation order: lanes by shuffle, then the four waves in order
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

}  // namespace

void launch_smart_triangulate(const DevProblem& P, const int* list, int n, const double* values, const SmartDev& S,
                              hipStream_t st) {
  if (n <= 0) return;
  smart_triangulate_kernel<<<(n + 63) / 64, 64, 0, st>>>(P, list, n, values, S);
}

void launch_smart_linearize(const DevProblem& P, const int* list, int n, const SmartDev& S, double* jac, hipStream_t st) {
  if (n <= 0) return;
  smart_linearize_kernel<<<(n + kWavesPerBlock - 1) / kWavesPerBlock, 64 * kWavesPerBlock, 0, st>>>(P, list, n, S, jac);
}

void launch_smart_error(const DevProblem& P, const int* list, int n, const SmartDev& S, double* partials, int blocks,
                        hipStream_t st) {
  if (n <= 0 || blocks <= 0) return;
  smart_error_kernel<<<blocks, 256, 0, st>>>(P, list, n, S, partials);
}

}  // namespace gsx
