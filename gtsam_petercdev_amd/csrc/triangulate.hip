// triangulate.hip — batched landmark triangulation on the device (gfx950, FP64): gsx_triangulate, gsx_triangulate_landmarks.
// Reference: gtsam/geometry/triangulation.{h,cpp} — triangulatePoint3 (DLT or LOST, optionally refined by LM on one Point3)
// and triangulateSafe — which the reference runs one track at a time through a NonlinearFactorGraph.  Here every track is
// independent work for one lane (short tracks) or one wave (long tracks); the per-track arithmetic is csrc/triangulate_math.h,
// shared with the host program of tests/native.
//
// Three kernels, no atomics, no LDS, nothing waits on another workgroup; the LM loop lives in the kernel, so the launch count
// does not depend on the data:
//   triangulate_cameras_kernel   one lane per camera: P = K [R' | -R' t], pose (composed with body_P_sensor), calibration
//   triangulate_short_kernel     one lane per track, for tracks shorter than kWaveTrackMin
//   triangulate_long_kernel      one wave per track: every lane reduces its observations (lane, lane + 64, ...) to its own
//                                4 x 4 triangle, the triangles are merged pairwise across the wave (TSQR: stack two triangles,
//                                re-triangularise) in 6 rounds of cross-lane moves, lane 0 finishes the track
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "init_device.h"
#include "triangulate_math.h"

using namespace gsx;
using namespace gsx::initdev;
namespace tm_ = gsx::trim;

namespace {

// A track of at least this many observations goes to the wave kernel.  Chosen from the code, not measured.  The wave kernel
// pays 6 merge rounds of 4 row insertions in each of its 64 lanes, 64 x 24 insertions of wave work, for ONE track; the lane
// kernel pays 2m insertions in one lane per track and keeps the other 63 lanes for 63 other tracks.  In throughput the lane
// kernel therefore wins at every BAL length; what the wave kernel removes is the tail, a wave of the lane kernel running as
// long as its longest track.  64 is the first length at which every lane of the wave has an observation to reduce.
constexpr int kWaveTrackMin = 64;
constexpr int kMaxBlocks = 2048;

enum { TT_HOST, TT_CAMERAS, TT_SHORT, TT_LONG, TT_TOTAL, TT_COUNT };
double g_timings[TT_COUNT] = {};

__global__ void __launch_bounds__(kThreads) triangulate_cameras_kernel(int n_cameras, const int* __restrict__ kind,
                                                                       const double* __restrict__ in,
                                                                       const int* __restrict__ sensor_of,
                                                                       const double* __restrict__ sensors,
                                                                       tm_::Camera* __restrict__ out) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_cameras) return;
  double st[tm_::kCameraInDoubles];
#pragma unroll
  for (int i = 0; i < tm_::kCameraInDoubles; ++i) st[i] = in[(int64_t)c * tm_::kCameraInDoubles + i];
  const int s = sensor_of ? sensor_of[c] : -1;
  tm_::Camera cam;
  tm_::prepare_camera(kind[c], st, s >= 0 ? sensors + 12 * (int64_t)s : nullptr, cam);
  out[c] = cam;
}

__global__ void __launch_bounds__(kThreads) triangulate_short_kernel(int64_t n, const int64_t* __restrict__ ids,
                                                                     const int64_t* __restrict__ track_ptr,
                                                                     const int32_t* __restrict__ obs_cam,
                                                                     const double* __restrict__ obs_xy,
                                                                     const tm_::Camera* __restrict__ cams, tm_::Params P,
                                                                     double* __restrict__ points, int32_t* __restrict__ status,
                                                                     int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x; w < n; w += stride) {
    const int64_t t = ids[w], b = track_ptr[t];
    const int m = (int)(track_ptr[t + 1] - b);
    double pt[3];
    int cnt[2];
    const int st = tm_::triangulate_track(cams, obs_cam + b, obs_xy + 2 * b, m, P, pt, cnt);
    points[3 * t] = pt[0]; points[3 * t + 1] = pt[1]; points[3 * t + 2] = pt[2];
    status[t] = st;
    if (counts) { counts[2 * t] = cnt[0]; counts[2 * t + 1] = cnt[1]; }
  }
}

__global__ void __launch_bounds__(kThreads) triangulate_long_kernel(int64_t n, const int64_t* __restrict__ ids,
                                                                    const int64_t* __restrict__ track_ptr,
                                                                    const int32_t* __restrict__ obs_cam,
                                                                    const double* __restrict__ obs_xy,
                                                                    const tm_::Camera* __restrict__ cams, tm_::Params P,
                                                                    double* __restrict__ points, int32_t* __restrict__ status,
                                                                    int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kThreads) >> 6;
  for (int64_t w = wave; w < n; w += n_waves) {   // wave-uniform
    const int64_t t = ids[w], b = track_ptr[t];
    const int m = (int)(track_ptr[t + 1] - b);
    const int32_t* oc = obs_cam + b;
    const double* oz = obs_xy + 2 * b;
    double T[10];
    tm_::tri_zero(T);
    int st = tm_::ST_VALID;
    for (int i = lane; i < m; i += 64) {
      const int s = tm_::accumulate_observation(cams, oc, oz, m, i, P, T);
      st = s > st ? s : st;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      double other[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) other[k] = __shfl_down(T[k], off, 64);
      const int so = __shfl_down(st, off, 64);
      if (lane < off) {
        tm_::tri_merge(T, other);
        st = so > st ? so : st;
      }
    }
    if (lane == 0) {
      double pt[3] = {NAN, NAN, NAN};
      int cnt[2];
      if (st == tm_::ST_VALID) st = tm_::linear_finish(T, P, pt);
      st = tm_::finish_track(cams, oc, oz, m, P, st, pt, cnt);
      points[3 * t] = pt[0]; points[3 * t + 1] = pt[1]; points[3 * t + 2] = pt[2];
      status[t] = st;
      if (counts) { counts[2 * t] = cnt[0]; counts[2 * t + 1] = cnt[1]; }
    }
  }
}

// the params of the ABI -> the header's, validated (GSX_NOISE_CONSTRAINED, zero sigmas: GSX_E_INVALID)
gsx_status lower_params(const gsx_triangulation_params* in, tm_::Params& P) {
  gsx_triangulation_params d;
  gsx_triangulation_params_default(&d);
  if (!in) in = &d;
  if (!(in->rank_tol >= 0.0)) return GSX_E_INVALID;
  P.rank_tol = in->rank_tol;
  P.optimize = in->optimize != 0;
  P.use_lost = in->use_lost != 0;
  P.safe = in->safe != 0;
  P.landmark_distance_threshold = in->landmark_distance_threshold;
  P.outlier_threshold = in->dynamic_outlier_rejection_threshold;
  for (double& v : P.noise.p) v = 0.0;
  if (in->noise_kind < 0) {   // no model: the factors are not whitened; LOST takes sigma 1e-4 (triangulation.h:439)
    P.noise.kind = GSX_NOISE_UNIT;
    P.lost_sigma = 1e-4;
    return GSX_OK;
  }
  const int base = in->noise_kind & GSX_NOISE_BASE_MASK, loss = in->noise_kind >> 4;
  if (base > GSX_NOISE_GAUSSIAN || loss < 0 || loss > 3) return GSX_E_INVALID;
  const int np = tm_::noise_base_params(base);
  for (int i = 0; i < np + (loss ? 1 : 0); ++i) {
    if (!std::isfinite(in->noise[i])) return GSX_E_INVALID;
    P.noise.p[i] = in->noise[i];
  }
  if (loss && !(in->noise[np] > 0.0)) return GSX_E_INVALID;
  P.noise.kind = in->noise_kind;
  const double* s = in->noise;
  if (base == GSX_NOISE_UNIT) {
    P.lost_sigma = 1.0;
  } else if (base == GSX_NOISE_ISOTROPIC) {
    if (!(s[0] > 0.0)) return GSX_E_INVALID;
    P.lost_sigma = s[0];
  } else if (base == GSX_NOISE_DIAGONAL) {
    if (!(s[0] > 0.0) || !(s[1] > 0.0)) return GSX_E_INVALID;
    P.lost_sigma = 0.5 * (s[0] + s[1]);
  } else {   // R = [a b; 0 c]: Gaussian::sigmas() = sqrt(diag((R'R)^-1)) (NoiseModel.cpp:159-161)
    const double a = s[0], b = s[1], c = s[3];
    if (a == 0.0 || c == 0.0) return GSX_E_INVALID;
    P.lost_sigma = 0.5 * (std::sqrt(b * b + c * c) / std::fabs(a * c) + 1.0 / std::fabs(c));
  }
  return GSX_OK;
}

struct CameraTable {   // host image of the cameras kernel's input
  std::vector<int> kind, sensor_of;
  std::vector<double> in, sensors;
  int size() const { return (int)kind.size(); }
};

gsx_status check_tracks(const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_camera, const double* obs_xy,
                        int n_cameras) {
  if (n_tracks < 0 || n_tracks > (int64_t)INT32_MAX * 16) return GSX_E_INVALID;
  if (n_tracks == 0) return GSX_OK;
  if (!track_ptr || track_ptr[0] != 0) return GSX_E_INVALID;
  for (int64_t t = 0; t < n_tracks; ++t) {
    const int64_t m = track_ptr[t + 1] - track_ptr[t];
    if (m < 0 || m > INT32_MAX) return GSX_E_INVALID;
  }
  const int64_t n_obs = track_ptr[n_tracks];
  if (n_obs > 0 && (!obs_camera || !obs_xy)) return GSX_E_INVALID;
  for (int64_t o = 0; o < n_obs; ++o)
    if (obs_camera[o] < 0 || obs_camera[o] >= n_cameras) return GSX_E_INVALID;
  return GSX_OK;
}

// everything after validation: classes, upload, three launches, download
gsx_status run_device(const CameraTable& C, const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_camera,
                      const double* obs_xy, const tm_::Params& P, int32_t device, double* points_out, int32_t* status_out,
                      int32_t* lm_counts_out) {
  const auto t_begin = std::chrono::steady_clock::now();
  std::fill(g_timings, g_timings + TT_COUNT, 0.0);
  gsx_status st = check_device(device);
  if (st != GSX_OK) return st;
  if (n_tracks == 0) return GSX_OK;
  // the host sorts the track indices into the two classes once
  std::vector<int64_t> ids((size_t)n_tracks);
  int64_t n_short = 0, n_long = 0;
  for (int64_t t = 0; t < n_tracks; ++t)
    if (track_ptr[t + 1] - track_ptr[t] < kWaveTrackMin) ids[n_short++] = t;
  for (int64_t t = 0; t < n_tracks; ++t)
    if (track_ptr[t + 1] - track_ptr[t] >= kWaveTrackMin) ids[n_short + n_long++] = t;
  const int64_t n_obs = track_ptr[n_tracks];
  g_timings[TT_HOST] = host_ms_since(t_begin);

  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  Dev<int> d_kind, d_sensor_of;
  Dev<double> d_in, d_sensors, d_xy, d_points;
  Dev<int64_t> d_ids, d_ptr;
  Dev<int32_t> d_oc, d_status, d_counts;
  Dev<tm_::Camera> d_cams;
  const bool any_sensor = !C.sensors.empty();
  HIPTRY(d_kind.upload(C.kind, S.s));
  HIPTRY(d_in.upload(C.in, S.s));
  if (any_sensor) {
    HIPTRY(d_sensor_of.upload(C.sensor_of, S.s));
    HIPTRY(d_sensors.upload(C.sensors, S.s));
  }
  HIPTRY(d_cams.alloc((size_t)C.size()));
  HIPTRY(d_ids.upload(ids, S.s));
  HIPTRY(d_ptr.alloc((size_t)n_tracks + 1));
  HIPTRY(hipMemcpyAsync(d_ptr.p, track_ptr, ((size_t)n_tracks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, S.s));
  HIPTRY(d_oc.alloc((size_t)n_obs));
  HIPTRY(d_xy.alloc(2 * (size_t)n_obs));
  if (n_obs > 0) {
    HIPTRY(hipMemcpyAsync(d_oc.p, obs_camera, (size_t)n_obs * sizeof(int32_t), hipMemcpyHostToDevice, S.s));
    HIPTRY(hipMemcpyAsync(d_xy.p, obs_xy, 2 * (size_t)n_obs * sizeof(double), hipMemcpyHostToDevice, S.s));
  }
  HIPTRY(d_points.alloc(3 * (size_t)n_tracks));
  HIPTRY(d_status.alloc((size_t)n_tracks));
  if (lm_counts_out) HIPTRY(d_counts.alloc(2 * (size_t)n_tracks));

  EventPair e_cam, e_short, e_long;
  if (C.size() > 0) {
    e_cam.begin(S.s);
    hipLaunchKernelGGL(triangulate_cameras_kernel, dim3(blocks_for(C.size())), dim3(kThreads), 0, S.s, C.size(), d_kind.p,
                       d_in.p, any_sensor ? d_sensor_of.p : (const int*)nullptr, d_sensors.p, d_cams.p);
    HIPTRY(hipGetLastError());
    e_cam.end();
  }
  if (n_short > 0) {
    e_short.begin(S.s);
    const int blocks = (int)std::min<int64_t>((n_short + kThreads - 1) / kThreads, kMaxBlocks);
    hipLaunchKernelGGL(triangulate_short_kernel, dim3(blocks), dim3(kThreads), 0, S.s, n_short, d_ids.p, d_ptr.p, d_oc.p,
                       d_xy.p, d_cams.p, P, d_points.p, d_status.p, lm_counts_out ? d_counts.p : (int32_t*)nullptr);
    HIPTRY(hipGetLastError());
    e_short.end();
  }
  if (n_long > 0) {
    e_long.begin(S.s);
    const int waves_per_block = kThreads / 64;
    const int blocks = (int)std::min<int64_t>((n_long + waves_per_block - 1) / waves_per_block, kMaxBlocks);
    hipLaunchKernelGGL(triangulate_long_kernel, dim3(blocks), dim3(kThreads), 0, S.s, n_long, d_ids.p + n_short, d_ptr.p,
                       d_oc.p, d_xy.p, d_cams.p, P, d_points.p, d_status.p, lm_counts_out ? d_counts.p : (int32_t*)nullptr);
    HIPTRY(hipGetLastError());
    e_long.end();
  }
  HIPTRY(hipMemcpyAsync(points_out, d_points.p, 3 * (size_t)n_tracks * sizeof(double), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipMemcpyAsync(status_out, d_status.p, (size_t)n_tracks * sizeof(int32_t), hipMemcpyDeviceToHost, S.s));
  if (lm_counts_out)
    HIPTRY(hipMemcpyAsync(lm_counts_out, d_counts.p, 2 * (size_t)n_tracks * sizeof(int32_t), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipStreamSynchronize(S.s));
  if (C.size() > 0) g_timings[TT_CAMERAS] = e_cam.ms();
  if (n_short > 0) g_timings[TT_SHORT] = e_short.ms();
  if (n_long > 0) g_timings[TT_LONG] = e_long.ms();
  g_timings[TT_TOTAL] = host_ms_since(t_begin);
  return GSX_OK;
}

// the tracks of a problem description: the GSX_F_SFM / GSX_F_PROJECTION factors grouped per landmark (their second key, a
// VECTOR(3) variable), landmarks in the order of desc, observations in factor order
struct Grouping {
  std::vector<int> landmark_vars;
  std::vector<int64_t> track_ptr;
  std::vector<int> obs_factor;
};

gsx_status group_tracks(const gsx_problem_desc* d, Grouping& G) {
  if (!d || d->n_vars < 0 || d->n_factors < 0) return GSX_E_INVALID;
  if (d->n_vars > 0 && (!d->var_types || !d->var_dims || !d->var_keys)) return GSX_E_INVALID;
  if (d->n_factors > 0 && (!d->f_type || !d->f_key_ptr || !d->f_vars || !d->f_meas_ptr || !d->meas)) return GSX_E_INVALID;
  std::vector<int64_t> count((size_t)d->n_vars, 0);
  std::vector<int> kind_seen((size_t)d->n_vars, -1);
  for (int f = 0; f < d->n_factors; ++f) {
    const int ty = d->f_type[f];
    if (ty != GSX_F_SFM && ty != GSX_F_PROJECTION) continue;
    if (d->f_key_ptr[f + 1] - d->f_key_ptr[f] != 2) return GSX_E_INVALID;
    const int cam = d->f_vars[d->f_key_ptr[f]], pt = d->f_vars[d->f_key_ptr[f] + 1];
    if (cam < 0 || cam >= d->n_vars || pt < 0 || pt >= d->n_vars) return GSX_E_INVALID;
    if (d->var_types[pt] != GSX_VAR_VECTOR || d->var_dims[pt] != 3) return GSX_E_INVALID;
    const int64_t nm = d->f_meas_ptr[f + 1] - d->f_meas_ptr[f];
    if (ty == GSX_F_SFM ? (d->var_types[cam] != GSX_VAR_CAMERA || nm != 2)
                        : (d->var_types[cam] != GSX_VAR_POSE3 || (nm != 7 && nm != 19)))
      return GSX_E_INVALID;
    if (kind_seen[pt] >= 0 && kind_seen[pt] != ty) return GSX_E_INVALID;   // a landmark seen by both camera kinds
    kind_seen[pt] = ty;
    ++count[pt];
  }
  std::vector<int64_t> slot((size_t)d->n_vars, -1);
  G.track_ptr.assign(1, 0);
  for (int v = 0; v < d->n_vars; ++v)
    if (count[v] > 0) {
      slot[v] = (int64_t)G.landmark_vars.size();
      G.landmark_vars.push_back(v);
      G.track_ptr.push_back(G.track_ptr.back() + count[v]);
    }
  G.obs_factor.assign((size_t)G.track_ptr.back(), 0);
  std::vector<int64_t> fill(G.track_ptr.begin(), G.track_ptr.end() - 1);
  for (int f = 0; f < d->n_factors; ++f) {
    const int ty = d->f_type[f];
    if (ty != GSX_F_SFM && ty != GSX_F_PROJECTION) continue;
    const int pt = d->f_vars[d->f_key_ptr[f] + 1];
    G.obs_factor[(size_t)fill[slot[pt]]++] = f;
  }
  return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_triangulation_params_default(gsx_triangulation_params* p) {
  if (!p) return;
  p->rank_tol = 1e-9;
  p->optimize = 0;
  p->use_lost = 0;
  p->noise_kind = -1;
  for (double& v : p->noise) v = 0.0;
  p->landmark_distance_threshold = -1.0;
  p->dynamic_outlier_rejection_threshold = -1.0;
  p->safe = 0;
}

gsx_status gsx_triangulate(int32_t camera_kind, const double* cameras, int32_t n_cameras, const double* calibrations,
                           int32_t n_calibrations, const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_camera,
                           const double* obs_xy, const gsx_triangulation_params* params, int32_t device, double* points_out,
                           int32_t* status_out, int32_t* lm_counts_out) {
  if (camera_kind != GSX_CAMERA_POSE3_CAL3_S2 && camera_kind != GSX_CAMERA_CAL3BUNDLER) return GSX_E_INVALID;
  if (n_cameras < 0 || (n_cameras > 0 && !cameras)) return GSX_E_INVALID;
  if (camera_kind == GSX_CAMERA_POSE3_CAL3_S2 && n_cameras > 0 &&
      (!calibrations || (n_calibrations != 1 && n_calibrations != n_cameras)))
    return GSX_E_INVALID;
  tm_::Params P;
  gsx_status st = lower_params(params, P);
  if (st != GSX_OK) return st;
  st = check_tracks(track_ptr, n_tracks, obs_camera, obs_xy, n_cameras);
  if (st != GSX_OK) return st;
  if (n_tracks > 0 && (!points_out || !status_out)) return GSX_E_INVALID;
  CameraTable C;
  C.kind.assign((size_t)n_cameras, camera_kind == GSX_CAMERA_CAL3BUNDLER ? tm_::CAM_BUNDLER : tm_::CAM_POSE3);
  C.in.resize((size_t)n_cameras * tm_::kCameraInDoubles);
  for (int c = 0; c < n_cameras; ++c) {
    double* o = C.in.data() + (size_t)c * tm_::kCameraInDoubles;
    if (camera_kind == GSX_CAMERA_CAL3BUNDLER) {
      std::copy(cameras + 17 * (size_t)c, cameras + 17 * (size_t)c + 17, o);
    } else {
      std::copy(cameras + 12 * (size_t)c, cameras + 12 * (size_t)c + 12, o);
      const double* k = calibrations + (n_calibrations == 1 ? 0 : 5 * (size_t)c);
      std::copy(k, k + 5, o + 12);
    }
  }
  return run_device(C, track_ptr, n_tracks, obs_camera, obs_xy, P, device, points_out, status_out, lm_counts_out);
}

gsx_status gsx_triangulation_tracks(const gsx_problem_desc* desc, int32_t* n_landmarks, int64_t* n_observations,
                                    int32_t* landmark_vars, int64_t* track_ptr, int32_t* obs_factor) {
  if (gsx::enter_call(desc, "gsx_triangulation_tracks") != GSX_OK) return GSX_E_INVALID;
  Grouping G;
  const gsx_status st = group_tracks(desc, G);
  if (st != GSX_OK) return st;
  if (n_landmarks) *n_landmarks = (int32_t)G.landmark_vars.size();
  if (n_observations) *n_observations = G.track_ptr.back();
  if (landmark_vars) std::copy(G.landmark_vars.begin(), G.landmark_vars.end(), landmark_vars);
  if (track_ptr) std::copy(G.track_ptr.begin(), G.track_ptr.end(), track_ptr);
  if (obs_factor) std::copy(G.obs_factor.begin(), G.obs_factor.end(), obs_factor);
  return GSX_OK;
}

gsx_status gsx_triangulate_landmarks(const gsx_problem_desc* desc, const double* values, int64_t n_values,
                                     const gsx_triangulation_params* params, int32_t device, double* values_out,
                                     int32_t* status_out, int32_t* n_landmarks_out) {
  if (gsx::enter_call(desc, "gsx_triangulate_landmarks") != GSX_OK) return GSX_E_INVALID;
  Grouping G;
  gsx_status st = group_tracks(desc, G);
  if (st != GSX_OK) return st;
  std::vector<int> state_off;
  const int64_t n_state = desc_state_size(desc, &state_off);
  if (n_values != n_state || (n_state > 0 && (!values || !values_out))) return GSX_E_INVALID;
  const int64_t n_tracks = (int64_t)G.landmark_vars.size();
  if (n_tracks > 0 && !status_out) return GSX_E_INVALID;
  tm_::Params P;
  st = lower_params(params, P);
  if (st != GSX_OK) return st;
  // cameras: one per GSX_VAR_CAMERA variable seen, one per GSX_F_PROJECTION factor (its pose, calibration and sensor)
  CameraTable C;
  std::vector<int> cam_of_var((size_t)desc->n_vars, -1);
  const int64_t n_obs = G.track_ptr.back();
  std::vector<int32_t> obs_camera((size_t)n_obs);
  std::vector<double> obs_xy(2 * (size_t)n_obs);
  bool any_sensor = false;
  for (int64_t o = 0; o < n_obs; ++o) {
    const int f = G.obs_factor[(size_t)o];
    const int cam = desc->f_vars[desc->f_key_ptr[f]];
    const double* z = desc->meas + desc->f_meas_ptr[f];
    obs_xy[2 * o] = z[0];
    obs_xy[2 * o + 1] = z[1];
    const double* s = values + state_off[cam];
    if (desc->f_type[f] == GSX_F_SFM) {
      if (cam_of_var[cam] < 0) {
        cam_of_var[cam] = C.size();
        C.kind.push_back(tm_::CAM_BUNDLER);
        C.sensor_of.push_back(-1);
        C.in.insert(C.in.end(), s, s + 17);
      }
      obs_camera[(size_t)o] = cam_of_var[cam];
    } else {
      obs_camera[(size_t)o] = C.size();
      C.kind.push_back(tm_::CAM_POSE3);
      C.in.insert(C.in.end(), s, s + 12);
      C.in.insert(C.in.end(), z + 2, z + 7);
      if (desc->f_meas_ptr[f + 1] - desc->f_meas_ptr[f] == 19) {
        C.sensor_of.push_back((int)(C.sensors.size() / 12));
        C.sensors.insert(C.sensors.end(), z + 7, z + 19);
        any_sensor = true;
      } else {
        C.sensor_of.push_back(-1);
      }
    }
  }
  if (!any_sensor) C.sensors.clear();
  std::vector<double> points(3 * (size_t)n_tracks);
  st = run_device(C, G.track_ptr.data(), n_tracks, obs_camera.data(), obs_xy.data(), P, device, points.data(), status_out,
                  nullptr);
  if (st != GSX_OK) return st;
  std::copy(values, values + n_state, values_out);
  for (int64_t t = 0; t < n_tracks; ++t)
    if (status_out[t] == tm_::ST_VALID)   // a landmark that fails keeps its input value
      std::copy(points.begin() + 3 * t, points.begin() + 3 * t + 3, values_out + state_off[G.landmark_vars[(size_t)t]]);
  if (n_landmarks_out) *n_landmarks_out = (int32_t)n_tracks;
  return GSX_OK;
}

gsx_status gsx_triangulate_timings(double* out_ms, int32_t n) {
  if (!out_ms || n != TT_COUNT) return GSX_E_INVALID;
  std::copy(g_timings, g_timings + TT_COUNT, out_ms);
  return GSX_OK;
}

}  // extern "C"
