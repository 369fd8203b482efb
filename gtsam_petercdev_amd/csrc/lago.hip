// lago.hip — device part of the Pose2 initializer lago (gtsam/slam/lago.cpp) and its C ABI (include/gsx.h).  The host
// lowering and the trees are lago_graph.cpp.
//   lago_theta_to_root_kernel        computeThetasToRoot (:56-98) as pointer jumping, one launch per round
//   lago_orientation_blocks_kernel   the whitened rows [-1/s, 1/s | dtheta/s] of buildLinearOrientationGraph (:165-199)
//   lago_pose_blocks_kernel          the whitened 3 x 7 blocks of computePoses (:308-356)
//   lago_compose_kernel              Pose2(x, y, theta_lago + dtheta) (:361-370), or Pose2(given x, given y, theta) (:399-407)
// The two linear systems are solved by internal handles (direct solver), as the Pose3 initializer's are.
// Product code: no CPU fallback — every numeric entry point returns GSX_E_NO_DEVICE without a usable GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gsx_internal.h"
#include "init_device.h"

using namespace gsx;
using namespace gsx::initdev;

namespace {

// stage times of the last lago call of the process (gsx_lago_timings): host milliseconds for the two analyses, HIP events
// on the internal handles' streams for the device stages
enum { TL_ORIENTATION_ANALYSIS, TL_THETA_TO_ROOT, TL_ORIENTATION_BLOCKS, TL_ORIENTATION_SOLVE, TL_POSE_ANALYSIS,
       TL_POSE_BLOCKS, TL_POSE_SOLVE, TL_COMPOSE, TL_COUNT };
double g_timings[TL_COUNT] = {};

// One round of pointer jumping, one thread per node: every node holds (ancestor, sum of the deltas from the node up to,
// not including, that ancestor); it adds its ancestor's sum and jumps to the ancestor's ancestor.  The root holds
// (itself, 0) and absorbs.  Reads the buffers of the previous round only (double-buffered by the host): no launch reads
// what it writes, and nothing waits on another workgroup.  After r rounds a node of depth <= 2^r holds its sum to the root.
// 12 B read, 12 B gathered and 12 B written per node and round.
__global__ void __launch_bounds__(kThreads) lago_theta_to_root_kernel(int n, const int* __restrict__ anc_in,
                                                                      const double* __restrict__ sum_in,
                                                                      int* __restrict__ anc_out,
                                                                      double* __restrict__ sum_out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int a = anc_in[i];
  sum_out[i] = sum_in[i] + sum_in[a];
  anc_out[i] = anc_in[a];
}

// One thread per edge of the pose graph: its whitened row of the orientation system, at blocks + block_off[e] (1 x 3
// column-major, or 1 x 2 for an edge from the anchor, whose theta = 0 is substituted).  A tree edge keeps its measured
// dtheta; a chord takes dtheta - 2 pi round((dtheta + theta_root[key1] - theta_root[key2]) / 2 pi) (:186-193).  Diagonal::
// whiten multiplies by 1 / sigma (NoiseModel.cpp:323-325); sigma is the model's third (:160).  reg (may be NULL) gets the
// regularized dtheta; blocks may be NULL.  44 B read, 16 B gathered, 24 B written per edge.
__global__ void __launch_bounds__(kThreads) lago_orientation_blocks_kernel(
    int n_edges, int anchor, const int* __restrict__ from, const int* __restrict__ to, const double* __restrict__ meas,
    const double* __restrict__ sigma, const unsigned char* __restrict__ is_chord, const double* __restrict__ theta_root,
    const int64_t* __restrict__ block_off, double* __restrict__ blocks, double* __restrict__ reg) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n_edges) return;
  const int k1 = from[e], k2 = to[e];
  double dtheta = meas[3 * (int64_t)e + 2];
  if (is_chord[e]) {
    const double k2pi_noise = dtheta + theta_root[k1] - theta_root[k2];
    const double k = round(k2pi_noise / (2 * M_PI));
    dtheta = dtheta - 2 * k * M_PI;
  }
  if (reg) reg[e] = dtheta;
  if (!blocks) return;
  const double w = 1.0 / sigma[3 * (int64_t)e + 2];
  double* B = blocks + block_off[e];
  if (k1 == anchor) {
    B[0] = w;
    B[1] = w * dtheta;
  } else {
    B[0] = -w;
    B[1] = w;
    B[2] = w * dtheta;
  }
}

// theta of a node from the solution of the orientation system: the anchor and a pose no used factor holds have none
__device__ __forceinline__ double node_theta(int node, const int* __restrict__ theta_var, const double* __restrict__ theta) {
  const int v = theta_var[node];
  return v < 0 ? 0.0 : theta[v];
}

// One thread per edge: the whitened 3 x 7 block [J1 J2 | b] of computePoses (:322-348) at blocks + 21 e, column-major.
// J1 = -I with J1(0,2) = s1 dx + c1 dy, J1(1,2) = -c1 dx + s1 dy; J2 = I; b = (c1 dx - s1 dy, s1 dx + c1 dy,
// Rot2(theta2 - theta1 - theta_meas).theta()); row r is multiplied by 1 / sigma_r.  56 B read, 16 B gathered, 168 B
// written per edge.
__global__ void __launch_bounds__(kThreads) lago_pose_blocks_kernel(int n_edges, const int* __restrict__ from,
                                                                    const int* __restrict__ to,
                                                                    const double* __restrict__ meas,
                                                                    const double* __restrict__ sigma,
                                                                    const int* __restrict__ theta_var,
                                                                    const double* __restrict__ theta,
                                                                    double* __restrict__ blocks) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n_edges) return;
  const double theta1 = node_theta(from[e], theta_var, theta), theta2 = node_theta(to[e], theta_var, theta);
  const double s1 = sin(theta1), c1 = cos(theta1);
  const double dx = meas[3 * (int64_t)e], dy = meas[3 * (int64_t)e + 1];
  double linearDeltaRot = theta2 - theta1 - meas[3 * (int64_t)e + 2];
  linearDeltaRot = atan2(sin(linearDeltaRot), cos(linearDeltaRot));  // Rot2(.).theta()
  const double w0 = 1.0 / sigma[3 * (int64_t)e], w1 = 1.0 / sigma[3 * (int64_t)e + 1], w2 = 1.0 / sigma[3 * (int64_t)e + 2];
  double* B = blocks + 21 * (int64_t)e;
  for (int k = 0; k < 21; ++k) B[k] = 0.0;
  B[0] = -w0;                       // J1
  B[4] = -w1;
  B[6] = w0 * (s1 * dx + c1 * dy);
  B[7] = w1 * (-c1 * dx + s1 * dy);
  B[8] = -w2;
  B[9] = w0;                        // J2
  B[13] = w1;
  B[17] = w2;
  B[18] = w0 * (c1 * dx - s1 * dy);  // b
  B[19] = w1 * (s1 * dx + c1 * dy);
  B[20] = w2 * linearDeltaRot;
}

// One thread per POSE2 variable that a used factor holds: its state (x, y, theta) in the packed Values.  With pose != NULL
// (x, y) are the solved ones and theta = theta_lago + dtheta (:366-367); without, (x, y) stay what the Values hold and
// theta = theta_lago (:402-404).  The state keeps the angle as Pose2(x, y, theta).theta() returns it: atan2(sin, cos).
__global__ void __launch_bounds__(kThreads) lago_compose_kernel(int n_poses, const int* __restrict__ theta_var,
                                                                const double* __restrict__ theta,
                                                                const int* __restrict__ pose_var,
                                                                const double* __restrict__ pose,
                                                                const int* __restrict__ state_off,
                                                                double* __restrict__ values) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_poses) return;
  const int v = theta_var[i];
  if (v < 0) return;
  double t = theta[v];
  double* s = values + state_off[i];
  if (pose) {
    const double* p = pose + 3 * (int64_t)pose_var[i];
    s[0] = p[0];
    s[1] = p[1];
    t = t + p[2];
  }
  s[2] = atan2(sin(t), cos(t));
}

// what one lago call keeps on the device between its stages
struct LagoDevice {
  Dev<int> from, to, theta_var;
  Dev<double> meas, sigma, theta;  // theta: the solution of the orientation system, one double per variable of it
  Dev<unsigned char> is_chord;
  std::vector<int> var_of_node;    // node -> variable of the orientation system (-1: none)
  int n_theta = 0;
};

gsx_status upload_graph(const LagoGraph& G, hipStream_t stream, LagoDevice& L) {
  HIPTRY(L.from.upload(G.from, stream));
  HIPTRY(L.to.upload(G.to, stream));
  HIPTRY(L.meas.upload(G.meas, stream));
  HIPTRY(L.sigma.upload(G.sigma, stream));
  std::vector<unsigned char> chord(G.is_chord.begin(), G.is_chord.end());
  HIPTRY(L.is_chord.upload(chord, stream));
  return GSX_OK;
}

// computeThetasToRoot on the device: up[n] (a root: itself), delta[n]; ceil(log2(max_depth + 1)) rounds enqueued back to
// back.  *result points at the sums of the last round (inside sum_a or sum_b).
struct JumpBuffers {
  Dev<int> anc_a, anc_b;
  Dev<double> sum_a, sum_b;
};
gsx_status thetas_to_root_device(const std::vector<int>& up, const std::vector<double>& delta, int max_depth,
                                 hipStream_t stream, JumpBuffers& J, const double** result) {
  const int n = (int)up.size();
  HIPTRY(J.anc_a.upload(up, stream));
  HIPTRY(J.sum_a.upload(delta, stream));
  HIPTRY(J.anc_b.alloc(up.size()));
  HIPTRY(J.sum_b.alloc(up.size()));
  int rounds = 0;
  while (((int64_t)1 << rounds) < (int64_t)max_depth + 1) ++rounds;
  int *anc_in = J.anc_a.p, *anc_out = J.anc_b.p;
  double *sum_in = J.sum_a.p, *sum_out = J.sum_b.p;
  for (int r = 0; r < rounds && n > 0; ++r) {
    hipLaunchKernelGGL(lago_theta_to_root_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, n, anc_in, sum_in, anc_out,
                       sum_out);
    std::swap(anc_in, anc_out);
    std::swap(sum_in, sum_out);
  }
  HIPTRY(hipGetLastError());
  *result = sum_in;
  return GSX_OK;
}

std::vector<int> up_links(const LagoGraph& G) {
  std::vector<int> up(G.n_poses + 1);
  for (int n = 0; n <= G.n_poses; ++n) up[n] = G.parent[n] < 0 ? n : G.parent[n];
  return up;
}

// the orientation stage (computeOrientations, :264-294): L.theta = the solution on the device
gsx_status orientations_device(const gsx_problem_desc* desc, const LagoGraph& G, int32_t device, LagoDevice& L) {
  const int ne = (int)G.from.size();
  OwnedDesc D;
  const auto t_analysis = std::chrono::steady_clock::now();
  lower_lago_orientations(desc, G, D, L.var_of_node);
  Handle H;
  gsx_status st = create_ordered(D, device, H);
  if (st != GSX_OK) return st;
  g_timings[TL_ORIENTATION_ANALYSIS] = host_ms_since(t_analysis);
  const HostProblem& P = handle_problem(H.h);
  if ((int)P.f_jac_off.size() != ne + 1 || P.tan_size != (int64_t)D.keys.size()) return GSX_E_STATE;
  for (int e = 0; e < ne; ++e)  // (the layout the blocks kernel writes)
    if (P.f_jac_off[e + 1] - P.f_jac_off[e] != (G.from[e] == G.n_poses ? 2 : 3)) return GSX_E_STATE;
  hipStream_t stream = (hipStream_t)handle_stream(H.h);
  L.n_theta = (int)D.keys.size();
  std::vector<double> zeros((size_t)P.state_size, 0.0);
  st = gsx_set_values(H.h, zeros.data(), P.state_size);
  if (st != GSX_OK) return st;
  st = upload_graph(G, stream, L);
  if (st != GSX_OK) return st;
  HIPTRY(L.theta_var.upload(L.var_of_node, stream));
  HIPTRY(L.theta.alloc((size_t)L.n_theta));
  Dev<int64_t> d_off;
  std::vector<int64_t> off(P.f_jac_off.begin(), P.f_jac_off.begin() + ne);
  HIPTRY(d_off.upload(off, stream));
  EventPair ev_root, ev_blocks, ev_solve;
  JumpBuffers J;
  const double* d_root = nullptr;
  ev_root.begin(stream);
  st = thetas_to_root_device(up_links(G), G.delta, G.max_depth, stream, J, &d_root);
  if (st != GSX_OK) return st;
  ev_root.end();
  ev_blocks.begin(stream);
  hipLaunchKernelGGL(lago_orientation_blocks_kernel, dim3(blocks_for(ne)), dim3(kThreads), 0, stream, ne, G.n_poses, L.from.p,
                     L.to.p, L.meas.p, L.sigma.p, L.is_chord.p, d_root, d_off.p, handle_jacobian_pool(H.h), (double*)nullptr);
  ev_blocks.end();
  HIPTRY(hipGetLastError());
  handle_blocks_written(H.h);
  ev_solve.begin(stream);
  uint64_t bad = 0;
  st = gsx_solve(H.h, 0.0, 0, 0.0, 0.0, nullptr, 0, &bad);
  if (st != GSX_OK) return st;
  HIPTRY(hipMemcpyAsync(L.theta.p, handle_delta(H.h), (size_t)L.n_theta * sizeof(double), hipMemcpyDeviceToDevice, stream));
  ev_solve.end();
  HIPTRY(hipStreamSynchronize(stream));  // (the handle and the jump buffers go with this frame)
  g_timings[TL_THETA_TO_ROOT] = ev_root.ms();
  g_timings[TL_ORIENTATION_BLOCKS] = ev_blocks.ms();
  g_timings[TL_ORIENTATION_SOLVE] = ev_solve.ms();
  return GSX_OK;
}

std::vector<int> pose_state_offsets(const gsx_problem_desc* desc, const LagoGraph& G) {
  std::vector<int> all, off(G.n_poses);
  desc_state_size(desc, &all);
  for (int n = 0; n < G.n_poses; ++n) off[n] = all[G.pose_var[n]];
  return off;
}

// the pose stage (computePoses, :308-372); d_values: packed Values of desc on the device, only the touched poses are written
gsx_status poses_device(const gsx_problem_desc* desc, const LagoGraph& G, int32_t device, const LagoDevice& L,
                        double* d_values) {
  const int ne = (int)G.from.size();
  OwnedDesc D;
  std::vector<int> var_of_node;
  const auto t_analysis = std::chrono::steady_clock::now();
  lower_lago_poses(desc, G, D, var_of_node);
  Handle H;
  gsx_status st = create_ordered(D, device, H);
  if (st != GSX_OK) return st;
  g_timings[TL_POSE_ANALYSIS] = host_ms_since(t_analysis);
  const HostProblem& P = handle_problem(H.h);
  if ((int)P.f_jac_off.size() != ne + 2 || P.tan_size != 3 * (int64_t)D.keys.size()) return GSX_E_STATE;
  for (int e = 0; e <= ne; ++e)
    if (P.f_jac_off[e] != 21 * (int64_t)e) return GSX_E_STATE;  // (the layout the blocks kernel writes)
  hipStream_t stream = (hipStream_t)handle_stream(H.h);
  std::vector<double> zeros((size_t)P.state_size, 0.0);
  st = gsx_set_values(H.h, zeros.data(), P.state_size);
  if (st != GSX_OK) return st;
  Dev<int> d_pose_var, d_state_off;
  HIPTRY(d_pose_var.upload(var_of_node, stream));
  HIPTRY(d_state_off.upload(pose_state_offsets(desc, G), stream));
  EventPair ev_blocks, ev_solve, ev_compose;
  ev_blocks.begin(stream);
  hipLaunchKernelGGL(lago_pose_blocks_kernel, dim3(blocks_for(ne)), dim3(kThreads), 0, stream, ne, L.from.p, L.to.p,
                     L.meas.p, L.sigma.p, L.theta_var.p, L.theta.p, handle_jacobian_pool(H.h));
  ev_blocks.end();
  HIPTRY(hipGetLastError());
  handle_blocks_written(H.h);
  ev_solve.begin(stream);
  uint64_t bad = 0;
  st = gsx_solve(H.h, 0.0, 0, 0.0, 0.0, nullptr, 0, &bad);
  if (st != GSX_OK) return st;
  ev_solve.end();
  ev_compose.begin(stream);
  hipLaunchKernelGGL(lago_compose_kernel, dim3(blocks_for(G.n_poses)), dim3(kThreads), 0, stream, G.n_poses, L.theta_var.p,
                     L.theta.p, d_pose_var.p, (const double*)handle_delta(H.h), d_state_off.p, d_values);
  ev_compose.end();
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(stream));
  g_timings[TL_POSE_BLOCKS] = ev_blocks.ms();
  g_timings[TL_POSE_SOLVE] = ev_solve.ms();
  g_timings[TL_COMPOSE] = ev_compose.ms();
  return GSX_OK;
}

// the checks every entry point makes before a device is touched
gsx_status host_stage(const gsx_problem_desc* desc, bool use_odometric_path, LagoGraph& G) {
  std::string err;
  gsx_status st = build_lago_graph(desc, G, err);
  if (st != GSX_OK) return st;
  return lago_tree(G, use_odometric_path, err);
}

// lago::initialize (:375-409); with_guess: (x, y) of `given` are kept
gsx_status initialize_common(const gsx_problem_desc* desc, bool use_odometric_path, bool with_guess, const double* given,
                             int64_t n_given, int32_t device, double* values_out, int64_t n_out) {
  LagoGraph G;
  gsx_status st = host_stage(desc, use_odometric_path, G);
  if (st != GSX_OK) return st;
  const int64_t n_state = desc_state_size(desc, nullptr);
  if (n_out != n_state || (n_out > 0 && !values_out)) return GSX_E_INVALID;
  if (given && n_given != n_state) return GSX_E_INVALID;
  // what the reference leaves out of its result is copied from the guess: there must be one
  if (!given && (with_guess || !G.all_touched || G.n_poses != desc->n_vars)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TL_COUNT, 0.0);
  if (!G.anchored) return GSX_E_INDETERMINATE;
  if (given) std::memcpy(values_out, given, (size_t)n_state * sizeof(double));
  if (G.from.empty()) return GSX_OK;
  LagoDevice L;
  st = orientations_device(desc, G, device, L);
  if (st != GSX_OK) return st;
  Dev<double> d_values;
  HIPTRY(d_values.alloc((size_t)n_state));
  if (given)
    HIPTRY(hipMemcpy(d_values.p, given, (size_t)n_state * sizeof(double), hipMemcpyHostToDevice));
  else
    HIPTRY(hipMemset(d_values.p, 0, (size_t)n_state * sizeof(double)));
  if (with_guess) {
    Stream S;
    HIPTRY(hipStreamCreate(&S.s));
    Dev<int> d_state_off;
    HIPTRY(d_state_off.upload(pose_state_offsets(desc, G), S.s));
    EventPair ev_compose;
    ev_compose.begin(S.s);
    hipLaunchKernelGGL(lago_compose_kernel, dim3(blocks_for(G.n_poses)), dim3(kThreads), 0, S.s, G.n_poses, L.theta_var.p,
                       L.theta.p, (const int*)nullptr, (const double*)nullptr, d_state_off.p, d_values.p);
    ev_compose.end();
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(S.s));
    g_timings[TL_COMPOSE] = ev_compose.ms();
  } else {
    st = poses_device(desc, G, device, L, d_values.p);
    if (st != GSX_OK) return st;
  }
  HIPTRY(hipMemcpy(values_out, d_values.p, (size_t)n_state * sizeof(double), hipMemcpyDeviceToHost));
  return GSX_OK;
}

}  // namespace

extern "C" {

gsx_status gsx_lago_initialize(const gsx_problem_desc* desc, int32_t use_odometric_path, const double* given,
                               int64_t n_given, int32_t device, double* values_out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_lago_initialize") != GSX_OK) return GSX_E_INVALID;
  return initialize_common(desc, use_odometric_path != 0, false, given, n_given, device, values_out, n_out);
}

gsx_status gsx_lago_initialize_with_guess(const gsx_problem_desc* desc, const double* given, int64_t n_given, int32_t device,
                                          double* values_out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_lago_initialize_with_guess") != GSX_OK) return GSX_E_INVALID;
  return initialize_common(desc, true, true, given, n_given, device, values_out, n_out);
}

gsx_status gsx_lago_initialize_orientations(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t device,
                                            double* theta_out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_lago_initialize_orientations") != GSX_OK) return GSX_E_INVALID;
  LagoGraph G;
  gsx_status st = host_stage(desc, use_odometric_path != 0, G);
  if (st != GSX_OK) return st;
  if (n_out != (int64_t)G.n_poses || (n_out > 0 && !theta_out)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TL_COUNT, 0.0);
  if (!G.anchored) return GSX_E_INDETERMINATE;
  std::fill(theta_out, theta_out + n_out, 0.0);  // (what a pose no used factor holds gets)
  if (G.from.empty()) return GSX_OK;
  LagoDevice L;
  st = orientations_device(desc, G, device, L);
  if (st != GSX_OK) return st;
  std::vector<double> theta((size_t)L.n_theta);
  HIPTRY(hipMemcpy(theta.data(), L.theta.p, theta.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int n = 0; n < G.n_poses; ++n)
    if (L.var_of_node[n] >= 0) theta_out[n] = theta[L.var_of_node[n]];
  return GSX_OK;
}

gsx_status gsx_lago_thetas_to_root(const int32_t* parent, const double* delta, int64_t n, int32_t device, double* out) {
  if (n < 0 || n > INT32_MAX || (n > 0 && (!parent || !delta || !out))) return GSX_E_INVALID;
  std::vector<int> depth;
  int max_depth = 0;
  if (!forest_depths(parent, n, depth, &max_depth)) return GSX_E_INVALID;
  gsx_status st = check_device(device);
  if (st != GSX_OK) return st;
  if (n == 0) return GSX_OK;
  std::vector<int> up(parent, parent + n);
  std::vector<double> d(delta, delta + n);
  for (int64_t i = 0; i < n; ++i)
    if (up[i] == i) d[i] = 0.0;  // the root is assumed to have orientation zero (:54)
  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  JumpBuffers J;
  const double* d_root = nullptr;
  st = thetas_to_root_device(up, d, max_depth, S.s, J, &d_root);
  if (st != GSX_OK) return st;
  HIPTRY(hipMemcpyAsync(out, d_root, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipStreamSynchronize(S.s));
  return GSX_OK;
}

gsx_status gsx_lago_regularized_measurements(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t device,
                                             double* out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_lago_regularized_measurements") != GSX_OK) return GSX_E_INVALID;
  LagoGraph G;
  gsx_status st = host_stage(desc, use_odometric_path != 0, G);
  if (st != GSX_OK) return st;
  const int ne = (int)G.from.size();
  if (n_out != (int64_t)ne || (n_out > 0 && !out)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  if (ne == 0) return GSX_OK;
  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  LagoDevice L;
  st = upload_graph(G, S.s, L);
  if (st != GSX_OK) return st;
  Dev<double> d_reg;
  HIPTRY(d_reg.alloc((size_t)ne));
  JumpBuffers J;
  const double* d_root = nullptr;
  st = thetas_to_root_device(up_links(G), G.delta, G.max_depth, S.s, J, &d_root);
  if (st != GSX_OK) return st;
  hipLaunchKernelGGL(lago_orientation_blocks_kernel, dim3(blocks_for(ne)), dim3(kThreads), 0, S.s, ne, G.n_poses, L.from.p,
                     L.to.p, L.meas.p, L.sigma.p, L.is_chord.p, d_root, (const int64_t*)nullptr, (double*)nullptr, d_reg.p);
  HIPTRY(hipGetLastError());
  HIPTRY(hipMemcpyAsync(out, d_reg.p, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipStreamSynchronize(S.s));
  return GSX_OK;
}

gsx_status gsx_lago_timings(double* out_ms, int32_t n) {
  if (!out_ms || n != TL_COUNT) return GSX_E_INVALID;
  std::copy(g_timings, g_timings + TL_COUNT, out_ms);
  return GSX_OK;
}

}  // extern "C"
