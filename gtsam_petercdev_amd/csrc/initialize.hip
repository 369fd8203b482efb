// initialize.hip — device part of the Pose3 initializer (gtsam/slam/InitializePose3.cpp, gtsam/slam/InitializePose.h) and
// its C ABI (include/gsx.h).  The host lowering is init_graph.cpp, the per-rotation arithmetic init_math.h.
//   chordal_blocks_kernel      the whitened 3 x 7 blocks [-w I, w Rij | 0] of the decoupled relaxed system (:37-71)
//   closest_rotation_kernel    normalizeRelaxedRotations (:75-92) = Rot3::ClosestTo (SO3.cpp:202-208) per pose
//   tron_gradient_kernel       the node gradients of computeOrientationsGradient (:158-188, gradientTron :256-275)
//   tron_update_kernel         its retraction and stopping test (:190-201)
//   pose_states_kernel         the initial Values of computePoses (InitializePose.h:61-74)
// Product code: no CPU fallback — every numeric entry point returns GSX_E_NO_DEVICE without a usable GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gsx_internal.h"
#include "init_device.h"
#include "init_math.h"

using namespace gsx;
using namespace gsx::initdev;

namespace {

constexpr int kBatch = 32;  // gradient iterations queued between two read-backs of the stop word

// stage times of the last initializer call of the process (gsx_pose3_init_timings): host milliseconds for the two
// analyses, HIP events on the internal handle's stream for the device stages
enum { TM_RELAXED_ANALYSIS, TM_BLOCKS, TM_SOLVES, TM_PROJECTION, TM_ANCHOR_ANALYSIS, TM_GAUSS_NEWTON, TM_GRADIENT,
       TM_GRADIENT_ITERATIONS, TM_COUNT };
double g_timings[TM_COUNT] = {};

// One thread per edge of non-zero weight: its block of the relaxed system, 3 x 7 column-major at 21 e, straight from the 9
// doubles of the measured rotation.  Isotropic::Precision(9, p) is Sigma(sqrt(1 / p)) (NoiseModel.h:577-579, :566-569):
// whitening multiplies by 1 / sqrt(1 / p).
__global__ void __launch_bounds__(kThreads) chordal_blocks_kernel(int n_edges, const int* __restrict__ edges,
                                                                  const double* __restrict__ rot,
                                                                  const double* __restrict__ weight,
                                                                  double* __restrict__ blocks) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_edges) return;
  const int e = edges[i];
  const double w = 1.0 / sqrt(1.0 / weight[e]);
  const double* R = rot + 9 * (int64_t)e;
  double* B = blocks + 21 * (int64_t)i;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      B[3 * c + r] = (r == c) ? -w : 0.0;      // -I on the first key
      B[9 + 3 * c + r] = w * R[3 * r + c];     // Rij on the second
    }
  B[18] = B[19] = B[20] = 0.0;
}

// One thread per matrix.  Row k of matrix p is the three doubles at src + off(p) + k * chunk_stride, where off(p) =
// 3 * var[p] (the solved rows of a pose: the three solutions lie chunk_stride apart) or 9 * p (var == NULL: matrices given
// directly, chunk_stride = 3).  The reference maps the 9-vector column-major and transposes (:84-87), so the solved chunk
// k IS row k of the matrix handed to ClosestTo.
__global__ void __launch_bounds__(kThreads) closest_rotation_kernel(int64_t n, const double* __restrict__ src,
                                                                    const int* __restrict__ var, int64_t chunk_stride,
                                                                    const int64_t* __restrict__ dst_index,
                                                                    double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const double* s = src + (var ? 3 * (int64_t)var[p] : 9 * p);
  double M[9], R[9];
  for (int k = 0; k < 3; ++k)
    for (int c = 0; c < 3; ++c) M[3 * k + c] = s[k * chunk_stride + c];
  initm::closest_rotation(M, R);
  double* o = out + 9 * (dst_index ? dst_index[p] : p);
  for (int i = 0; i < 9; ++i) o[i] = R[i];
}

// words of the gradient iterations' control block
struct TronCtl {
  int stop_it;                          // the iteration after whose update the loop stopped; INT_MAX: still running
  int pad;
  unsigned long long max_grad[kBatch];  // bit pattern of the iteration's largest gradient norm (slot it % kBatch)
};

// One thread per node, anchor included: the sum of gradientTron over its incident edges in adjacency order, from the
// rotations of the previous iteration; grad = stepsize * sum.  The norm of the UNSCALED sum goes into the iteration's
// maximum: a non-negative double orders like its bit pattern, and a NaN is skipped as `>` skips it in the reference.
__global__ void __launch_bounds__(kThreads) tron_gradient_kernel(int n_nodes, int it, const int* __restrict__ adj_ptr,
                                                                 const int* __restrict__ adj, const int* __restrict__ from,
                                                                 const int* __restrict__ to, const double* __restrict__ rot,
                                                                 const double* __restrict__ inv, double a, double b,
                                                                 double stepsize, double* __restrict__ grad, TronCtl* ctl) {
  if (ctl->stop_it < it) return;  // (written by the update of an EARLIER iteration: stream order)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double norm = 0.0;
  if (i < n_nodes) {
    double Ri[9];
    for (int k = 0; k < 9; ++k) Ri[k] = inv[9 * (int64_t)i + k];
    double g[3] = {0.0, 0.0, 0.0};
    for (int q = adj_ptr[i]; q < adj_ptr[i + 1]; ++q) {
      const int e = adj[q];
      const double* Rij = rot + 9 * (int64_t)e;
      double Rj[9], R2[9], ge[3];
      if (from[e] == i) {  // key == keys[0]: Rij * Rj
        for (int k = 0; k < 9; ++k) Rj[k] = inv[9 * (int64_t)to[e] + k];
        initm::mat_mul(Rij, Rj, R2);
      } else {             // key == keys[1]: Rij.between(Rj) = Rij' Rj
        for (int k = 0; k < 9; ++k) Rj[k] = inv[9 * (int64_t)from[e] + k];
        initm::mat_tmul(Rij, Rj, R2);
      }
      initm::gradient_tron(Ri, R2, a, b, ge);
      g[0] = g[0] + ge[0]; g[1] = g[1] + ge[1]; g[2] = g[2] + ge[2];
    }
    grad[3 * (int64_t)i] = stepsize * g[0];
    grad[3 * (int64_t)i + 1] = stepsize * g[1];
    grad[3 * (int64_t)i + 2] = stepsize * g[2];
    norm = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  }
  // largest norm of the wave, then one atomic per wave
  unsigned long long bits = (norm == norm) ? (unsigned long long)__double_as_longlong(norm) : 0ull;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(bits, off, 64);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits != 0ull) atomicMax(&ctl->max_grad[it % kBatch], bits);
}

// One thread per node: Ri = Ri.retract(grad) with the full exponential map (Rot3::ChartAtOrigin::Retract in EXPMAP mode,
// Rot3M.cpp:202-207).  Thread 0 evaluates the stopping test of iteration `it` (:200): the maximum is complete, its kernel
// ended before this one started.  stop_it = it does not stop THIS launch (every thread tests stop_it < it).
__global__ void __launch_bounds__(kThreads) tron_update_kernel(int n_nodes, int it, const double* __restrict__ grad,
                                                               double* __restrict__ inv, TronCtl* ctl) {
  if (ctl->stop_it < it) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n_nodes) {
    double R[9], E[9], T[9];
    for (int k = 0; k < 9; ++k) R[k] = inv[9 * (int64_t)i + k];
    const double w[3] = {grad[3 * (int64_t)i], grad[3 * (int64_t)i + 1], grad[3 * (int64_t)i + 2]};
    initm::so3_exp(w, E);
    initm::mat_mul(R, E, T);
    for (int k = 0; k < 9; ++k) inv[9 * (int64_t)i + k] = T[k];
  }
  if (i == 0) {
    const double max_grad = __longlong_as_double((long long)ctl->max_grad[it % kBatch]);
    if (it > 20 && max_grad < 5e-3) ctl->stop_it = it;
  }
}

// inverse rotations of the given guess (:122-129); the anchor (node n_poses) starts at the identity
__global__ void __launch_bounds__(kThreads) tron_init_kernel(int n_poses, const int* __restrict__ state_off,
                                                             const double* __restrict__ given, double* __restrict__ inv) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i > n_poses) return;
  double R[9], T[9];
  if (i == n_poses) {
    initm::mat_identity(T);
  } else {
    for (int k = 0; k < 9; ++k) R[k] = given[state_off[i] + k];
    initm::mat_transpose(R, T);
  }
  for (int k = 0; k < 9; ++k) inv[9 * (int64_t)i + k] = T[k];
}

// R.inverse(), or Rref.compose(R.inverse()) with Rref = the anchor's inverse rotation (:204-217)
__global__ void __launch_bounds__(kThreads) tron_output_kernel(int n_poses, int set_ref_frame, const double* __restrict__ inv,
                                                               double* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_poses) return;
  double R[9], T[9], O[9];
  for (int k = 0; k < 9; ++k) R[k] = inv[9 * (int64_t)i + k];
  initm::mat_transpose(R, T);
  if (set_ref_frame) {
    double Rref[9];
    for (int k = 0; k < 9; ++k) Rref[k] = inv[9 * (int64_t)n_poses + k];
    initm::mat_mul(Rref, T, O);
  } else {
    for (int k = 0; k < 9; ++k) O[k] = T[k];
  }
  for (int k = 0; k < 9; ++k) out[9 * (int64_t)i + k] = O[k];
}

// One thread per variable of the anchor graph: Pose3(rot, origin), the anchor Pose3() (InitializePose.h:61-74).
// node_of_var[v] = node (n_poses: the anchor); rot is indexed by node.
__global__ void __launch_bounds__(kThreads) pose_states_kernel(int n_vars, int n_poses, const int* __restrict__ node_of_var,
                                                               const double* __restrict__ rot, double* __restrict__ values) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vars) return;
  const int node = node_of_var[v];
  double* s = values + 12 * (int64_t)v;
  for (int k = 0; k < 9; ++k) s[k] = node == n_poses ? ((k % 4 == 0) ? 1.0 : 0.0) : rot[9 * (int64_t)node + k];
  s[9] = s[10] = s[11] = 0.0;
}

// computeOrientationsChordal on the device; d_rot: 9 doubles per NODE (anchor excluded), device memory; the entries of
// untouched nodes are left alone
gsx_status chordal_device(const gsx_problem_desc* desc, const PoseGraph& G, int32_t device, double* d_rot) {
  if (!G.anchored) return GSX_E_INDETERMINATE;
  OwnedDesc D;
  std::vector<int> var_of_node, edges;
  const auto t_analysis = std::chrono::steady_clock::now();
  lower_relaxed(desc, G, D, var_of_node, edges);
  const int ne = (int)edges.size();
  Handle H;
  gsx_status st = create_ordered(D, device, H);
  if (st != GSX_OK) return st;
  g_timings[TM_RELAXED_ANALYSIS] = host_ms_since(t_analysis);
  EventPair ev_blocks, ev_solves, ev_projection;
  const HostProblem& P = handle_problem(H.h);
  for (int e = 0; e <= ne; ++e)
    if (P.f_jac_off[e] != 21 * (int64_t)e) return GSX_E_STATE;  // (the layout the blocks kernel writes)
  hipStream_t stream = (hipStream_t)handle_stream(H.h);
  const int64_t nt = P.tan_size;  // 3 per variable
  std::vector<double> zeros((size_t)P.state_size, 0.0);
  st = gsx_set_values(H.h, zeros.data(), P.state_size);
  if (st != GSX_OK) return st;
  Dev<int> d_edges, d_var;
  Dev<double> d_erot, d_w, d_sol;
  Dev<int64_t> d_dst;
  HIPTRY(d_edges.upload(edges, stream));
  HIPTRY(d_erot.upload(G.rot, stream));
  HIPTRY(d_w.upload(G.weight, stream));
  HIPTRY(d_sol.alloc(3 * (size_t)nt));
  double* blocks = handle_jacobian_pool(H.h);
  ev_blocks.begin(stream);
  if (ne > 0)
    hipLaunchKernelGGL(chordal_blocks_kernel, dim3(blocks_for(ne)), dim3(kThreads), 0, stream, ne, d_edges.p, d_erot.p,
                       d_w.p, blocks);
  ev_blocks.end();
  HIPTRY(hipGetLastError());
  ev_solves.begin(stream);
  for (int k = 0; k < 3; ++k) {
    // the anchor prior's right-hand side e_k: column 3 of its 3 x 4 block
    double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    HIPTRY(hipMemcpyAsync(blocks + 21 * (int64_t)ne + 9, ek, sizeof(ek), hipMemcpyHostToDevice, stream));
    HIPTRY(hipStreamSynchronize(stream));  // (ek lives on this frame)
    handle_blocks_written(H.h);
    uint64_t bad = 0;
    st = gsx_solve(H.h, 0.0, 0, 0.0, 0.0, nullptr, 0, &bad);
    if (st != GSX_OK) return st;
    HIPTRY(hipMemcpyAsync(d_sol.p + k * nt, handle_delta(H.h), (size_t)nt * sizeof(double), hipMemcpyDeviceToDevice, stream));
  }
  ev_solves.end();
  // the touched nodes: their variable in the internal problem and their slot in d_rot
  std::vector<int> var;
  std::vector<int64_t> dst;
  for (int n = 0; n < G.n_poses; ++n)
    if (var_of_node[n] >= 0) {
      var.push_back(var_of_node[n]);
      dst.push_back(n);
    }
  HIPTRY(d_var.upload(var, stream));
  HIPTRY(d_dst.upload(dst, stream));
  ev_projection.begin(stream);
  if (!var.empty())
    hipLaunchKernelGGL(closest_rotation_kernel, dim3(blocks_for((int64_t)var.size())), dim3(kThreads), 0, stream,
                       (int64_t)var.size(), d_sol.p, d_var.p, nt, d_dst.p, d_rot);
  ev_projection.end();
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(stream));
  g_timings[TM_BLOCKS] = ev_blocks.ms();
  g_timings[TM_SOLVES] = ev_solves.ms();
  g_timings[TM_PROJECTION] = ev_projection.ms();
  return GSX_OK;
}

// computeOrientationsGradient on the device; d_given: packed Values of desc; d_rot: 9 doubles per node (anchor excluded)
gsx_status gradient_device(const gsx_problem_desc* desc, const PoseGraph& G, const double* d_given, int max_iter,
                           int set_ref_frame, hipStream_t stream, double* d_rot, int32_t* iterations) {
  const int n_nodes = G.n_poses + 1;
  std::vector<int> state_off_all, state_off(G.n_poses);
  desc_state_size(desc, &state_off_all);
  for (int n = 0; n < G.n_poses; ++n) state_off[n] = state_off_all[G.pose_var[n]];
  // maximum node degree, anchor included, and the step size (:137-152)
  size_t maxNodeDeg = 0;
  for (int n = 0; n < n_nodes; ++n) maxNodeDeg = std::max<size_t>(maxNodeDeg, (size_t)(G.adj_ptr[n + 1] - G.adj_ptr[n]));
  const double b = 1;
  const double f0 = 1 / b - (1 / b + M_PI) * exp(-b * M_PI);
  const double a = (M_PI * M_PI) / (2 * f0);
  const double rho = 2 * a * b;
  const double mu_max = maxNodeDeg * rho;
  const double stepsize = 2 / mu_max;
  Dev<int> d_state_off, d_adj_ptr, d_adj, d_from, d_to;
  Dev<double> d_erot, d_inv, d_grad;
  Dev<TronCtl> d_ctl;
  HIPTRY(d_state_off.upload(state_off, stream));
  HIPTRY(d_adj_ptr.upload(G.adj_ptr, stream));
  HIPTRY(d_adj.upload(G.adj, stream));
  HIPTRY(d_from.upload(G.from, stream));
  HIPTRY(d_to.upload(G.to, stream));
  HIPTRY(d_erot.upload(G.rot, stream));
  HIPTRY(d_inv.alloc(9 * (size_t)n_nodes));
  HIPTRY(d_grad.alloc(3 * (size_t)n_nodes));
  HIPTRY(d_ctl.alloc(1));
  const dim3 grid(blocks_for(n_nodes)), block(kThreads);
  hipLaunchKernelGGL(tron_init_kernel, grid, block, 0, stream, G.n_poses, d_state_off.p, d_given, d_inv.p);
  TronCtl ctl0;
  std::memset(&ctl0, 0, sizeof(ctl0));
  ctl0.stop_it = INT_MAX;
  HIPTRY(hipMemcpyAsync(d_ctl.p, &ctl0, sizeof(ctl0), hipMemcpyHostToDevice, stream));
  HIPTRY(hipStreamSynchronize(stream));
  int executed = max_iter > 0 ? max_iter : 0;
  EventPair ev_gradient;
  ev_gradient.begin(stream);
  for (int it0 = 0; it0 < max_iter; it0 += kBatch) {
    HIPTRY(hipMemsetAsync(d_ctl.p->max_grad, 0, sizeof(ctl0.max_grad), stream));
    const int it1 = std::min(max_iter, it0 + kBatch);
    for (int it = it0; it < it1; ++it) {
      hipLaunchKernelGGL(tron_gradient_kernel, grid, block, 0, stream, n_nodes, it, d_adj_ptr.p, d_adj.p, d_from.p, d_to.p,
                         d_erot.p, d_inv.p, a, b, stepsize, d_grad.p, d_ctl.p);
      hipLaunchKernelGGL(tron_update_kernel, grid, block, 0, stream, n_nodes, it, d_grad.p, d_inv.p, d_ctl.p);
    }
    HIPTRY(hipGetLastError());
    int stop[2] = {INT_MAX, 0};  // one 8-byte read-back per batch
    HIPTRY(hipMemcpyAsync(stop, d_ctl.p, sizeof(stop), hipMemcpyDeviceToHost, stream));
    HIPTRY(hipStreamSynchronize(stream));
    if (stop[0] != INT_MAX) {
      executed = stop[0] + 1;
      break;
    }
  }
  ev_gradient.end();
  if (G.n_poses > 0)
    hipLaunchKernelGGL(tron_output_kernel, dim3(blocks_for(G.n_poses)), block, 0, stream, G.n_poses, set_ref_frame, d_inv.p,
                       d_rot);
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(stream));
  g_timings[TM_GRADIENT] = ev_gradient.ms();
  g_timings[TM_GRADIENT_ITERATIONS] = (double)executed;
  if (iterations) *iterations = executed;
  return GSX_OK;
}

// computePoses on the device; d_rot: 9 doubles per node; values_out: packed Values of desc (host), only the touched poses
// are written
gsx_status compute_poses_device(const gsx_problem_desc* desc, const PoseGraph& G, const double* d_rot, int single_iter,
                                int32_t device, double* values_out) {
  OwnedDesc D;
  std::vector<int> var_of_node;
  const auto t_analysis = std::chrono::steady_clock::now();
  lower_anchor_graph(desc, G, D, var_of_node);
  Handle H;
  gsx_status st = create_ordered(D, device, H);
  if (st != GSX_OK) return st;
  g_timings[TM_ANCHOR_ANALYSIS] = host_ms_since(t_analysis);
  EventPair ev_gn;
  const int nv = (int)D.keys.size();
  std::vector<int> node_of_var(nv, -1);
  for (int n = 0; n <= G.n_poses; ++n)
    if (var_of_node[n] >= 0) node_of_var[var_of_node[n]] = n;
  hipStream_t stream = (hipStream_t)handle_stream(H.h);
  Dev<int> d_node;
  HIPTRY(d_node.upload(node_of_var, stream));
  ev_gn.begin(stream);
  hipLaunchKernelGGL(pose_states_kernel, dim3(blocks_for(nv)), dim3(kThreads), 0, stream, nv, G.n_poses, d_node.p, d_rot,
                     handle_values(H.h));
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(stream));
  handle_values_written(H.h);
  // GaussNewtonParams: maxIterations 100, relativeErrorTol 1e-5, absoluteErrorTol 1e-5, errorTol 0
  // (NonlinearOptimizerParams.h:42-108); params.maxIterations = 1 with singleIter (InitializePose.h:78-83)
  st = gsx_gn_optimize(H.h, single_iter ? 1 : 100, 1e-5, 1e-5, 0.0, nullptr);
  if (st != GSX_OK) return st;
  ev_gn.end();
  g_timings[TM_GAUSS_NEWTON] = ev_gn.ms();
  std::vector<double> vals(12 * (size_t)nv);
  st = gsx_get_values(H.h, vals.data(), (int64_t)vals.size());
  if (st != GSX_OK) return st;
  std::vector<int> state_off;
  desc_state_size(desc, &state_off);
  for (int n = 0; n < G.n_poses; ++n)  // (the anchor is dropped, :88-95)
    if (var_of_node[n] >= 0)
      std::memcpy(values_out + state_off[G.pose_var[n]], vals.data() + 12 * (size_t)var_of_node[n], 12 * sizeof(double));
  return GSX_OK;
}

void identity_rotations(std::vector<double>& r, int n) {
  r.assign(9 * (size_t)n, 0.0);
  for (int i = 0; i < n; ++i) r[9 * (size_t)i] = r[9 * (size_t)i + 4] = r[9 * (size_t)i + 8] = 1.0;
}

}  // namespace

extern "C" {

gsx_status gsx_closest_rotations(const double* m, int64_t n, int32_t device, double* r_out) {
  if (n < 0 || (n > 0 && (!m || !r_out))) return GSX_E_INVALID;
  gsx_status st = check_device(device);
  if (st != GSX_OK) return st;
  if (n == 0) return GSX_OK;
  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  Dev<double> d_m, d_r;
  HIPTRY(d_m.alloc(9 * (size_t)n));
  HIPTRY(d_r.alloc(9 * (size_t)n));
  HIPTRY(hipMemcpyAsync(d_m.p, m, 9 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, S.s));
  hipLaunchKernelGGL(closest_rotation_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, S.s, n, d_m.p, (const int*)nullptr,
                     (int64_t)3, (const int64_t*)nullptr, d_r.p);
  HIPTRY(hipGetLastError());
  HIPTRY(hipMemcpyAsync(r_out, d_r.p, 9 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipStreamSynchronize(S.s));
  return GSX_OK;
}

gsx_status gsx_pose3_orientations_chordal(const gsx_problem_desc* desc, int32_t device, double* rot_out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_pose3_orientations_chordal") != GSX_OK) return GSX_E_INVALID;
  PoseGraph G;
  std::string err;
  gsx_status st = build_pose_graph(desc, G, err);
  if (st != GSX_OK) return st;
  if (n_out != 9 * (int64_t)G.n_poses || (n_out > 0 && !rot_out)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TM_COUNT, 0.0);
  std::vector<double> rot;
  identity_rotations(rot, G.n_poses);  // (what a pose no used factor holds keeps)
  Dev<double> d_rot;
  HIPTRY(d_rot.alloc(rot.size()));
  HIPTRY(hipMemcpy(d_rot.p, rot.data(), rot.size() * sizeof(double), hipMemcpyHostToDevice));
  st = chordal_device(desc, G, device, d_rot.p);
  if (st != GSX_OK) return st;
  HIPTRY(hipMemcpy(rot_out, d_rot.p, rot.size() * sizeof(double), hipMemcpyDeviceToHost));
  return GSX_OK;
}

gsx_status gsx_pose3_orientations_gradient(const gsx_problem_desc* desc, const double* given, int64_t n_given,
                                           int32_t max_iter, int32_t set_ref_frame, int32_t device, double* rot_out,
                                           int64_t n_out, int32_t* iterations) {
  if (gsx::enter_call(desc, "gsx_pose3_orientations_gradient") != GSX_OK) return GSX_E_INVALID;
  PoseGraph G;
  std::string err;
  gsx_status st = build_pose_graph(desc, G, err);
  if (st != GSX_OK) return st;
  if (!given || n_given != desc_state_size(desc, nullptr) || max_iter < 0) return GSX_E_INVALID;
  if (n_out != 9 * (int64_t)G.n_poses || (n_out > 0 && !rot_out)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TM_COUNT, 0.0);
  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  Dev<double> d_given, d_rot;
  HIPTRY(d_given.alloc((size_t)n_given));
  HIPTRY(d_rot.alloc((size_t)n_out));
  HIPTRY(hipMemcpyAsync(d_given.p, given, (size_t)n_given * sizeof(double), hipMemcpyHostToDevice, S.s));
  st = gradient_device(desc, G, d_given.p, max_iter, set_ref_frame, S.s, d_rot.p, iterations);
  if (st != GSX_OK) return st;
  HIPTRY(hipMemcpy(rot_out, d_rot.p, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost));
  return GSX_OK;
}

gsx_status gsx_pose3_compute_poses(const gsx_problem_desc* desc, const double* rot, int64_t n_rot, int32_t single_iter,
                                   int32_t device, double* values_out, int64_t n_out) {
  if (gsx::enter_call(desc, "gsx_pose3_compute_poses") != GSX_OK) return GSX_E_INVALID;
  PoseGraph G;
  std::string err;
  gsx_status st = build_pose_graph(desc, G, err);
  if (st != GSX_OK) return st;
  if (n_rot != 9 * (int64_t)G.n_poses || (n_rot > 0 && !rot)) return GSX_E_INVALID;
  if (n_out != desc_state_size(desc, nullptr) || (n_out > 0 && !values_out)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TM_COUNT, 0.0);
  if (!G.anchored) return GSX_E_INDETERMINATE;
  Dev<double> d_rot;
  HIPTRY(d_rot.alloc((size_t)n_rot));
  HIPTRY(hipMemcpy(d_rot.p, rot, (size_t)n_rot * sizeof(double), hipMemcpyHostToDevice));
  return compute_poses_device(desc, G, d_rot.p, single_iter, device, values_out);
}

gsx_status gsx_initialize_pose3(const gsx_problem_desc* desc, const double* given, int64_t n_given,
                                const gsx_init_pose3_params* p, int32_t device, double* values_out, int64_t n_out,
                                int32_t* gradient_iterations) {
  if (gsx::enter_call(desc, "gsx_initialize_pose3") != GSX_OK) return GSX_E_INVALID;
  gsx_init_pose3_params prm;
  gsx_init_pose3_params_default(&prm);
  if (p) prm = *p;
  PoseGraph G;
  std::string err;
  gsx_status st = build_pose_graph(desc, G, err);
  if (st != GSX_OK) return st;
  const int64_t n_state = desc_state_size(desc, nullptr);
  if (n_out != n_state || (n_out > 0 && !values_out)) return GSX_E_INVALID;
  if (given && n_given != n_state) return GSX_E_INVALID;
  if (prm.use_gradient && (!given || prm.max_gradient_iterations < 0)) return GSX_E_INVALID;
  // what the reference leaves out of its result is copied from the guess: there must be one
  if (!given && (!G.all_touched || G.n_poses != desc->n_vars)) return GSX_E_INVALID;
  st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TM_COUNT, 0.0);
  if (!G.anchored) return GSX_E_INDETERMINATE;
  if (given) std::memcpy(values_out, given, (size_t)n_state * sizeof(double));
  if (gradient_iterations) *gradient_iterations = 0;
  Dev<double> d_rot;
  HIPTRY(d_rot.alloc(9 * (size_t)G.n_poses));
  if (prm.use_gradient) {
    Stream S;
    HIPTRY(hipStreamCreate(&S.s));
    Dev<double> d_given;
    HIPTRY(d_given.alloc((size_t)n_given));
    HIPTRY(hipMemcpyAsync(d_given.p, given, (size_t)n_given * sizeof(double), hipMemcpyHostToDevice, S.s));
    st = gradient_device(desc, G, d_given.p, prm.max_gradient_iterations, prm.set_ref_frame, S.s, d_rot.p,
                         gradient_iterations);
  } else {
    std::vector<double> rot;
    identity_rotations(rot, G.n_poses);
    HIPTRY(hipMemcpy(d_rot.p, rot.data(), rot.size() * sizeof(double), hipMemcpyHostToDevice));
    st = chordal_device(desc, G, device, d_rot.p);
  }
  if (st != GSX_OK) return st;
  return compute_poses_device(desc, G, d_rot.p, prm.single_iter, device, values_out);
}

gsx_status gsx_pose3_init_timings(double* out_ms, int32_t n) {
  if (!out_ms || n != TM_COUNT) return GSX_E_INVALID;
  std::copy(g_timings, g_timings + TM_COUNT, out_ms);
  return GSX_OK;
}

}  // extern "C"
