// mfas.hip — batched MFAS (minimum feedback arc set, gtsam/sfm/MFAS.cpp:36-171) on the device (gfx950, wave64): the
// outlier weights of one edge set under many 1-D projections at once.  One workgroup per projection direction; the
// adjacency (CSR over the unordered pairs) is built once on the host and shared by all directions — only the orientation
// of an edge (the sign of its weight) depends on the direction.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "init_device.h"

namespace gsx {
namespace {

using namespace initdev;

enum { TM_HOST = 0, TM_MFAS = 1, TM_MEAN = 2, TM_TOTAL = 3, TM_COUNT = 4 };
double g_timings[TM_COUNT] = {};

constexpr int kMfasThreads = 256, kMfasWaves = kMfasThreads / 64;
constexpr double kRootThreshold = 1e-8;   // "root node if the inWeightSum is close to zero" (MFAS.cpp:67)

// CSR entry of node v: the neighbour, the unique edge between them, and whether v is the edge's key1
struct MfasAdj {
  int nbr, edge_first;   // edge << 1 | (v is key1)
};

// dynamic LDS of one workgroup: in-sums, out-sums (doubles), alive flags (bytes)
size_t mfas_lds_bytes(int n_nodes) { return (size_t)n_nodes * (2 * sizeof(double) + 1); }

// One workgroup per direction (grid-stride over directions).  Per direction:
//   1. the weights w[u] = edge_dirs[u] . proj_dirs[d] (x, y, z in order, no fused multiply-add), or the given row;
//   2. the in / out weight sums of every node, one lane per node, summed in CSR order (graphFromEdges, :36-60);
//   3. n steps: a workgroup reduction picks the node (selectNextNodeInOrdering, :63-82: the lowest-index alive node with
//      in-sum < 1e-8, else the alive node of the largest (out + 1) / (in + 1), the lowest index on an exact tie), then the
//      lanes walk its CSR row and subtract |w| from each alive neighbour's in- or out-sum (removeNodeFromGraph, :94-112) —
//      the pairs are unique, so a neighbour is written once per step: no atomics, bitwise reproducible;
//   4. |w| for every edge whose destination precedes its source, else 0 (computeOutlierWeights, :141-171).
__global__ void __launch_bounds__(kMfasThreads) mfas_kernel(int n_nodes, int n_edges, int n_dirs, const int* row_ptr,
                                                            const MfasAdj* adj, const int* e_key1, const int* e_key2,
                                                            const double* edge_dirs, const double* proj_dirs,
                                                            const double* w_given, double* w_work, int* pos,
                                                            int* order, double* out_w) {
  extern __shared__ double mfas_lds[];
  double* s_in = mfas_lds;
  double* s_out = mfas_lds + n_nodes;
  unsigned char* s_alive = (unsigned char*)(mfas_lds + 2 * (size_t)n_nodes);
  __shared__ int s_root[kMfasWaves], s_best[kMfasWaves];
  __shared__ double s_heur[kMfasWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = blockIdx.x; d < n_dirs; d += gridDim.x) {
    const double* w = w_given ? w_given + (size_t)d * n_edges : w_work + (size_t)d * n_edges;
    if (!w_given) {
      const double px = proj_dirs[3 * d], py = proj_dirs[3 * d + 1], pz = proj_dirs[3 * d + 2];
      for (int u = tid; u < n_edges; u += kMfasThreads)
        w_work[(size_t)d * n_edges + u] = __dadd_rn(__dadd_rn(__dmul_rn(edge_dirs[3 * u], px), __dmul_rn(edge_dirs[3 * u + 1], py)),
                                                    __dmul_rn(edge_dirs[3 * u + 2], pz));
      __syncthreads();   // (the rows of w_work are read by other lanes below)
    }
    for (int v = tid; v < n_nodes; v += kMfasThreads) {
      double in = 0.0, out = 0.0;
      for (int k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
        const int ef = adj[k].edge_first;
        const double wv = w[ef >> 1];
        // the edge runs key1 -> key2 when w >= 0 (:48-49): v is its source when (v is key1) == (w >= 0)
        if (((ef & 1) != 0) == (wv >= 0)) out += fabs(wv);
        else in += fabs(wv);
      }
      s_in[v] = in;
      s_out[v] = out;
      s_alive[v] = 1;
    }
    __syncthreads();
    int* my_pos = pos + (size_t)d * n_nodes;
    for (int step = 0; step < n_nodes; ++step) {
      int root = INT_MAX, best = INT_MAX;
      double heur = -1.0;   // (a heuristic is positive: the sums are sums of absolute values, never below -1)
      for (int v = tid; v < n_nodes; v += kMfasThreads) {   // ascending v per lane: the first hit is the lowest
        if (!s_alive[v]) continue;
        const double in = s_in[v];
        if (in < kRootThreshold && root == INT_MAX) root = v;
        const double h = (s_out[v] + 1.0) / (in + 1.0);
        if (h > heur || best == INT_MAX) {
          heur = h;
          best = v;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        root = min(root, __shfl_down(root, o, 64));
        const double oh = __shfl_down(heur, o, 64);
        const int ob = __shfl_down(best, o, 64);
        if (ob != INT_MAX && (best == INT_MAX || oh > heur || (oh == heur && ob < best))) {
          heur = oh;
          best = ob;
        }
      }
      if (lane == 0) {
        s_root[wave] = root;
        s_best[wave] = best;
        s_heur[wave] = heur;
      }
      __syncthreads();
      root = s_root[0];
      best = s_best[0];
      heur = s_heur[0];
#pragma unroll
      for (int q = 1; q < kMfasWaves; ++q) {   // every thread forms the same choice from the same four entries
        root = min(root, s_root[q]);
        if (s_best[q] != INT_MAX && (best == INT_MAX || s_heur[q] > heur || (s_heur[q] == heur && s_best[q] < best))) {
          heur = s_heur[q];
          best = s_best[q];
        }
      }
      const int p = root != INT_MAX ? root : best;   // (an alive node exists at every step: best != INT_MAX)
      if (tid == 0) {
        my_pos[p] = step;
        if (order) order[(size_t)d * n_nodes + step] = p;
        s_alive[p] = 0;   // (no lane reads alive[p] below: a node is not its own neighbour)
      }
      for (int k = row_ptr[p] + tid; k < row_ptr[p + 1]; k += kMfasThreads) {
        const int nb = adj[k].nbr, ef = adj[k].edge_first;
        if (!s_alive[nb]) continue;
        const double wv = w[ef >> 1];
        if (((ef & 1) != 0) == (wv >= 0)) s_in[nb] -= fabs(wv);   // p is the source: the neighbour loses an incoming edge
        else s_out[nb] -= fabs(wv);
      }
      __syncthreads();
    }
    for (int u = tid; u < n_edges; u += kMfasThreads) {
      const double wv = w[u];
      const int src = wv >= 0 ? e_key1[u] : e_key2[u], dst = wv >= 0 ? e_key2[u] : e_key1[u];
      out_w[(size_t)d * n_edges + u] = my_pos[dst] < my_pos[src] ? fabs(wv) : 0.0;
    }
    __syncthreads();   // (the LDS and the scratch words are the next direction's)
  }
}

// out_mean[u] = sum over d, in order of d, of out_w[d][u] / n_dirs: one thread per edge
__global__ void __launch_bounds__(kThreads) mfas_mean_kernel(int n_edges, int n_dirs, const double* out_w, double* mean) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_edges) return;
  double acc = 0.0;
  for (int d = 0; d < n_dirs; ++d) acc += out_w[(size_t)d * n_edges + u] / (double)n_dirs;
  mean[u] = acc;
}

}  // namespace
}  // namespace gsx

using namespace gsx;
using namespace gsx::initdev;

extern "C" {

gsx_status gsx_mfas_outlier_weights(const uint64_t* key1, const uint64_t* key2, int64_t n_edges, const double* edge_dirs,
                                    const double* proj_dirs, const double* weights, int32_t n_dirs, int32_t device,
                                    double* out_mean, double* out_weights, uint64_t* out_ordering) {
  const auto t_total = std::chrono::steady_clock::now();
  if (n_edges < 0 || n_dirs < 1 || (n_edges > 0 && (!key1 || !key2))) return GSX_E_INVALID;
  if (edge_dirs ? !proj_dirs : (n_edges > 0 && !weights)) return GSX_E_INVALID;
  if ((int64_t)n_dirs * std::max<int64_t>(n_edges, 1) >= ((int64_t)1 << 31)) return GSX_E_INVALID;
  // nodes by ascending key; unique pairs in ascending (key1, key2) order, the last entry of a repeated pair
  std::map<uint64_t, int> node;
  std::map<std::pair<uint64_t, uint64_t>, int64_t> last;
  for (int64_t i = 0; i < n_edges; ++i) {
    if (key1[i] == key2[i]) return GSX_E_INVALID;
    node[key1[i]] = node[key2[i]] = 0;
    last[{key1[i], key2[i]}] = i;
  }
  for (const auto& kv : last)
    if (kv.first.first > kv.first.second && last.count({kv.first.second, kv.first.first})) return GSX_E_INVALID;
  const int n_nodes = (int)node.size(), nu = (int)last.size();
  if (n_nodes > GSX_MFAS_MAX_NODES) {
    fprintf(stderr, "gsx: MFAS on %d nodes: more than GSX_MFAS_MAX_NODES = %d (the node sums live in LDS)\n", n_nodes,
            GSX_MFAS_MAX_NODES);
    return GSX_E_INVALID;
  }
  std::vector<uint64_t> node_key;
  for (auto& kv : node) {
    kv.second = (int)node_key.size();
    node_key.push_back(kv.first);
  }
  std::vector<int> e1(nu), e2(nu), row_ptr(n_nodes + 1, 0);
  std::vector<int64_t> source(nu);              // unique edge -> the entry that defines it
  std::map<std::pair<uint64_t, uint64_t>, int> slot;
  {
    int u = 0;
    for (const auto& kv : last) {
      e1[u] = node[kv.first.first];
      e2[u] = node[kv.first.second];
      source[u] = kv.second;
      slot[kv.first] = u;
      ++row_ptr[e1[u] + 1];
      ++row_ptr[e2[u] + 1];
      ++u;
    }
  }
  for (int v = 0; v < n_nodes; ++v) row_ptr[v + 1] += row_ptr[v];
  std::vector<MfasAdj> adj((size_t)2 * nu);
  {
    std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1);
    for (int u = 0; u < nu; ++u) {
      adj[fill[e1[u]]++] = MfasAdj{e2[u], u << 1 | 1};
      adj[fill[e2[u]]++] = MfasAdj{e1[u], u << 1};
    }
  }
  gsx_status st = check_device(device);
  if (st != GSX_OK) return st;
  std::fill(g_timings, g_timings + TM_COUNT, 0.0);
  if (n_edges == 0) return GSX_OK;
  hipFuncAttributes fa;
  size_t fixed = 8192;
  if (hipFuncGetAttributes(&fa, (const void*)mfas_kernel) == hipSuccess) fixed = fa.sharedSizeBytes;
  const size_t lds = mfas_lds_bytes(n_nodes);
  if (lds + fixed > (size_t)160 * 1024) {   // (dynamic + what the compiler placed; cannot fire below GSX_MFAS_MAX_NODES)
    fprintf(stderr, "gsx: mfas_kernel needs %zu + %zu bytes of LDS: launch refused\n", lds, fixed);
    return GSX_E_INVALID;
  }
  // the weights (or the edge directions) of the unique edges
  std::vector<double> h_dirs, h_w;
  if (edge_dirs) {
    h_dirs.resize((size_t)3 * nu);
    for (int u = 0; u < nu; ++u) std::copy(edge_dirs + 3 * source[u], edge_dirs + 3 * source[u] + 3, h_dirs.begin() + 3 * (size_t)u);
  } else {
    h_w.resize((size_t)n_dirs * nu);
    for (int d = 0; d < n_dirs; ++d)
      for (int u = 0; u < nu; ++u) h_w[(size_t)d * nu + u] = weights[(size_t)d * n_edges + source[u]];
  }
  g_timings[TM_HOST] = host_ms_since(t_total);
  Stream S;
  HIPTRY(hipStreamCreate(&S.s));
  Dev<int> d_row, d_e1, d_e2, d_pos, d_order;
  Dev<MfasAdj> d_adj;
  Dev<double> d_dirs, d_proj, d_wgiven, d_wwork, d_outw, d_mean;
  HIPTRY(d_row.upload(row_ptr, S.s));
  HIPTRY(d_adj.upload(adj, S.s));
  HIPTRY(d_e1.upload(e1, S.s));
  HIPTRY(d_e2.upload(e2, S.s));
  if (edge_dirs) {
    HIPTRY(d_dirs.upload(h_dirs, S.s));
    HIPTRY(d_proj.upload(std::vector<double>(proj_dirs, proj_dirs + 3 * (size_t)n_dirs), S.s));
    HIPTRY(d_wwork.alloc((size_t)n_dirs * nu));
  } else {
    HIPTRY(d_wgiven.upload(h_w, S.s));
  }
  HIPTRY(d_pos.alloc((size_t)n_dirs * n_nodes));
  if (out_ordering) HIPTRY(d_order.alloc((size_t)n_dirs * n_nodes));
  HIPTRY(d_outw.alloc((size_t)n_dirs * nu));
  HIPTRY(d_mean.alloc((size_t)nu));
  if (lds > 48 * 1024)
    HIPTRY(hipFuncSetAttribute((const void*)mfas_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  // as many workgroups as can be resident: LDS and 2048 threads a CU; more directions than that take the grid-stride
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)(156 * 1024) / (lds + fixed + 256), 2048 / kMfasThreads));
  int grid = std::min(n_dirs, cus * per_cu);
  if (const char* cap = std::getenv("GSX_MFAS_MAX_GRID")) {   // (include/gsx.h: fewer workgroups, same bits)
    const int v = std::atoi(cap);
    if (v > 0) grid = std::min(grid, v);
  }
  EventPair ev_mfas, ev_mean;
  ev_mfas.begin(S.s);
  hipLaunchKernelGGL(mfas_kernel, dim3(grid), dim3(kMfasThreads), lds, S.s, n_nodes, nu, (int)n_dirs, d_row.p, d_adj.p, d_e1.p,
                     d_e2.p, (const double*)d_dirs.p, (const double*)d_proj.p, (const double*)d_wgiven.p, d_wwork.p, d_pos.p,
                     d_order.p, d_outw.p);
  ev_mfas.end();
  HIPTRY(hipGetLastError());
  ev_mean.begin(S.s);
  hipLaunchKernelGGL(mfas_mean_kernel, dim3(blocks_for(nu)), dim3(kThreads), 0, S.s, nu, (int)n_dirs, (const double*)d_outw.p,
                     d_mean.p);
  ev_mean.end();
  HIPTRY(hipGetLastError());
  std::vector<double> h_mean((size_t)nu), h_outw(out_weights ? (size_t)n_dirs * nu : 0);
  std::vector<int> h_order(out_ordering ? (size_t)n_dirs * n_nodes : 0);
  HIPTRY(hipMemcpyAsync(h_mean.data(), d_mean.p, h_mean.size() * sizeof(double), hipMemcpyDeviceToHost, S.s));
  if (out_weights) HIPTRY(hipMemcpyAsync(h_outw.data(), d_outw.p, h_outw.size() * sizeof(double), hipMemcpyDeviceToHost, S.s));
  if (out_ordering) HIPTRY(hipMemcpyAsync(h_order.data(), d_order.p, h_order.size() * sizeof(int), hipMemcpyDeviceToHost, S.s));
  HIPTRY(hipStreamSynchronize(S.s));
  g_timings[TM_MFAS] = ev_mfas.ms();
  g_timings[TM_MEAN] = ev_mean.ms();
  // back to the caller's edge list (a superseded duplicate reads its successor's slot) and keys
  for (int64_t i = 0; i < n_edges; ++i) {
    const int u = slot[{key1[i], key2[i]}];
    if (out_mean) out_mean[i] = h_mean[u];
    if (out_weights)
      for (int d = 0; d < n_dirs; ++d) out_weights[(size_t)d * n_edges + i] = h_outw[(size_t)d * nu + u];
  }
  if (out_ordering)
    for (size_t k = 0; k < h_order.size(); ++k) out_ordering[k] = node_key[h_order[k]];
  g_timings[TM_TOTAL] = host_ms_since(t_total);
  return GSX_OK;
}

gsx_status gsx_mfas_timings(double* out_ms, int32_t n) {
  if (!out_ms || n != TM_COUNT) return GSX_E_INVALID;
  std::copy(g_timings, g_timings + TM_COUNT, out_ms);
  return GSX_OK;
}

}  // extern "C"
