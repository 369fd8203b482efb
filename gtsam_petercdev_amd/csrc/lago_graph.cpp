// lago_graph.cpp — host part of the Pose2 initializer (lago): the pose graph, the two spanning trees, the tree / chord
// split and the lowering of the two linear systems to ordinary gsx_problem_desc's.  No device code.
//   buildPoseGraph<Pose2>           gtsam/slam/InitializePose.h:36-52
//   findOdometricPath               gtsam/slam/lago.cpp:202-226
//   findMinimumSpanningTree         gtsam/slam/lago.cpp:229-260 (kruskal: gtsam/base/kruskal-inl.h:54-104)
//   getSymbolicGraph                gtsam/slam/lago.cpp:101-138
//   buildLinearOrientationGraph     gtsam/slam/lago.cpp:165-199
//   computePoses                    gtsam/slam/lago.cpp:308-356
#include <algorithm>
#include <cmath>
#include <numeric>

#include "gsx_internal.h"

namespace gsx {

// the three sigmas of a Diagonal model (lago.cpp:142-162, :344-348: the reference casts to noiseModel::Diagonal and throws
// invalid_argument otherwise — Unit, Isotropic and Constrained derive from it, Gaussian and Robust do not).  A sigma that
// is not positive is refused: the reference would carry a constrained row into its linear graphs.
static bool diagonal_sigmas(int kind, const double* np, int64_t nn, double* s) {
  if (kind < 0 || (kind >> 4) != 0) return false;
  switch (kind & GSX_NOISE_BASE_MASK) {
    case GSX_NOISE_UNIT:
      if (nn != 0) return false;
      s[0] = s[1] = s[2] = 1.0;
      break;
    case GSX_NOISE_ISOTROPIC:
      if (nn != 1) return false;
      s[0] = s[1] = s[2] = np[0];
      break;
    case GSX_NOISE_DIAGONAL:
      if (nn != 3) return false;
      std::copy(np, np + 3, s);
      break;
    case GSX_NOISE_CONSTRAINED:
      if (nn != 6) return false;
      std::copy(np, np + 3, s);
      break;
    default:
      return false;
  }
  return s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0;
}

// measured().theta(): Pose2(x, y, theta) keeps cos / sin, so theta() is atan2(sin, cos) (Rot2.h:191-193).  An angle
// already inside (-pi, pi] is kept as it is stored.
static double measured_theta(double t) { return (t > M_PI || t <= -M_PI) ? std::atan2(std::sin(t), std::cos(t)) : t; }

gsx_status build_lago_graph(const gsx_problem_desc* d, LagoGraph& G, std::string& err) {
  if (!d || d->n_vars < 0 || d->n_factors < 0 || (d->n_vars > 0 && (!d->var_keys || !d->var_types || !d->var_dims)) ||
      (d->n_factors > 0 && (!d->f_type || !d->f_key_ptr || !d->f_vars || !d->f_meas_ptr || !d->f_noise_kind ||
                            !d->f_noise_ptr))) {
    err = "null or negative-sized description";
    return GSX_E_INVALID;
  }
  G = LagoGraph();
  G.node_of_var.assign(d->n_vars, -1);
  for (int v = 0; v < d->n_vars; ++v) {
    if (v > 0 && !(d->var_keys[v] > d->var_keys[v - 1])) {
      err = "var_keys must be strictly ascending";
      return GSX_E_INVALID;
    }
    if (d->var_keys[v] == kAnchorKey) {
      err = "a variable carries the initializer's anchor key 99999999";
      return GSX_E_INVALID;
    }
    if (d->var_types[v] == GSX_VAR_POSE2) {
      if (d->var_dims[v] != 3) {
        err = "bad variable type/dim";
        return GSX_E_INVALID;
      }
      G.node_of_var[v] = (int)G.pose_var.size();
      G.pose_var.push_back(v);
      G.key.push_back(d->var_keys[v]);
    }
  }
  G.key.push_back(kAnchorKey);
  G.n_poses = (int)G.pose_var.size();
  const int anchor = G.n_poses;
  G.touched.assign(G.n_poses + 1, 0);
  for (int f = 0; f < d->n_factors; ++f) {
    const int t = d->f_type[f];
    if (t != GSX_F_BETWEEN && t != GSX_F_PRIOR) continue;
    const int kp = d->f_key_ptr[f], nk = d->f_key_ptr[f + 1] - kp;
    if (nk != (t == GSX_F_BETWEEN ? 2 : 1)) {
      err = "malformed factor " + std::to_string(f);
      return GSX_E_INVALID;
    }
    int nodes[2] = {-1, -1};
    bool pose = true;
    for (int k = 0; k < nk; ++k) {
      const int v = d->f_vars[kp + k];
      if (v < 0 || v >= d->n_vars) {
        err = "factor " + std::to_string(f) + " refers to a variable out of range";
        return GSX_E_INVALID;
      }
      nodes[k] = G.node_of_var[v];
      pose = pose && nodes[k] >= 0;
    }
    if (!pose) continue;  // a between / prior on another type: dropped, as the dynamic casts drop it
    if (nk == 2 && nodes[0] == nodes[1]) {
      err = "factor " + std::to_string(f) + " lists a variable twice";
      return GSX_E_INVALID;
    }
    const int64_t nm = d->f_meas_ptr[f + 1] - d->f_meas_ptr[f], nn = d->f_noise_ptr[f + 1] - d->f_noise_ptr[f];
    double s[3];
    if (nm != 3 || !d->meas || (nn > 0 && !d->noise)) {
      err = "malformed factor " + std::to_string(f);
      return GSX_E_INVALID;
    }
    if (!diagonal_sigmas(d->f_noise_kind[f], d->noise + d->f_noise_ptr[f], nn, s)) {
      err = "factor " + std::to_string(f) + ": lago needs a Diagonal noise model with positive sigmas";
      return GSX_E_INVALID;
    }
    const int a = nk == 2 ? nodes[0] : anchor, b = nk == 2 ? nodes[1] : nodes[0];
    G.from.push_back(a);
    G.to.push_back(b);
    G.factor.push_back(f);
    const double* m = d->meas + d->f_meas_ptr[f];
    G.meas.push_back(m[0]);
    G.meas.push_back(m[1]);
    G.meas.push_back(measured_theta(m[2]));
    G.sigma.insert(G.sigma.end(), s, s + 3);
    G.touched[a] = G.touched[b] = 1;
  }
  G.all_touched = std::all_of(G.touched.begin(), G.touched.begin() + G.n_poses, [](char c) { return c != 0; });
  return GSX_OK;
}

// findOdometricPath (lago.cpp:202-226), with its emplace semantics: the first consecutive-key edge of a node wins, the
// smallest key seen is attached to the anchor.  An edge from the anchor is never "consecutive".
static void odometric_path(LagoGraph& G, int* min_node) {
  const int anchor = G.n_poses;
  uint64_t minKey = kAnchorKey;
  int minNode = anchor;
  bool minUnassigned = true;
  for (size_t e = 0; e < G.from.size(); ++e) {
    int n1 = G.from[e], n2 = G.to[e];
    if (G.key[n1] > G.key[n2]) std::swap(n1, n2);
    if (minUnassigned) {
      minKey = G.key[n1];
      minNode = n1;
      minUnassigned = false;
    }
    if (n1 != anchor && n2 != anchor && G.key[n2] - G.key[n1] == 1) {  // consecutive keys
      if (G.parent[n2] < 0) G.parent[n2] = n1;
      if (G.key[n1] < minKey) {
        minKey = G.key[n1];
        minNode = n1;
      }
    }
  }
  if (G.parent[minNode] < 0) G.parent[minNode] = anchor;
  G.parent[anchor] = anchor;  // root
  *min_node = minNode;
}

// findMinimumSpanningTree (lago.cpp:229-260): Kruskal with unit weights — a stable sort, so the edges are tried in factor
// order (kruskal-inl.h:36-51, :78-102) — then the stack-driven walk from the anchor: the unvisited neighbours of a node
// are pushed in MST-edge order and popped last-in-first-out.  The walk reads an adjacency list instead of scanning every
// MST edge per node: O(N + E).
static void minimum_spanning_tree(LagoGraph& G) {
  const int n_nodes = G.n_poses + 1, anchor = G.n_poses;
  std::vector<int> root(n_nodes);
  std::iota(root.begin(), root.end(), 0);
  auto find = [&](int x) {
    while (root[x] != x) x = root[x] = root[root[x]];
    return x;
  };
  std::vector<int> mst;
  for (int e = 0; e < (int)G.from.size(); ++e) {
    const int u = find(G.from[e]), v = find(G.to[e]);
    if (u == v) continue;
    root[u] = v;
    mst.push_back(e);
  }
  std::vector<int> adj_ptr(n_nodes + 1, 0);
  for (int e : mst) {
    adj_ptr[G.from[e] + 1]++;
    adj_ptr[G.to[e] + 1]++;
  }
  for (int n = 0; n < n_nodes; ++n) adj_ptr[n + 1] += adj_ptr[n];
  std::vector<int> adj(2 * mst.size()), fill(adj_ptr.begin(), adj_ptr.end() - 1);
  for (int e : mst) {
    adj[fill[G.from[e]]++] = G.to[e];
    adj[fill[G.to[e]]++] = G.from[e];
  }
  std::vector<char> visited(n_nodes, 0);
  std::vector<std::pair<int, int>> stack;
  stack.push_back({anchor, anchor});
  while (!stack.empty()) {
    const auto [u, parent] = stack.back();
    stack.pop_back();
    if (visited[u]) continue;
    visited[u] = 1;
    G.parent[u] = parent;
    for (int q = adj_ptr[u]; q < adj_ptr[u + 1]; ++q)
      if (!visited[adj[q]]) stack.push_back({adj[q], u});
  }
}

bool forest_depths(const int32_t* parent, int64_t n, std::vector<int>& depth, int* max_depth) {
  depth.assign((size_t)n, -1);
  int deepest = 0;
  std::vector<int64_t> path;
  for (int64_t i = 0; i < n; ++i) {
    if (depth[i] >= 0) continue;
    path.clear();
    int64_t x = i;
    while (depth[x] < 0) {
      const int64_t p = parent[x];
      if (p < 0 || p >= n) return false;
      if (p == x) {
        depth[x] = 0;
        break;
      }
      if ((int64_t)path.size() > n) return false;  // a cycle
      depth[x] = -2;                               // on the current path
      path.push_back(x);
      x = p;
      if (depth[x] == -2) return false;            // a cycle
    }
    int dd = depth[x];
    for (size_t k = path.size(); k-- > 0;) depth[path[k]] = ++dd;
    if (!path.empty()) deepest = std::max(deepest, depth[path[0]]);
  }
  if (max_depth) *max_depth = deepest;
  return true;
}

gsx_status lago_tree(LagoGraph& G, bool use_odometric_path, std::string& err) {
  const int n_nodes = G.n_poses + 1, anchor = G.n_poses, ne = (int)G.from.size();
  G.parent.assign(n_nodes, -1);
  G.delta.assign(n_nodes, 0.0);
  G.tree_ids.clear();
  G.chord_ids.clear();
  G.is_chord.assign(ne, 0);
  int min_node = anchor;
  if (use_odometric_path)
    odometric_path(G, &min_node);
  else
    minimum_spanning_tree(G);
  // getSymbolicGraph (:101-138): tree.at(key1) is looked up first, tree.at(key2) only when the first test fails; the
  // signed deltaTheta of a node is inserted once
  std::vector<char> has_delta(n_nodes, 0);
  for (int e = 0; e < ne; ++e) {
    const int n1 = G.from[e], n2 = G.to[e];
    const double deltaTheta = G.meas[3 * (size_t)e + 2];
    bool inTree = false;
    if (G.parent[n1] < 0) {
      err = "a pose of factor " + std::to_string(G.factor[e]) + " is not in the spanning tree";
      return GSX_E_INVALID;
    }
    if (G.parent[n1] == n2) {  // key2 -> key1
      if (!has_delta[n1]) G.delta[n1] = -deltaTheta;
      has_delta[n1] = 1;
      inTree = true;
    } else {
      if (G.parent[n2] < 0) {
        err = "a pose of factor " + std::to_string(G.factor[e]) + " is not in the spanning tree";
        return GSX_E_INVALID;
      }
      if (G.parent[n2] == n1) {  // key1 -> key2
        if (!has_delta[n2]) G.delta[n2] = deltaTheta;
        has_delta[n2] = 1;
        inTree = true;
      }
    }
    if (inTree) {
      G.tree_ids.push_back(e);
    } else {
      G.chord_ids.push_back(e);
      G.is_chord[e] = 1;
    }
  }
  // computeThetaToRoot (:56-79) walks tree.at() from every node of deltaThetaMap up to the anchor
  std::vector<int32_t> up(n_nodes);
  for (int n = 0; n < n_nodes; ++n) up[n] = G.parent[n] < 0 ? n : G.parent[n];
  std::vector<int> depth;
  if (!forest_depths(up.data(), n_nodes, depth, nullptr)) {
    err = "the spanning tree has a cycle";
    return GSX_E_INVALID;
  }
  G.max_depth = 0;
  std::vector<signed char> joined(n_nodes, -1);  // to the anchor: -1 not known yet
  std::vector<int> path;
  for (int n = 0; n < n_nodes; ++n)
    if (G.parent[n] < 0) joined[n] = 0;
  joined[anchor] = 1;
  for (int n = 0; n < G.n_poses; ++n) {
    if (G.parent[n] < 0) continue;
    path.clear();
    int x = n;
    for (; joined[x] < 0; x = up[x]) path.push_back(x);
    for (int p : path) joined[p] = joined[x];
    if (!joined[n]) {
      err = "a pose of the spanning tree is not joined to the anchor";
      return GSX_E_INVALID;
    }
    G.max_depth = std::max(G.max_depth, depth[n]);
  }
  // the one tree link no factor stands behind: minKey -> anchor of the odometric path.  Without a prior on that pose the
  // reference's deltaThetaMap.at(minKey) throws; the orientation system would have no row that fixes the gauge.
  G.anchored = !(use_odometric_path && min_node != anchor && G.parent[min_node] == anchor && !has_delta[min_node]);
  return GSX_OK;
}

// the touched nodes (and the anchor when with_anchor), in ascending key order
static void lago_variables(const LagoGraph& G, bool with_anchor, int dim, OwnedDesc& out, std::vector<int>& var_of_node) {
  var_of_node.assign(G.n_poses + 1, -1);
  bool anchor_in = !with_anchor;
  auto push_anchor = [&]() {
    var_of_node[G.n_poses] = (int)out.keys.size();
    out.keys.push_back(kAnchorKey);
    anchor_in = true;
  };
  for (int n = 0; n < G.n_poses; ++n) {
    if (!G.touched[n]) continue;
    if (!anchor_in && G.key[n] > kAnchorKey) push_anchor();
    var_of_node[n] = (int)out.keys.size();
    out.keys.push_back(G.key[n]);
  }
  if (!anchor_in) push_anchor();
  out.types.assign(out.keys.size(), GSX_VAR_VECTOR);
  out.dims.assign(out.keys.size(), dim);
}

static void push_linear(OwnedDesc& out, int rows, int cols) {
  out.f_type.push_back(GSX_F_LINEAR);
  out.f_rows.push_back(rows);
  out.f_key_ptr.push_back((int32_t)out.f_vars.size());
  out.meas.insert(out.meas.end(), (size_t)rows * cols, 0.0);
  out.f_meas_ptr.push_back((int64_t)out.meas.size());
  out.f_noise_kind.push_back(GSX_NOISE_UNIT);
  out.f_noise_ptr.push_back(0);
}

void lower_lago_orientations(const gsx_problem_desc* d, const LagoGraph& G, OwnedDesc& out, std::vector<int>& var_of_node) {
  (void)d;
  out = OwnedDesc();
  lago_variables(G, false, 1, out, var_of_node);
  out.f_key_ptr.push_back(0);
  out.f_meas_ptr.push_back(0);
  out.f_noise_ptr.push_back(0);
  for (size_t e = 0; e < G.from.size(); ++e) {
    // theta_anchor = 0 is substituted for the reference's sigma-0 prior on the anchor (:196-197): an edge from the anchor
    // is the unary row [1 / sigma | delta / sigma]
    const bool unary = G.from[e] == G.n_poses;
    if (!unary) out.f_vars.push_back(var_of_node[G.from[e]]);
    out.f_vars.push_back(var_of_node[G.to[e]]);
    push_linear(out, 1, unary ? 2 : 3);
  }
  out.noise.push_back(0.0);  // (keeps the pointer valid)
}

void lower_lago_poses(const gsx_problem_desc* d, const LagoGraph& G, OwnedDesc& out, std::vector<int>& var_of_node) {
  (void)d;
  out = OwnedDesc();
  lago_variables(G, true, 3, out, var_of_node);
  out.f_key_ptr.push_back(0);
  out.f_meas_ptr.push_back(0);
  out.f_noise_ptr.push_back(0);
  for (size_t e = 0; e < G.from.size(); ++e) {
    out.f_vars.push_back(var_of_node[G.from[e]]);
    out.f_vars.push_back(var_of_node[G.to[e]]);
    push_linear(out, 3, 7);
  }
  // linearPose2graph.add(kAnchorKey, I3, Vector3(0, 0, 0), priorPose2Noise) (:355), priorPose2Noise =
  // Diagonal::Variances(1e-6, 1e-6, 1e-8) (:45-46): whitened here, 3 x 4 column-major
  out.f_vars.push_back(var_of_node[G.n_poses]);
  push_linear(out, 3, 4);
  double* prior = out.meas.data() + out.meas.size() - 12;
  prior[0] = 1.0 / std::sqrt(1e-6);
  prior[4] = 1.0 / std::sqrt(1e-6);
  prior[8] = 1.0 / std::sqrt(1e-8);
  out.noise.push_back(0.0);  // (keeps the pointer valid)
}

}  // namespace gsx

extern "C" {

gsx_status gsx_lago_structure(const gsx_problem_desc* desc, int32_t use_odometric_path, int32_t* n_edges, int32_t* edge_from,
                              int32_t* edge_to, int32_t* parent, double* delta, int32_t* n_tree, int32_t* tree_ids,
                              int32_t* chord_ids, int32_t* max_depth) {
  if (gsx::enter_call(desc, "gsx_lago_structure") != GSX_OK) return GSX_E_INVALID;
  gsx::LagoGraph G;
  std::string err;
  gsx_status st = gsx::build_lago_graph(desc, G, err);
  if (st != GSX_OK) return st;
  if (n_edges) *n_edges = (int32_t)G.from.size();
  if (edge_from) std::copy(G.from.begin(), G.from.end(), edge_from);
  if (edge_to) std::copy(G.to.begin(), G.to.end(), edge_to);
  if (!parent && !delta && !n_tree && !tree_ids && !chord_ids && !max_depth) return GSX_OK;
  st = gsx::lago_tree(G, use_odometric_path != 0, err);
  if (st != GSX_OK) return st;
  if (parent) std::copy(G.parent.begin(), G.parent.end(), parent);
  if (delta) std::copy(G.delta.begin(), G.delta.end(), delta);
  if (n_tree) *n_tree = (int32_t)G.tree_ids.size();
  if (tree_ids) std::copy(G.tree_ids.begin(), G.tree_ids.end(), tree_ids);
  if (chord_ids) std::copy(G.chord_ids.begin(), G.chord_ids.end(), chord_ids);
  if (max_depth) *max_depth = G.max_depth;
  return GSX_OK;
}

}  // extern "C"
