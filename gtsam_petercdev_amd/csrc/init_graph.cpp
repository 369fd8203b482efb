// init_graph.cpp — host part of the Pose3 initializer (InitializePose3): the pose graph, its adjacency, and the lowering of
// the two internal problems (relaxed rotations, anchored Gauss-Newton) to ordinary gsx_problem_desc's.  No device code.
//   buildPoseGraph<Pose3>           gtsam/slam/InitializePose.h:36-52
//   buildLinearOrientationGraph     gtsam/slam/InitializePose3.cpp:37-71
//   createSymbolicGraph             gtsam/slam/InitializePose3.cpp:221-253
//   computePoses<Pose3>             gtsam/slam/InitializePose.h:57-97
#include <algorithm>
#include <cmath>
#include <numeric>

#include "gsx_internal.h"

namespace gsx {

gsx_problem_desc OwnedDesc::view() const {
  gsx_problem_desc d{};
  d.n_vars = (int32_t)keys.size();
  d.var_keys = keys.data();
  d.var_types = types.data();
  d.var_dims = dims.data();
  d.n_factors = (int32_t)f_type.size();
  d.f_type = f_type.data();
  d.f_rows = f_rows.data();
  d.f_key_ptr = f_key_ptr.data();
  d.f_vars = f_vars.data();
  d.f_meas_ptr = f_meas_ptr.data();
  d.meas = meas.data();
  d.f_noise_kind = f_noise_kind.data();
  d.f_noise_ptr = f_noise_ptr.data();
  d.noise = noise.data();
  return d;
}

// first entry of noiseModel->whiten(e_0), which the reference then treats as the rotation precision
// (InitializePose3.cpp:48-51).  Unit: 1; Isotropic: 1 / sigma (NoiseModel.cpp:647-649); Diagonal: 1 / sigma_0 (:323-325);
// Gaussian: R(0, 0) (whiten = R v); a zero sigma: Constrained::whiten leaves the entry alone (:395-409).  Robust: its base
// model — a deliberate deviation: the reference's Robust::whitenInPlace reweights as well (NoiseModel.h:711-712; see
// include/gsx.h).  false: malformed parameters.
static bool rotation_weight(int kind, const double* np, int64_t nn, double* w) {
  const int base = kind & GSX_NOISE_BASE_MASK, loss = kind >> 4;
  if (kind < 0 || loss > 3) return false;
  const int64_t extra = loss ? 1 : 0;
  switch (base) {
    case GSX_NOISE_UNIT:
      if (nn != extra) return false;
      *w = 1.0;
      return true;
    case GSX_NOISE_ISOTROPIC:
      if (nn != 1 + extra) return false;
      *w = 1.0 / np[0];
      return true;
    case GSX_NOISE_DIAGONAL:
      if (nn != 6 + extra) return false;
      *w = np[0] == 0.0 ? 1.0 : 1.0 / np[0];
      return true;
    case GSX_NOISE_GAUSSIAN:
      if (nn != 36 + extra) return false;
      *w = np[0];
      return true;
    case GSX_NOISE_CONSTRAINED:
      if (nn != 12 || loss) return false;
      *w = np[0] == 0.0 ? 1.0 : 1.0 / np[0];
      return true;
  }
  return false;
}

gsx_status build_pose_graph(const gsx_problem_desc* d, PoseGraph& G, std::string& err) {
  if (!d || d->n_vars < 0 || d->n_factors < 0 || (d->n_vars > 0 && (!d->var_keys || !d->var_types || !d->var_dims)) ||
      (d->n_factors > 0 && (!d->f_type || !d->f_key_ptr || !d->f_vars || !d->f_meas_ptr || !d->f_noise_kind ||
                            !d->f_noise_ptr))) {
    err = "null or negative-sized description";
    return GSX_E_INVALID;
  }
  G = PoseGraph();
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
    if (d->var_types[v] == GSX_VAR_POSE3) {
      if (d->var_dims[v] != 6) {
        err = "bad variable type/dim";
        return GSX_E_INVALID;
      }
      G.node_of_var[v] = (int)G.pose_var.size();
      G.pose_var.push_back(v);
    }
  }
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
    double w = 0.0;
    if (nm != 12 || !d->meas || (nn > 0 && !d->noise) ||
        !rotation_weight(d->f_noise_kind[f], d->noise + d->f_noise_ptr[f], nn, &w)) {
      err = "malformed factor " + std::to_string(f);
      return GSX_E_INVALID;
    }
    const int a = nk == 2 ? nodes[0] : anchor, b = nk == 2 ? nodes[1] : nodes[0];
    G.from.push_back(a);
    G.to.push_back(b);
    G.factor.push_back(f);
    G.weight.push_back(w);
    const double* m = d->meas + d->f_meas_ptr[f];
    G.rot.insert(G.rot.end(), m, m + 9);
    G.touched[a] = G.touched[b] = 1;
  }
  G.touched[anchor] = 1;
  G.all_touched = std::all_of(G.touched.begin(), G.touched.end(), [](char c) { return c != 0; });
  // adjacency: both ends of every edge, in factor order
  const int ne = (int)G.from.size();
  G.adj_ptr.assign(G.n_poses + 2, 0);
  for (int e = 0; e < ne; ++e) {
    G.adj_ptr[G.from[e] + 1]++;
    G.adj_ptr[G.to[e] + 1]++;
  }
  for (int n = 0; n <= G.n_poses; ++n) G.adj_ptr[n + 1] += G.adj_ptr[n];
  G.adj.assign(2 * (size_t)ne, 0);
  {
    std::vector<int> fill(G.adj_ptr.begin(), G.adj_ptr.end() - 1);
    for (int e = 0; e < ne; ++e) {
      G.adj[fill[G.from[e]]++] = e;
      G.adj[fill[G.to[e]]++] = e;
    }
  }
  // joined to the anchor by edges that carry weight?  (otherwise the relaxed system is rank deficient: the reference
  // throws IndeterminantLinearSystemException from its elimination)
  std::vector<int> root(G.n_poses + 1);
  std::iota(root.begin(), root.end(), 0);
  auto find = [&](int x) {
    while (root[x] != x) x = root[x] = root[root[x]];
    return x;
  };
  for (int e = 0; e < ne; ++e)
    if (G.weight[e] != 0.0) root[find(G.from[e])] = find(G.to[e]);
  G.anchored = true;
  for (int n = 0; n < G.n_poses; ++n)
    if (G.touched[n] && find(n) != find(anchor)) G.anchored = false;
  return GSX_OK;
}

// the touched nodes and the anchor, in ascending key order
static void internal_variables(const gsx_problem_desc* d, const PoseGraph& G, int type, int dim, OwnedDesc& out,
                               std::vector<int>& var_of_node) {
  var_of_node.assign(G.n_poses + 1, -1);
  bool anchor_in = false;
  auto push_anchor = [&]() {
    var_of_node[G.n_poses] = (int)out.keys.size();
    out.keys.push_back(kAnchorKey);
    anchor_in = true;
  };
  for (int n = 0; n < G.n_poses; ++n) {
    if (!G.touched[n]) continue;
    const uint64_t key = d->var_keys[G.pose_var[n]];
    if (!anchor_in && key > kAnchorKey) push_anchor();
    var_of_node[n] = (int)out.keys.size();
    out.keys.push_back(key);
  }
  if (!anchor_in) push_anchor();
  out.types.assign(out.keys.size(), type);
  out.dims.assign(out.keys.size(), dim);
}

void lower_relaxed(const gsx_problem_desc* d, const PoseGraph& G, OwnedDesc& out, std::vector<int>& var_of_node,
                   std::vector<int>& edges) {
  out = OwnedDesc();
  edges.clear();
  internal_variables(d, G, GSX_VAR_VECTOR, 3, out, var_of_node);
  out.f_key_ptr.push_back(0);
  out.f_meas_ptr.push_back(0);
  out.f_noise_ptr.push_back(0);
  for (int e = 0; e < (int)G.from.size(); ++e) {
    if (G.weight[e] == 0.0) continue;  // Isotropic::Precision(9, 0): the whitened block vanishes
    edges.push_back(e);
    out.f_type.push_back(GSX_F_LINEAR);
    out.f_rows.push_back(3);
    out.f_vars.push_back(var_of_node[G.from[e]]);
    out.f_vars.push_back(var_of_node[G.to[e]]);
    out.f_key_ptr.push_back((int32_t)out.f_vars.size());
    out.meas.insert(out.meas.end(), 21, 0.0);
    out.f_meas_ptr.push_back((int64_t)out.meas.size());
    out.f_noise_kind.push_back(GSX_NOISE_UNIT);
    out.f_noise_ptr.push_back(0);
  }
  // the anchor's prior [I | e_1] (InitializePose3.cpp:64-69), 3 x 4 column-major
  out.f_type.push_back(GSX_F_LINEAR);
  out.f_rows.push_back(3);
  out.f_vars.push_back(var_of_node[G.n_poses]);
  out.f_key_ptr.push_back((int32_t)out.f_vars.size());
  const double prior[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0};
  out.meas.insert(out.meas.end(), prior, prior + 12);
  out.f_meas_ptr.push_back((int64_t)out.meas.size());
  out.f_noise_kind.push_back(GSX_NOISE_UNIT);
  out.f_noise_ptr.push_back(0);
  out.noise.push_back(0.0);  // (keeps the pointer valid)
}

void lower_anchor_graph(const gsx_problem_desc* d, const PoseGraph& G, OwnedDesc& out, std::vector<int>& var_of_node) {
  out = OwnedDesc();
  internal_variables(d, G, GSX_VAR_POSE3, 6, out, var_of_node);
  out.f_key_ptr.push_back(0);
  out.f_meas_ptr.push_back(0);
  out.f_noise_ptr.push_back(0);
  for (int e = 0; e < (int)G.from.size(); ++e) {
    if (G.weight[e] == 0.0) continue;  // an infinite sigma: the whitened factor vanishes
    const int f = G.factor[e];
    out.f_type.push_back(GSX_F_BETWEEN);  // a prior becomes a between from the anchor (InitializePose.h:47-49)
    out.f_rows.push_back(6);
    out.f_vars.push_back(var_of_node[G.from[e]]);
    out.f_vars.push_back(var_of_node[G.to[e]]);
    out.f_key_ptr.push_back((int32_t)out.f_vars.size());
    out.meas.insert(out.meas.end(), d->meas + d->f_meas_ptr[f], d->meas + d->f_meas_ptr[f + 1]);
    out.f_meas_ptr.push_back((int64_t)out.meas.size());
    out.f_noise_kind.push_back(d->f_noise_kind[f]);
    if (d->f_noise_ptr[f + 1] > d->f_noise_ptr[f])
      out.noise.insert(out.noise.end(), d->noise + d->f_noise_ptr[f], d->noise + d->f_noise_ptr[f + 1]);
    out.f_noise_ptr.push_back((int64_t)out.noise.size());
  }
  // PriorFactor<Pose3>(kAnchorKey, Pose3(), Unit::Create(6)) (InitializePose.h:73-75)
  out.f_type.push_back(GSX_F_PRIOR);
  out.f_rows.push_back(6);
  out.f_vars.push_back(var_of_node[G.n_poses]);
  out.f_key_ptr.push_back((int32_t)out.f_vars.size());
  const double identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  out.meas.insert(out.meas.end(), identity, identity + 12);
  out.f_meas_ptr.push_back((int64_t)out.meas.size());
  out.f_noise_kind.push_back(GSX_NOISE_UNIT);
  out.f_noise_ptr.push_back((int64_t)out.noise.size());
  out.noise.push_back(0.0);  // (keeps the pointer valid)
}

}  // namespace gsx

extern "C" {

void gsx_init_pose3_params_default(gsx_init_pose3_params* p) {
  if (!p) return;
  p->use_gradient = 0;
  p->max_gradient_iterations = 10000;  // InitializePose3.h: computeOrientationsGradient(..., maxIter = 10000, setRefFrame = true)
  p->set_ref_frame = 1;
  p->single_iter = 1;
}

gsx_status gsx_pose3_init_structure(const gsx_problem_desc* desc, int32_t* n_edges, int32_t* edge_from, int32_t* edge_to,
                                    int32_t* adj_ptr, int32_t* adj, int64_t adj_cap) {
  if (gsx::enter_call(desc, "gsx_pose3_init_structure") != GSX_OK) return GSX_E_INVALID;
  gsx::PoseGraph G;
  std::string err;
  gsx_status st = gsx::build_pose_graph(desc, G, err);
  if (st != GSX_OK) return st;
  const int ne = (int)G.from.size();
  if (n_edges) *n_edges = ne;
  if (edge_from) std::copy(G.from.begin(), G.from.end(), edge_from);
  if (edge_to) std::copy(G.to.begin(), G.to.end(), edge_to);
  if (adj_ptr) std::copy(G.adj_ptr.begin(), G.adj_ptr.end(), adj_ptr);
  if (adj) {
    if (adj_cap < (int64_t)G.adj.size()) return GSX_E_INVALID;
    std::copy(G.adj.begin(), G.adj.end(), adj);
  }
  return GSX_OK;
}

}  // extern "C"
