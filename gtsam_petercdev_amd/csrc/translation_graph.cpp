// translation_graph.cpp — TranslationRecovery (gtsam/sfm/TranslationRecovery.cpp:49-228) on the host: the zero-edge merge,
// the graph of translation factors with its priors, the random initial values; and the driver that runs it on an ordinary
// handle.  Host code only: the device work is the handle's (GSX_F_TRANSLATION / GSX_F_BILINEAR_TRANSLATION in kernels.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <random>
#include <set>

#include "gsx_internal.h"

namespace {

// DSFMap<Key> (gtsam/base/DSFMap.h:47-113): union by rank, the root of x on a tie; find creates the entry
struct Dsf {
  struct Entry {
    uint64_t parent;
    size_t rank;
  };
  std::map<uint64_t, Entry> e;
  uint64_t find(uint64_t k) {
    auto it = e.find(k);
    if (it == e.end()) {
      e[k] = Entry{k, 0};
      return k;
    }
    uint64_t root = k;
    while (e[root].parent != root) root = e[root].parent;
    while (e[k].parent != root) {  // path compression (does not change a root)
      const uint64_t next = e[k].parent;
      e[k].parent = root;
      k = next;
    }
    return root;
  }
  uint64_t find_const(uint64_t k) const {  // a key no unit edge holds is its own set
    auto it = e.find(k);
    if (it == e.end()) return k;
    while (it->second.parent != it->first) it = e.find(it->second.parent);
    return it->first;
  }
  void merge(uint64_t x, uint64_t y) {
    const uint64_t xr = find(x), yr = find(y);
    if (xr == yr) return;
    if (e[xr].rank < e[yr].rank) e[xr].parent = yr;
    else if (e[xr].rank > e[yr].rank) e[yr].parent = xr;
    else {
      e[yr].parent = xr;
      e[xr].rank += 1;
    }
  }
};

struct Edge {
  uint64_t k1, k2;
  double z[3];
  int32_t kind;
  const double* noise;
  int64_t n_noise;
};

// std::uniform_real_distribution<double>(-1, 1) on std::mt19937 as libstdc++ and libc++ form it: generate_canonical takes
// two 32-bit outputs, (x0 + x1 2^32) / 2^64 in double, then (b - a) r + a
double draw(std::mt19937& rng) {
  const double x0 = (double)rng(), x1 = (double)rng();
  double r = (x0 + x1 * 4294967296.0) / 18446744073709551616.0;
  if (r >= 1.0) r = std::nextafter(1.0, 0.0);
  return 2.0 * r + -1.0;
}

bool is_zero_direction(const double* z) {  // Unit3::equals(Unit3(0, 0, 0), 1e-9): equal_with_abs_tol on the 3 components
  return std::fabs(z[0]) <= 1e-9 && std::fabs(z[1]) <= 1e-9 && std::fabs(z[2]) <= 1e-9;
}

struct Built {
  gsx_dataset* D = nullptr;
  std::vector<uint64_t> translation_keys;            // the VECTOR(3) variables, ascending
  std::vector<uint64_t> merged_keys, merged_into;    // members of the sets that are not their root, and that root
};

gsx_status build(const gsx_translation_input* in, const gsx_translation_params* p, Built& B) {
  if (!in || !p || in->n_unit < 0 || in->n_between < 0 || in->n_given < 0 || in->n_unit > INT32_MAX / 4 ||
      in->n_between > INT32_MAX / 4 || !(p->prior_sigma > 0) || !std::isfinite(p->prior_sigma) || !std::isfinite(in->scale))
    return GSX_E_INVALID;
  if (in->n_unit > 0 && (!in->unit_key1 || !in->unit_key2 || !in->unit_dirs || !in->unit_noise_kind || !in->unit_noise_ptr))
    return GSX_E_INVALID;
  if (in->n_between > 0 &&
      (!in->between_key1 || !in->between_key2 || !in->between_meas || !in->between_noise_kind || !in->between_noise_ptr))
    return GSX_E_INVALID;
  if (in->n_given > 0 && (!in->given_keys || !in->given_values)) return GSX_E_INVALID;
  auto noise_ok = [](const int64_t* ptr, const double* data, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
      if (ptr[i + 1] < ptr[i] || ptr[i] < 0) return false;
    return n == 0 || ptr[n] == ptr[0] || data != nullptr;
  };
  if (!noise_ok(in->unit_noise_ptr, in->unit_noise, in->n_unit) ||
      !noise_ok(in->between_noise_ptr, in->between_noise, in->n_between))
    return GSX_E_INVALID;

  // getSameTranslationDSFMap (:49-60)
  Dsf dsf;
  for (int64_t i = 0; i < in->n_unit; ++i) {
    const uint64_t a = dsf.find(in->unit_key1[i]), b = dsf.find(in->unit_key2[i]);
    if (a != b && is_zero_direction(in->unit_dirs + 3 * i)) dsf.merge(a, b);
  }
  // removeSameTranslationNodes (:65-76) on both lists
  auto keep = [&](int64_t n, const uint64_t* k1, const uint64_t* k2, const double* z, const int32_t* kind, const int64_t* ptr,
                  const double* noise, std::vector<Edge>& out) {
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = dsf.find_const(k1[i]), b = dsf.find_const(k2[i]);
      if (a == b) continue;
      out.push_back(Edge{a, b, {z[3 * i], z[3 * i + 1], z[3 * i + 2]}, kind[i], noise ? noise + ptr[i] : nullptr,
                         ptr[i + 1] - ptr[i]});
    }
  };
  std::vector<Edge> unit, between;
  keep(in->n_unit, in->unit_key1, in->unit_key2, in->unit_dirs, in->unit_noise_kind, in->unit_noise_ptr, in->unit_noise, unit);
  keep(in->n_between, in->between_key1, in->between_key2, in->between_meas, in->between_noise_kind, in->between_noise_ptr,
       in->between_noise, between);

  // initializeRandomly (:145-181): first-appearance order, a fresh generator per call
  std::map<uint64_t, const double*> given;
  for (int64_t i = 0; i < in->n_given; ++i) given.emplace(in->given_keys[i], in->given_values + 3 * i);
  std::mt19937 rng(p->seed);
  std::map<uint64_t, std::vector<double>> initial;   // key -> state (3 doubles, or 1 for a scale)
  auto insert = [&](uint64_t j) {
    if (initial.count(j)) return;
    auto g = given.find(j);
    if (g != given.end()) {
      initial[j] = {g->second[0], g->second[1], g->second[2]};
    } else {
      const double x = draw(rng), y = draw(rng), z = draw(rng);
      initial[j] = {x, y, z};
    }
  };
  for (const Edge& e : unit) { insert(e.k1); insert(e.k2); }
  for (const Edge& e : between) { insert(e.k1); insert(e.k2); }
  // no valid edge, but zero-distance edges: one node per set at the origin (:216-223)
  if (initial.empty())
    for (const auto& kv : dsf.e)
      if (dsf.find_const(kv.first) == kv.first) initial[kv.first] = {0.0, 0.0, 0.0};
  for (const auto& kv : initial) B.translation_keys.push_back(kv.first);
  if (p->use_bilinear)
    for (size_t i = 0; i < unit.size(); ++i) {
      const uint64_t s = ((uint64_t)'S' << 56) | (uint64_t)i;   // Symbol('S', i) (gtsam/inference/Symbol.cpp)
      if (initial.count(s)) return GSX_E_INVALID;               // a translation key that collides with a scale key
      initial[s] = {1.0};
    }
  for (const auto& kv : dsf.e) {
    const uint64_t root = dsf.find_const(kv.first);
    if (root != kv.first) {
      B.merged_keys.push_back(kv.first);
      B.merged_into.push_back(root);
    }
  }

  gsx_dataset* D = new (std::nothrow) gsx_dataset();
  if (!D) return GSX_E_NOMEM;
  B.D = D;
  std::map<uint64_t, int32_t> index;
  for (const auto& kv : initial) {
    index[kv.first] = (int32_t)D->var_keys.size();
    D->var_keys.push_back(kv.first);
    D->var_types.push_back(GSX_VAR_VECTOR);
    D->var_dims.push_back((int32_t)kv.second.size());
    D->values.insert(D->values.end(), kv.second.begin(), kv.second.end());
  }
  D->f_key_ptr.push_back(0);
  D->f_meas_ptr.push_back(0);
  D->f_noise_ptr.push_back(0);
  auto add = [&](int32_t type, std::initializer_list<uint64_t> keys, const double* z, int32_t kind, const double* noise,
                 int64_t n_noise) {
    D->f_type.push_back(type);
    D->f_rows.push_back(3);
    for (uint64_t k : keys) D->f_vars.push_back(index[k]);
    D->f_key_ptr.push_back((int32_t)D->f_vars.size());
    D->meas.insert(D->meas.end(), z, z + 3);
    D->f_meas_ptr.push_back((int64_t)D->meas.size());
    D->f_noise_kind.push_back(kind);
    if (n_noise > 0) D->noise.insert(D->noise.end(), noise, noise + n_noise);
    D->f_noise_ptr.push_back((int64_t)D->noise.size());
  };
  // buildGraph (:99-117)
  for (size_t i = 0; i < unit.size(); ++i) {
    const Edge& e = unit[i];
    if (p->use_bilinear)
      add(GSX_F_BILINEAR_TRANSLATION, {e.k1, e.k2, ((uint64_t)'S' << 56) | (uint64_t)i}, e.z, e.kind, e.noise, e.n_noise);
    else
      add(GSX_F_TRANSLATION, {e.k1, e.k2}, e.z, e.kind, e.noise, e.n_noise);
  }
  // addPrior (:119-143)
  if (!unit.empty()) {
    const Edge& e = unit.front();
    const double origin[3] = {0.0, 0.0, 0.0}, sigma = p->prior_sigma;
    add(GSX_F_PRIOR, {e.k1}, origin, GSX_NOISE_ISOTROPIC, &sigma, 1);
    if (between.empty()) {
      const double sz[3] = {in->scale * e.z[0], in->scale * e.z[1], in->scale * e.z[2]};
      add(GSX_F_PRIOR, {e.k2}, sz, e.kind, e.noise, e.n_noise);
    } else {
      for (const Edge& b : between) add(GSX_F_BETWEEN, {b.k1, b.k2}, b.z, b.kind, b.noise, b.n_noise);
    }
  }
  // the description must be one gsx_create takes: noise models sized for m = 3, no key twice in a factor, ...
  gsx_problem_desc v;
  gsx_dataset_get(D, &v, nullptr, nullptr);
  gsx::HostProblem P;
  return gsx::lower_problem(&v, P, D->err);
}

}  // namespace

extern "C" {

void gsx_translation_params_default(gsx_translation_params* p) {
  if (!p) return;
  gsx_lm_params_legacy(&p->lm);
  p->use_bilinear = 0;
  p->seed = 42;
  p->prior_sigma = 0.01;
}

gsx_status gsx_translation_recovery_problem(const gsx_translation_input* in, const gsx_translation_params* p, gsx_dataset** out,
                                            uint64_t* merged_keys, uint64_t* merged_into, int64_t* n_merged) {
  if (!out) return GSX_E_INVALID;
  *out = nullptr;
  Built B;
  const gsx_status st = build(in, p, B);
  if (st != GSX_OK) {
    delete B.D;
    return st;
  }
  if (merged_keys) std::copy(B.merged_keys.begin(), B.merged_keys.end(), merged_keys);
  if (merged_into) std::copy(B.merged_into.begin(), B.merged_into.end(), merged_into);
  if (n_merged) *n_merged = (int64_t)B.merged_keys.size();
  *out = B.D;
  return GSX_OK;
}

gsx_status gsx_translation_recovery(const gsx_translation_input* in, const gsx_translation_params* p, int32_t device,
                                    uint64_t* keys_out, double* translations_out, int64_t* n_out, gsx_lm_result* r) {
  if (!keys_out || !translations_out || !n_out) return GSX_E_INVALID;
  Built B;
  gsx_status st = build(in, p, B);
  struct Free {
    gsx_dataset* d;
    gsx_handle h = nullptr;
    ~Free() {
      if (h) gsx_destroy(h);
      delete d;
    }
  } guard{B.D};
  if (st != GSX_OK) return st;
  gsx_dataset* D = B.D;
  std::vector<double> values = D->values;
  if (r) {
    r->initial_error = r->final_error = r->final_lambda = 0.0;
    r->iterations = r->inner_iterations = r->n_solve_failures = r->trace_len = 0;
  }
  if (!D->f_type.empty()) {   // (an empty graph leaves the initial values: LM has nothing to do)
    gsx_problem_desc v;
    gsx_dataset_get(D, &v, nullptr, nullptr);
    st = gsx_create(&v, device, &guard.h);
    if (st != GSX_OK) return st;
    std::vector<uint64_t> ord(D->var_keys.size());
    st = gsx_compute_ordering(guard.h, GSX_ORDER_MINDEGREE, ord.data());
    if (st == GSX_OK) st = gsx_set_ordering(guard.h, ord.data(), (int32_t)ord.size());
    if (st == GSX_OK) st = gsx_set_values(guard.h, values.data(), (int64_t)values.size());
    gsx_lm_result local;
    std::memset(&local, 0, sizeof local);
    if (st == GSX_OK) st = gsx_lm_optimize(guard.h, &p->lm, r ? r : &local);
    if (st == GSX_OK) st = gsx_get_values(guard.h, values.data(), (int64_t)values.size());
    if (st != GSX_OK) return st;
  }
  // the translation variables, then addSameTranslationNodes (:80-97)
  std::map<uint64_t, const double*> at;
  int64_t off = 0, n = 0;
  for (size_t v = 0; v < D->var_keys.size(); ++v) {
    if (D->var_dims[v] == 3 && std::binary_search(B.translation_keys.begin(), B.translation_keys.end(), D->var_keys[v])) {
      at[D->var_keys[v]] = values.data() + off;
      keys_out[n] = D->var_keys[v];
      std::copy(values.data() + off, values.data() + off + 3, translations_out + 3 * n);
      ++n;
    }
    off += D->var_dims[v];
  }
  for (size_t i = 0; i < B.merged_keys.size(); ++i) {
    auto it = at.find(B.merged_into[i]);
    if (it == at.end() || at.count(B.merged_keys[i])) continue;
    keys_out[n] = B.merged_keys[i];
    std::copy(it->second, it->second + 3, translations_out + 3 * n);
    ++n;
  }
  *n_out = n;
  return GSX_OK;
}

}  // extern "C"
