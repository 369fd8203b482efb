// upload.hip — the device tables of a handle: the problem (gsx_create, gsx_update) and the symbolic factorization with its
// launch plan (gsx_set_ordering, gsx_update).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <array>
#include <map>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsx;

namespace gsx {

// INVARIANT: the length handed to type_list_of / absolute_kind_of is that of the handle's OWN measurement table, which
// lower_problem lengthens for GSX_F_ATTITUDE (6 doubles from the caller, 12 with B behind them).  Both functions decide by
// length only for GSX_F_PROJECTION, _STEREO, _RANGE and GSX_F_GPS, whose entries lower_problem leaves as given; a type whose
// entry it lengthens must not be told apart by length.
// the list of factor f (kernels.h: type_list_of; the types of its first two variables pick the family's variant, the
// length of its measurement the form with body_P_sensor)
int factor_type_list(const HostProblem& P, int f) {
  const int kp = P.f_key_ptr[f], nk = P.f_key_ptr[f + 1] - kp;
  return type_list_of(P.f_type[f], nk > 0 ? P.types[P.f_vars[kp]] : -1, nk > 1 ? P.types[P.f_vars[kp + 1]] : -1,
                      P.f_meas_ptr[f + 1] - P.f_meas_ptr[f]);
}
int factor_absolute_kind(const HostProblem& P, int f) {
  const int kp = P.f_key_ptr[f], nk = P.f_key_ptr[f + 1] - kp;
  const int k = absolute_kind_of(P.f_type[f], nk > 0 ? P.types[P.f_vars[kp]] : -1, nk > 1 ? P.types[P.f_vars[kp + 1]] : -1,
                                 P.f_meas_ptr[f + 1] - P.f_meas_ptr[f]);
  return k < 0 ? 0 : k;
}
void sort_absolute_list(const HostProblem& P, std::vector<int>& list) {
  std::stable_sort(list.begin(), list.end(), [&](int a, int b) { return factor_absolute_kind(P, a) < factor_absolute_kind(P, b); });
}
// factor lists of the linearize kernels (one per factor family) and of the error kernels; `owned` (may be null: all)
// restricts them to the factors this rank evaluates
gsx_status upload_factor_lists(gsx_context* c, const std::vector<char>* owned) {
  const HostProblem& P = c->P;
  hipStream_t st = c->stream;
  std::vector<int> lists[kNumTypeLists], active;
  for (int f = 0; f < P.n_factors; ++f) {
    if (owned && !(*owned)[f]) continue;
    active.push_back(f);
    const int k = factor_type_list(P, f);
    if (k >= 0) lists[k].push_back(f);
  }
  sort_absolute_list(P, lists[TL_ABSOLUTE]);
  for (int k = 0; k < kNumTypeLists; ++k) {
    c->type_count[k] = (int)lists[k].size();
    HIPCHK(c, c->d_type_list[k].upload(lists[k], st));
  }
  if (owned) {
    HIPCHK(c, c->d_f_active.upload(active, st));
    c->DP.f_active = c->d_f_active.p;
  } else {
    c->DP.f_active = nullptr;
  }
  c->DP.n_active = (int)active.size();
  HIPCHK(c, hipStreamSynchronize(st));
  return GSX_OK;
}

// [A b] of a GSX_F_LINEAR factor with its noise model folded in: data preparation of a GIVEN linear factor
// (JacobianFactor::whiten, gtsam/linear/JacobianFactor.cpp), on the host
void whiten_linear_factor(const HostProblem& P, int f, const double* src, double* J) {
  const int m = P.f_rows[f], nc = P.f_cols[f];
  std::copy(src, src + (size_t)m * nc, J);
  const double* np = P.noise.data() + P.f_noise_ptr[f];
  const int kind = P.f_noise_kind[f];
  for (int cidx = 0; cidx < nc; ++cidx) {
    if (kind == GSX_NOISE_ISOTROPIC)
      for (int r = 0; r < m; ++r) J[cidx * m + r] *= 1.0 / np[0];
    else if (kind == GSX_NOISE_DIAGONAL)
      for (int r = 0; r < m; ++r) J[cidx * m + r] *= 1.0 / np[r];
    else if (kind == GSX_NOISE_GAUSSIAN)
      for (int r = 0; r < m; ++r) {
        double sacc = 0;
        for (int k = r; k < m; ++k) sacc += np[r * m + k] * J[cidx * m + k];
        J[cidx * m + r] = sacc;
      }
  }
}

gsx_status upload_problem(gsx_context* c) {
  const HostProblem& P = c->P;
  hipStream_t st = c->stream;
  pcg_work_destroy(c->pcg);
  c->pcg = nullptr;
  HIPCHK(c, c->d_var_type.upload(P.types, st));
  HIPCHK(c, c->d_var_dim.upload(P.dims, st));
  HIPCHK(c, c->d_var_state_off.upload(P.state_off, st));
  HIPCHK(c, c->d_var_tan_off.upload(P.tan_off, st));
  HIPCHK(c, c->d_f_type.upload(P.f_type, st));
  HIPCHK(c, c->d_f_rows.upload(P.f_rows, st));
  HIPCHK(c, c->d_f_key_ptr.upload(P.f_key_ptr, st));
  HIPCHK(c, c->d_f_vars.upload(P.f_vars, st));
  HIPCHK(c, c->d_f_noise_kind.upload(P.f_noise_kind, st));
  HIPCHK(c, c->d_f_cols.upload(P.f_cols, st));
  std::vector<i64> mo(P.f_meas_ptr.begin(), P.f_meas_ptr.end()), no(P.f_noise_ptr.begin(), P.f_noise_ptr.end()),
      jo(P.f_jac_off.begin(), P.f_jac_off.end());
  HIPCHK(c, c->d_f_meas_off.upload(mo, st));
  HIPCHK(c, c->d_f_noise_off.upload(no, st));
  HIPCHK(c, c->d_f_jac_off.upload(jo, st));
  {
    // the largest [A b] range of 64 consecutive factors (the blocks are laid out in factor order)
    int64_t worst = 0;
    bool ordered = true;
    for (int i0 = 0; i0 < P.n_factors; i0 += 64) {
      const int l = std::min(P.n_factors, i0 + 64) - 1;
      worst = std::max<int64_t>(worst, P.f_jac_off[l] + (int64_t)P.f_rows[l] * P.f_cols[l] - P.f_jac_off[i0]);
    }
    for (int f = 1; f < P.n_factors; ++f) ordered = ordered && P.f_jac_off[f] >= P.f_jac_off[f - 1];
    worst = (worst + 1) & ~(int64_t)1;
    c->lin_err_slice = (ordered && worst > 0 && 2 * worst * (int64_t)sizeof(double) <= 96 * 1024) ? (int)worst : 0;
  }
  HIPCHK(c, c->d_meas.upload(P.meas, st));
  HIPCHK(c, c->d_noise.upload(P.noise, st));
  c->con_hd_n = 0;
  if (!P.con_factor.empty()) {
    struct E {
      int tan;
      i64 jidx;
      double w;
    };
    std::vector<E> es;
    for (size_t i = 0; i < P.con_factor.size(); ++i) {
      const int f = P.con_factor[i], m = P.f_rows[f];
      int col = 0;
      for (int q = P.f_key_ptr[f]; q < P.f_key_ptr[f + 1]; ++q)
        for (int d = 0; d < P.dims[P.f_vars[q]]; ++d, ++col)
          es.push_back(E{P.tan_off[P.f_vars[q]] + d, P.f_jac_off[f] + (i64)col * m + P.con_row[i], 1.0 - 1.0 / P.con_mu[i]});
    }
    std::stable_sort(es.begin(), es.end(), [](const E& a, const E& b) { return a.tan < b.tan; });
    std::vector<int> tan, ptr;
    std::vector<i64> jidx;
    std::vector<double> w;
    for (const E& e : es) {
      if (tan.empty() || tan.back() != e.tan) {
        tan.push_back(e.tan);
        ptr.push_back((int)jidx.size());
      }
      jidx.push_back(e.jidx);
      w.push_back(e.w);
    }
    ptr.push_back((int)jidx.size());
    c->con_hd_n = (int)tan.size();
    HIPCHK(c, c->d_con_hd_tan.upload(tan, st));
    HIPCHK(c, c->d_con_hd_ptr.upload(ptr, st));
    HIPCHK(c, c->d_con_hd_jidx.upload(jidx, st));
    HIPCHK(c, c->d_con_hd_w.upload(w, st));
  }
  gsx_status fl = upload_factor_lists(c, nullptr);
  if (fl != GSX_OK) return fl;
  if (c->n_smart) {
    std::vector<int> slot(P.n_factors, -1), never(c->n_smart, -1);
    int ns = 0;
    for (int f = 0; f < P.n_factors; ++f)
      if (P.f_type[f] == GSX_F_SMART_PROJECTION) slot[f] = ns++;
    HIPCHK(c, c->d_smart_slot.upload(slot, st));
    HIPCHK(c, c->d_smart_status.upload(never, st));
    HIPCHK(c, c->d_smart_counters.alloc(2));
    HIPCHK(c, c->d_smart_cams.alloc((size_t)ns * 8 * 32));
    HIPCHK(c, c->d_smart_cache.alloc((size_t)ns * 8 * 12));
    HIPCHK(c, c->d_smart_point.alloc((size_t)ns * 3));
    HIPCHK(c, hipMemsetAsync(c->d_smart_counters.p, 0, 2 * sizeof(int), st));
    HIPCHK(c, hipMemsetAsync(c->d_smart_cache.p, 0, (size_t)ns * 8 * 12 * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(c->d_smart_point.p, 0xFF, (size_t)ns * 3 * sizeof(double), st));   // (all-ones bytes are a NaN)
    c->SD = SmartDev{c->d_smart_slot.p, c->d_smart_cams.p, c->d_smart_cache.p, c->d_smart_point.p, c->d_smart_status.p,
                     c->d_smart_counters.p, ns};
  } else {
    c->SD = SmartDev{};
  }
  HIPCHK(c, c->d_values.alloc(std::max<int64_t>(P.state_size, 1)));
  HIPCHK(c, c->d_trial.alloc(std::max<int64_t>(P.state_size, 1)));
  HIPCHK(c, c->d_delta.alloc(std::max<int64_t>(P.tan_size, 1)));
  HIPCHK(c, c->d_udelta.alloc(std::max<int64_t>(P.tan_size, 1)));
  HIPCHK(c, c->d_hdiag.alloc(std::max<int64_t>(P.tan_size, 1)));
  HIPCHK(c, c->d_damp.alloc(std::max<int64_t>(P.tan_size, 1)));
  HIPCHK(c, c->d_jac.alloc(std::max<int64_t>(P.jac_size, 1)));
  HIPCHK(c, c->d_partials.alloc(gsx_context::kPartials));
  HIPCHK(c, c->d_scalars.alloc(SC_COUNT));
  HIPCHK(c, c->d_status.alloc(1));
  if (!c->h_scalars) HIPCHK(c, hipHostMalloc((void**)&c->h_scalars, SC_COUNT * sizeof(double)));  // (gsx_update comes here again)
  if (!c->h_status) HIPCHK(c, hipHostMalloc((void**)&c->h_status, sizeof(DevStatus)));
  HIPCHK(c, hipMemsetAsync(c->d_scalars.p, 0, SC_COUNT * sizeof(double), st));
  HIPCHK(c, hipMemsetAsync(c->d_delta.p, 0, std::max<int64_t>(P.tan_size, 1) * sizeof(double), st));
  // LINEAR factors: their (whitened) [A b] as given at creation (gsx_set_block_jacobians refreshes them in place)
  {
    std::vector<double> jac;
    bool any = false;
    for (int f = 0; f < P.n_factors; ++f) any = any || P.f_type[f] == GSX_F_LINEAR;
    if (any) {
      jac.assign(P.jac_size, 0.0);
      for (int f = 0; f < P.n_factors; ++f)
        if (P.f_type[f] == GSX_F_LINEAR) whiten_linear_factor(P, f, P.meas.data() + P.f_meas_ptr[f], jac.data() + P.f_jac_off[f]);
      HIPCHK(c, hipMemcpyAsync(c->d_jac.p, jac.data(), jac.size() * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(c, hipStreamSynchronize(st));
    }
  }
  {
    // one 32-byte record per factor (kernels.h: FactorRec)
    if (P.meas.size() >= (size_t)INT32_MAX || P.noise.size() >= (size_t)INT32_MAX || P.state_size >= INT32_MAX) {
      c->err = "problem too large for 32-bit measurement / noise / state offsets";
      return GSX_E_INVALID;
    }
    std::vector<FactorRec> fr(std::max(P.n_factors, 1));
    for (int f = 0; f < P.n_factors; ++f) {
      if (P.f_cols[f] >= 32768 || P.f_rows[f] > 255) {
        c->err = "factor too wide for the packed factor record";
        return GSX_E_INVALID;
      }
      const int kp = P.f_key_ptr[f], nk = P.f_key_ptr[f + 1] - kp;
      const int v0 = nk > 0 ? P.f_vars[kp] : -1, v1 = nk > 1 ? P.f_vars[kp + 1] : -1;
      fr[f] = FactorRec{(i64)P.f_jac_off[f], v0 >= 0 ? P.state_off[v0] : -1, v1 >= 0 ? P.state_off[v1] : -1,
                        (int)P.f_meas_ptr[f], (int)P.f_noise_ptr[f],
                        P.f_type[f] | (P.f_noise_kind[f] << 8) | (factor_absolute_kind(P, f) << 16) |
                            ((v0 >= 0 ? P.types[v0] : 0) << 24),
                        P.f_rows[f] | (std::min(v0 >= 0 ? P.dims[v0] : 0, 255) << 8) | (P.f_cols[f] << 16)};
    }
    HIPCHK(c, c->d_frec.upload(fr, st));
  }
  DevProblem& D = c->DP;
  D.n_vars = P.n_vars;
  D.n_factors = P.n_factors;
  D.frec = c->d_frec.p;
  D.var_type = c->d_var_type.p; D.var_dim = c->d_var_dim.p;
  D.var_state_off = c->d_var_state_off.p; D.var_tan_off = c->d_var_tan_off.p;
  D.f_type = c->d_f_type.p; D.f_rows = c->d_f_rows.p; D.f_key_ptr = c->d_f_key_ptr.p; D.f_vars = c->d_f_vars.p;
  D.f_noise_kind = c->d_f_noise_kind.p; D.f_cols = c->d_f_cols.p;
  D.f_meas_off = c->d_f_meas_off.p; D.f_noise_off = c->d_f_noise_off.p; D.f_jac_off = c->d_f_jac_off.p;
  D.meas = c->d_meas.p; D.noise = c->d_noise.p;
  HIPCHK(c, hipStreamSynchronize(st));
  return GSX_OK;
}

// (ScheduleOptions::small_threads_shift: twice the threads the row-per-thread panel needed)
static int small_threads_for(const gsx_context* c, int n) {
  int t = 512;
  if (n <= 48) t = 64;
  else if (n <= 72) t = 128;
  else if (n <= 100) t = 256;
  return std::min(512, t << c->opt.small_threads_shift);
}

// ---- the back-substitution's launch plan (handle.h: BsLaunch) -----------------------------------------------------------
// The launches of one level's fronts above the leaf kernel: ids[sb, mid) the LDS-class ones, ids[mid, e) the blocked ones.
// Each class has a kernel of its own that takes the class whole or not at all (backsolve_small_fits, backsolve_big_lds);
// what they refuse goes to the generic kernel, which keeps only n - 1 doubles a front in LDS — the factorization's size
// groups mean nothing to it, a class is ONE launch.
// (A gap, recorded and left: launch_backsolve asks for max_n doubles of LDS against an attribute of 128 KB and nothing
//  here refuses a front beyond that, as lds_fits does for the factorization — a front of more than 16 384 rows.)
// level_sched: the schedule of all fronts (S.sched).  There, and only there, few generic fronts of both classes share one
// launch, and the classes with a kernel of their own go first; the upper schedule runs the blocked fronts, then the others.
static void plan_bs_group(const Symbolic& S, const std::vector<int>& ids, int level, int sb, int mid, int e, bool level_sched,
                          std::vector<BsLaunch>& out) {
  auto range = [&](int b, int end, int threads) {
    BsLaunch r{BS_GENERIC, level, b, end - b, 0, 0, threads};
    for (int k = b; k < end; ++k) {
      r.max_n = std::max(r.max_n, S.N[ids[k]]);
      r.max_F = std::max(r.max_F, S.F[ids[k]]);
    }
    return r;
  };
  BsLaunch big = range(mid, e, 1024), small = range(sb, mid, 0);
  small.threads = small.max_n <= 48 ? 64 : 256;
  int big_sep = 0;
  for (int k = mid; k < e; ++k) big_sep = std::max(big_sep, S.N[ids[k]] - S.F[ids[k]]);
  if (big.count && backsolve_big_lds(big.max_n, big.max_F, big_sep) > 0) big.kind = BS_BIG;
  if (small.count && backsolve_small_fits(small.max_n, small.max_F)) small.kind = BS_SMALL;
  if (big.kind != BS_GENERIC) big.threads = 0;
  if (small.kind != BS_GENERIC) small.threads = 0;
  const int n_rest = e - sb;
  if (level_sched && big.count && small.count && big.kind == BS_GENERIC && small.kind == BS_GENERIC && n_rest <= 512 &&
      n_rest > big.count) {
    out.push_back(range(sb, e, 1024));   // few fronts: small and big ones of the level in ONE launch of the generic kernel
    return;
  }
  const bool small_first = level_sched && big.kind == BS_GENERIC && small.kind == BS_SMALL;
  const BsLaunch* order[2] = {small_first ? &small : &big, small_first ? &big : &small};
  for (const BsLaunch* b : order)
    if (b->count) out.push_back(*b);
}

// Both plans of a tree, from the symbolic analysis alone (no handle, no device): what every solve then only walks.
void plan_backsolve(const Symbolic& S, std::vector<BsLaunch>& level_plan, std::vector<BsLaunch>& plan) {
  level_plan.clear();
  plan.clear();
  auto leaves = [&](int l) { return BsLaunch{BS_LEAF, l, S.lvl_ptr[l], S.lvl_leaf_end[l] - S.lvl_ptr[l], 0, 0, 0}; };
  for (int l = S.n_levels - 1; l >= 0; --l) {
    plan_bs_group(S, S.sched, l, S.lvl_leaf_end[l], S.lvl_small_end[l], S.lvl_ptr[l + 1], true, level_plan);
    if (leaves(l).count) level_plan.push_back(leaves(l));
  }
  // OptimizeClique top-down: the upper fronts level by level (Symbolic::ulevel), then — every upper front solved — the tree
  // fronts of all levels in one launch, then the leaf-kernel cliques (childless: level 0)
  for (int l = S.n_ulevels - 1; l >= 0; --l)
    plan_bs_group(S, S.usched, l, S.ulvl_ptr[l], S.ulvl_small_end[l], S.ulvl_ptr[l + 1], false, plan);
  BsLaunch tree{BS_TREE, 0, 0, 0, 0, 0, 0};
  for (int f = 0; f < S.n_fronts; ++f)
    if (S.tree_tier[f] >= 0) {
      tree.count++;
      tree.max_n = std::max(tree.max_n, S.N[f]);
      tree.max_F = std::max(tree.max_F, S.F[f]);
    }
  if (tree.count) plan.push_back(tree);
  if (S.n_levels > 0 && leaves(0).count) plan.push_back(leaves(0));
}

// (for tests/test_host_backsolve_plan.py: the plans as integers, host only; not part of the C ABI of include/gsx.h.  A
//  handle without a device never reached upload_symbolic: it is planned here.)  which = 0: the level plan, a record
// (front, kind, threads, max_F, launch) per front in launch order; 1: the default plan, a record (kind, level, count,
// threads, max_n) per launch.  For a leaf-kernel clique `threads` is the lanes it is solved with: leaf_pack_class, or a wave
// when the handle does not pack.  Returns the number of records, of which the first `cap` are written.
extern "C" int gsxtest_backsolve_plan(gsx_context* c, int which, int* out, int cap) {
  if (!c || !c->has_symbolic) return -1;
  const Symbolic& S = c->S;
  std::vector<BsLaunch> level_plan = c->bs_level_plan, plan = c->bs_plan;
  if (!c->has_device) plan_backsolve(S, level_plan, plan);
  std::vector<std::array<int, 5>> recs;
  for (const BsLaunch& b : plan)
    if (which == 1) recs.push_back({b.kind, b.level, b.count, b.threads, b.max_n});
  for (size_t i = 0; which == 0 && i < level_plan.size(); ++i) {
    const BsLaunch& b = level_plan[i];
    const bool packs = b.kind == BS_LEAF && b.level == 0 && c->opt.bs_leaf_pack;
    int leaf_max_F = 0;
    for (int k = b.begin; packs && k < b.begin + b.count; ++k) leaf_max_F = std::max(leaf_max_F, S.F[S.sched[k]]);
    for (int k = b.begin; k < b.begin + b.count; ++k) {
      const int f = S.sched[k];
      const int lanes = packs ? leaf_pack_class(S.N[f], S.F[f], leaf_max_F) : 64;
      recs.push_back({f, b.kind, b.kind == BS_LEAF ? lanes : b.threads, b.max_F, (int)i});
    }
  }
  for (size_t i = 0; out && i < recs.size() && (int)i < cap; ++i) std::copy(recs[i].begin(), recs[i].end(), out + 5 * i);
  return (int)recs.size();
}

// The star records of one launch group as front_star_leaf_kernel takes them: a stable partition by the lanes a clique gets
// (kernels.h: star_leaf_pack_class; !pack: every clique a wave, the table stays as it is).  n16, n32: the leading classes.
// The arena rows of different cliques are disjoint, so their order changes no result.
static void partition_star_leaves(StarLeafRec* recs, int count, bool pack, int& n16, int& n32) {
  n16 = n32 = 0;
  if (!pack) return;
  auto lanes = [](const StarLeafRec& r) { return star_leaf_pack_class(r.nf, r.dB); };
  StarLeafRec* m = std::stable_partition(recs, recs + count, [&](const StarLeafRec& r) { return lanes(r) == 16; });
  StarLeafRec* e = std::stable_partition(m, recs + count, [&](const StarLeafRec& r) { return lanes(r) == 32; });
  n16 = (int)(m - recs);
  n32 = (int)(e - m);
}

// (for tests/test_host_star_leaf_partition.py, host only; not part of the C ABI of include/gsx.h.)  The partition above of
// `count` records of nf[i] factors and partners of dimension dB[i]: order[k] = the index i of the record at place k,
// counts = the cliques of 16 lanes, of 32 lanes and of a wave.
extern "C" void gsxtest_star_leaf_partition(const int* nf, const int* dB, int count, int pack, int* order, int* counts) {
  std::vector<StarLeafRec> recs((size_t)count);
  for (int i = 0; i < count; ++i) {
    recs[i] = StarLeafRec{};
    recs[i].nf = nf[i];
    recs[i].dB = dB[i];
    recs[i].front = i;
  }
  partition_star_leaves(recs.data(), count, pack != 0, counts[0], counts[1]);
  counts[2] = count - counts[0] - counts[1];
  for (int k = 0; k < count; ++k) order[k] = recs[k].front;
}
// (for tests/test_gpu_star_leaf_packed.py.)  Per launch group of the leaf-kernel cliques a record (cliques of 16 lanes, of
// 32 lanes, of a wave, leaves that are no star leaves); returns the number of groups — 0 when the handle does not fuse.
extern "C" int gsxtest_star_leaf_classes(gsx_context* c, int* out, int cap) {
  if (!c || !c->fused_star) return 0;
  for (size_t g = 0; out && g < c->leaf_split.size() && (int)g < cap; ++g) {
    const gsx_context::LeafSplit& ls = c->leaf_split[g];
    const int r[4] = {ls.s16, ls.s32, ls.scount - ls.s16 - ls.s32, ls.rcount};
    std::copy(r, r + 4, out + 4 * g);
  }
  return (int)c->leaf_split.size();
}

// ---- H assembly groups: variables bucketed by panel size (LDS) and term count (host only: gsx_get_hessian_groups
//      reads the plan, and makes it itself on a handle without a device) ----
void plan_hessian_groups(gsx_context* c) {
  const Symbolic& S = c->S;
  const HostProblem& P = c->P;
  struct VI {
    int v, psize;
    int64_t terms;
  };
  std::vector<VI> light, heavy, huge, diag, star, tile;
  // a "tile" variable: at most 64 terms, all from NARROW factors (<= 16 columns with the rhs, <= 8 rows): one matrix-core
  // product per factor (assemble_h_tile_kernel).  ScheduleOptions::h_tile off keeps the generic kernel (measurements).
  auto is_tile = [&](int v) {
    const int64_t tb = S.term_ptr[v], te = S.term_ptr[v + 1];
    if (!c->opt.h_tile || te - tb < 2 || te - tb > 64 || (int64_t)S.h_rows[v] * P.dims[v] * 8 * 4 > 48 * 1024) return false;
    int64_t t = tb;
    while (t < te) {
      int64_t e = t + 1;
      while (e < te && S.t_jac[e] == S.t_jac[t]) ++e;
      // the factor's last term is its rhs term: column index = number of columns - 1
      if (S.t_m[t] > 8 || S.t_dB[e - 1] != 1 || S.t_dst[e - 1] != S.h_rows[v] - 1 || S.t_colB[e - 1] + 1 > 16) return false;
      t = e;
    }
    return true;
  };
  // a "star" variable: all its factors are binary with a later-eliminated partner, all of one shape (three terms
  // each: own block, partner block, rhs — with equal rows, columns and partner dimension)
  std::vector<int> star_dst;
  auto is_star = [&](int v) {
    const int64_t tb = S.term_ptr[v], te = S.term_ptr[v + 1];
    if (te - tb < 3 || (te - tb) % 3 != 0 || P.dims[v] > 7) return false;
    star_dst.clear();
    for (int64_t t = tb; t < te; t += 3) {
      star_dst.push_back(S.t_dst[t + 1]);
      if (S.t_dst[t] != 0 || S.t_dst[t + 2] != S.h_rows[v] - 1 || S.t_dB[t + 2] != 1) return false;
      if (S.t_dst[t + 1] == 0 || S.t_dst[t + 1] == S.h_rows[v] - 1) return false;
      if (S.t_m[t] != S.t_m[tb] || S.t_colA[t] != S.t_colA[tb] || S.t_colB[t + 1] != S.t_colB[tb + 1] ||
          S.t_dB[t + 1] != S.t_dB[tb + 1] || S.t_colB[t + 2] != S.t_colB[tb + 2] || S.t_jac[t] != S.t_jac[t + 1] ||
          S.t_jac[t] != S.t_jac[t + 2])
        return false;
    }
    // every partner block is written by exactly one factor (two factors to the same partner would have to be summed)
    std::sort(star_dst.begin(), star_dst.end());
    return std::adjacent_find(star_dst.begin(), star_dst.end()) == star_dst.end();
  };
  for (int v = 0; v < P.n_vars; ++v) {
    if (!S.scheduled[S.front_of_var[v]]) continue;  // another rank's subtree
    const int psize = S.h_rows[v] * P.dims[v];
    const int64_t terms = S.term_ptr[v + 1] - S.term_ptr[v];
    if (is_star(v)) {
      star.push_back({v, psize, terms});
      continue;
    }
    // no later neighbour through any factor (panel = own block + rhs) and many factors: the matrix-core kernel
    if (terms >= 64 && S.h_rows[v] == P.dims[v] + 1 && P.dims[v] <= 15) diag.push_back({v, psize, terms});
    else if (is_tile(v)) tile.push_back({v, psize, terms});
    else if (terms >= 96 && (int64_t)psize * 4 * 8 <= 48 * 1024) heavy.push_back({v, psize, terms});
    else if ((int64_t)psize * 8 <= 48 * 1024) light.push_back({v, psize, terms});
    else huge.push_back({v, psize, terms});
  }
  auto by_psize = [](const VI& a, const VI& b) { return a.psize < b.psize; };
  std::stable_sort(light.begin(), light.end(), by_psize);
  std::stable_sort(heavy.begin(), heavy.end(), by_psize);
  std::vector<int> hv;
  c->hgroups.clear();
  auto emit = [&](std::vector<VI>& L, int threads, int copies, bool global) {
    size_t i = 0;
    while (i < L.size()) {
      // group = run whose largest panel is at most 2x (and at least 1 KB) of its smallest
      size_t j = i;
      const int lo = std::max(L[i].psize, 128);
      while (j < L.size() && L[j].psize <= 2 * lo) ++j;
      const int maxp = L[j - 1].psize;
      c->hgroups.push_back({(int)hv.size(), (int)(j - i), threads, global ? 0 : maxp * copies * 8, global});
      for (size_t k = i; k < j; ++k) hv.push_back(L[k].v);
      i = j;
    }
  };
  std::stable_sort(tile.begin(), tile.end(), by_psize);
  emit(tile, -2, 4, false);   // (four waves a workgroup, a panel each)
  emit(light, 64, 1, false);
  emit(heavy, 256, 4, false);
  emit(huge, 64, 1, true);
  c->n_star_bundles = 0;
  c->h_star_bundles.clear();
  if (!star.empty()) {  // threads == -1 marks the group
    c->hgroups.push_back({(int)hv.size(), (int)star.size(), -1, 0, false});
    for (const VI& x : star) hv.push_back(x.v);
    // bundles for the one-wave-per-bundle kernel: consecutive variables of one shape, <= 5 of them (the own entries of
    // a bundle fit a wave: 5 x (3*3 + 3) lanes), <= 64 factors; a variable too big or of another shape is alone
    auto shape = [&](int v) {
      const int64_t t = S.term_ptr[v];
      return std::array<int, 6>{P.dims[v], S.t_m[t], S.t_colA[t], S.t_colB[t + 1], S.t_dB[t + 1], S.t_colB[t + 2]};
    };
    std::vector<int2>& bundles = c->h_star_bundles;
    size_t i = 0;
    while (i < star.size()) {
      const auto sh = shape(star[i].v);
      const int nown = sh[0] * sh[0] + sh[0];
      int nf = (int)(star[i].terms / 3), nv = 1;
      if (nf > 64 || nown > 64) {  // (the bundle kernel holds a factor per lane)
        bundles.clear();
        break;
      }
      while (i + nv < star.size() && nv < 5 && (nv + 1) * nown <= 64 && shape(star[i + nv].v) == sh &&
             nf + (int)(star[i + nv].terms / 3) <= 64) {
        nf += (int)(star[i + nv].terms / 3);
        ++nv;
      }
      bundles.push_back(int2{(int)i, nv});
      i += nv;
    }
    c->n_star_bundles = (int)bundles.size();
  }
  if (!diag.empty()) {  // threads == 0 marks the group for launch_assemble_h_group
    c->hgroups.push_back({(int)hv.size(), (int)diag.size(), 0, 0, false});
    for (const VI& x : diag) hv.push_back(x.v);
  }
  c->hv_list = hv;
  c->hv_group_of_var.assign(P.n_vars, -1);
  c->hv_pos.assign(P.n_vars, -1);
  for (size_t g = 0; g < c->hgroups.size(); ++g)
    for (int k = c->hgroups[g].begin; k < c->hgroups[g].begin + c->hgroups[g].count; ++k) {
      c->hv_group_of_var[hv[k]] = (int)g;
      c->hv_pos[hv[k]] = k;
    }
}

// Build the launch plan (host) and upload the symbolic tables.
gsx_status upload_symbolic(gsx_context* c) {
  const Symbolic& S = c->S;
  const HostProblem& P = c->P;
  hipStream_t st = c->stream;
  c->marg_release();   // (sized and listed by the tree that is being replaced)
  HIPCHK(c, c->d_fr_off.upload(std::vector<i64>(S.off.begin(), S.off.end()), st));
  HIPCHK(c, c->d_fr_N.upload(S.N, st));
  HIPCHK(c, c->d_fr_F.upload(S.F, st));
  HIPCHK(c, c->d_fr_nfv.upload(S.nfrontal_vars, st));
  HIPCHK(c, c->d_fr_fvar_ptr.upload(S.fvar_ptr, st));
  HIPCHK(c, c->d_fvars.upload(S.fvars, st));
  HIPCHK(c, c->d_fr_parent.upload(S.parent, st));
  {
    std::vector<int> flags(S.n_fronts);  // bit 0: lean leaf, bit 1: blocked (big) layout
    for (int f = 0; f < S.n_fronts; ++f) flags[f] = (S.lean[f] ? 1 : 0) | (S.cls[f] == 2 ? 2 : 0);
    HIPCHK(c, c->d_fr_lean.upload(flags, st));
  }
  if (c->sharded()) {
    // what this rank evaluates, and the masks that complete a vector across the ranks: `own` = this rank's subtree
    // variables (+ the cap's on rank 0): each scalar owned exactly once; `sched` = every variable this rank assembles
    gsx_status fl = upload_factor_lists(c, &S.f_owned);
    if (fl != GSX_OK) return fl;
    std::vector<unsigned char> own_tan(std::max<int64_t>(P.tan_size, 1), 0), sched_tan(own_tan.size(), 0),
        own_state(std::max<int64_t>(P.state_size, 1), 0);
    for (int v = 0; v < P.n_vars; ++v) {
      const int o = S.owner[S.front_of_var[v]];
      const bool own = o < 0 ? c->shard_rank == 0 : o == c->shard_rank;
      const bool sched = o < 0 || o == c->shard_rank;
      for (int d = 0; d < P.dims[v]; ++d) {
        own_tan[P.tan_off[v] + d] = own;
        sched_tan[P.tan_off[v] + d] = sched;
      }
      const int sd = (v + 1 < P.n_vars ? P.state_off[v + 1] : (int)P.state_size) - P.state_off[v];
      for (int d = 0; d < sd; ++d) own_state[P.state_off[v] + d] = own;
    }
    HIPCHK(c, c->d_own_tan.upload(own_tan, st));
    HIPCHK(c, c->d_sched_tan.upload(sched_tan, st));
    HIPCHK(c, c->d_own_state.upload(own_state, st));
    HIPCHK(c, c->d_xscal.alloc(kXScalars));
    HIPCHK(c, hipMemsetAsync(c->d_delta.p, 0, std::max<int64_t>(P.tan_size, 1) * sizeof(double), st));
  }
  HIPCHK(c, c->d_fr_child_ptr.upload(S.child_ptr, st));
  HIPCHK(c, c->d_children.upload(S.children, st));
  HIPCHK(c, c->d_cmap_ptr.upload(std::vector<i64>(S.cmap_ptr.begin(), S.cmap_ptr.end()), st));
  HIPCHK(c, c->d_gidx_ptr.upload(std::vector<i64>(S.gidx_ptr.begin(), S.gidx_ptr.end()), st));
  HIPCHK(c, c->d_cmap.upload(S.cmap, st));
  HIPCHK(c, c->d_gidx.upload(S.gidx, st));
  HIPCHK(c, c->d_h_off.upload(std::vector<i64>(S.h_off.begin(), S.h_off.end()), st));
  HIPCHK(c, c->d_hmap_ptr.upload(std::vector<i64>(S.hmap_ptr.begin(), S.hmap_ptr.end()), st));
  HIPCHK(c, c->d_h_rows.upload(S.h_rows, st));
  HIPCHK(c, c->d_hmap.upload(S.hmap, st));
  HIPCHK(c, c->d_h_loc.upload(S.h_loc, st));
  HIPCHK(c, c->d_term_ptr.upload(std::vector<i64>(S.term_ptr.begin(), S.term_ptr.end()), st));
  {
    std::vector<TermRec> terms(S.t_jac.size());
    for (size_t i = 0; i < terms.size(); ++i)
      terms[i] = TermRec{(i64)S.t_jac[i], S.t_m[i], S.t_colA[i], S.t_colB[i], S.t_dB[i], S.t_dst[i], 0};
    HIPCHK(c, c->d_terms.upload(terms, st));
    std::vector<VarRec> vrec(P.n_vars);
    for (int v = 0; v < P.n_vars; ++v)
      vrec[v] = VarRec{(i64)S.h_off[v], (i64)S.hmap_ptr[v], P.dims[v], S.h_rows[v], S.h_loc[v], P.tan_off[v]};
    std::vector<ChildRec> crec(S.children.size());
    for (size_t i = 0; i < crec.size(); ++i) {
      const int ch = S.children[i];
      crec[i] = ChildRec{(i64)S.off[ch] + (i64)S.F[ch] * S.N[ch] + S.F[ch], (i64)S.cmap_ptr[ch], S.N[ch],
                         S.N[ch] - S.F[ch], 0, 0};
    }
    std::vector<VarRec> fvrec(S.fvars.size());
    for (size_t i = 0; i < fvrec.size(); ++i) fvrec[i] = vrec[S.fvars[i]];
    std::vector<FrontRec> frec(S.n_fronts);
    for (int f = 0; f < S.n_fronts; ++f)
      frec[f] = FrontRec{(i64)S.off[f], S.N[f], S.F[f], S.nfrontal_vars[f], S.fvar_ptr[f], S.child_ptr[f],
                         S.child_ptr[f + 1] - S.child_ptr[f]};
    HIPCHK(c, c->d_var_recs.upload(vrec, st));
    HIPCHK(c, c->d_child_recs.upload(crec, st));
    HIPCHK(c, c->d_front_recs.upload(frec, st));
    HIPCHK(c, c->d_cond_last.upload(std::vector<i64>(S.cond_last.begin(), S.cond_last.end()), st));
    HIPCHK(c, c->d_cond_prev.upload(std::vector<i64>(S.cond_prev.begin(), S.cond_prev.end()), st));
    HIPCHK(c, c->d_cond_front.upload(S.cond_front, st));
    HIPCHK(c, c->d_fvar_recs.upload(fvrec, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  HIPCHK(c, c->d_sched.upload(S.sched, st));
  {
    // leaf-kernel cliques are childless, hence all at level 0, first in its schedule
    const int b = S.n_levels ? S.lvl_ptr[0] : 0, e = S.n_levels ? S.lvl_leaf_end[0] : 0;
    std::vector<LeafRec> lr((size_t)std::max(e - b, 0));
    for (int k = b; k < e; ++k) {
      const int f = S.sched[k];
      const int v0 = S.fvars[S.fvar_ptr[f]];
      lr[k - b] = LeafRec{(i64)S.off[f], (i64)S.h_off[v0], (i64)S.hmap_ptr[v0], (i64)S.gidx_ptr[f],
                          S.N[f], S.F[f], S.nfrontal_vars[f], (int)S.lean[f],
                          P.dims[v0], S.h_rows[v0], S.h_loc[v0], P.tan_off[v0],
                          S.fvar_ptr[f], f, 0, 0};
    }
    c->leaf_base = b;
    c->h_leaf_recs = lr;
    HIPCHK(c, c->d_leaf_recs.upload(lr, st));
    // the back-substitution's copy: a stable partition by lanes per clique (kernels.h: leaf_pack_class), made only when
    // some clique shares its wave
    int max_F = 0, cnt[3] = {0, 0, 0};
    auto cls = [&](const LeafRec& r) { const int g = leaf_pack_class(r.n, r.F, max_F); return g == 16 ? 0 : g == 32 ? 1 : 2; };
    for (const LeafRec& r : lr) max_F = std::max(max_F, r.F);
    if (c->opt.bs_leaf_pack)
      for (const LeafRec& r : lr) ++cnt[cls(r)];
    c->leaf_bs_n[0] = c->leaf_bs_n[1] = c->leaf_bs_n[2] = 0;
    if (cnt[0] + cnt[1] > 0) {
      std::vector<LeafRec> br(lr.size());
      size_t at[3] = {0, (size_t)cnt[0], (size_t)cnt[0] + cnt[1]};
      for (const LeafRec& r : lr) br[at[cls(r)]++] = r;
      for (int q = 0; q < 3; ++q) c->leaf_bs_n[q] = cnt[q];
      HIPCHK(c, c->d_leaf_bs_recs.upload(br, st));
    }
  }
  HIPCHK(c, c->d_H.alloc(std::max<int64_t>(S.h_size, 1)));
  HIPCHK(c, c->d_arena.alloc(std::max<int64_t>(S.arena_size, 1)));
  plan_hessian_groups(c);
  if (c->n_star_bundles) HIPCHK(c, c->d_star_bundles.upload(c->h_star_bundles, st));
  HIPCHK(c, c->d_hvars.upload(c->hv_list, st));
  // ---- factorization launch plan ---------------------------------------------------------------------
  c->small_launch.assign(S.n_levels, {});
  c->big_descs.clear();
  c->big_max_n = c->big_max_nfv = 0;
  c->leaf_launch.assign(S.n_levels, {});
  c->leaf_max_F.assign(S.n_levels, 0);
  std::vector<int> rest_ids;
  for (int l = 0; l < S.n_levels; ++l) {
    int i = S.lvl_ptr[l];
    for (int k = i; k < S.lvl_leaf_end[l]; ++k) c->leaf_max_F[l] = std::max(c->leaf_max_F[l], S.F[S.sched[k]]);
    // leaf-kernel fronts: sorted by (F, N); a launch = same F, panel size within 1.5x — or more, see below
    const int le_all = S.lvl_leaf_end[l];
    if (l == 0) c->leaf_side_group0 = (size_t)-1;
    for (int part = 0; part < 2; ++part) {   // the leaves launched with the level, then (level 0 only) the side leaves
    const int le = (l == 0 && part == 0) ? S.leaf_side_begin : le_all;
    if (l == 0 && part == 1) c->leaf_side_group0 = c->leaf_launch[l].size();
    while (i < le) {
      const int F0 = S.F[S.sched[i]], n0 = std::max(S.N[S.sched[i]], 8);
      int j = i, maxp = 0, maxn = 0;
      // (when every leaf of this width is lean and narrow — the landmarks under blocked camera fronts: panel only, no
      //  Schur complement to form — they go in ONE launch of one-wave workgroups whatever their height: four launches by
      //  panel height took 178 us on BAL-1723, one takes 155.  Otherwise the 1.5x rule and the thread classes: the outer
      //  product of a stored complement wants a thread per row, and the Pose2 leaves got slower in one launch.)
      bool narrow = F0 <= 4;
      for (int k = i; narrow && k < le && S.F[S.sched[k]] == F0; ++k) narrow = S.lean[S.sched[k]] != 0;
      // (few leaves — every level of a pose graph: ONE launch whatever their width and height, with the thread class of
      //  the tallest; the launches by (F, height) were each bound by the latency of one leaf: pose2_100k 11 x 18 us ->
      //  38 us, pose3_100k 4 x 21 -> 30)
      const bool all = !narrow && (le - S.lvl_ptr[l]) <= 16384;
      while (j < le && (all || (S.F[S.sched[j]] == F0 && (narrow || (!narrow && S.N[S.sched[j]] * 2 <= n0 * 3))))) {
        maxp = std::max(maxp, S.N[S.sched[j]] * S.F[S.sched[j]]);
        maxn = std::max(maxn, S.N[S.sched[j]]);
        ++j;
      }
      // (the outer product of a stored complement runs a thread per trailing row: never fewer threads than n - F)
      int rows_below = 0;
      for (int k = i; k < j; ++k) rows_below = std::max(rows_below, S.N[S.sched[k]] - S.F[S.sched[k]]);
      c->leaf_launch[l].push_back({i, j - i, maxn, narrow ? 64 : (maxn <= 72 && rows_below <= 64 ? 64 : (maxn <= 110 ? 128 : 256)), maxp});
      i = j;
    }
    }
    const int se = S.lvl_small_end[l];
    int se_lds = se;   // the medium fronts (n > kSmallMaxN) sit at the end of the level's LDS-class range (sorted by n)
    while (se_lds > i && S.med[S.sched[se_lds - 1]]) --se_lds;
    while (i < se_lds) {
      const int thr = small_threads_for(c, S.N[S.sched[i]]);
      int j = i, maxn = 0;
      // same thread class, and rows within 1.6x of the smallest member (LDS footprint within 2.6x: in effect one group per
      // thread class — measured on the 100 000-pose graphs: 4 launches per level beat 7 finer ones (1.3x) by 3 %)
      const int n0 = std::max(S.N[S.sched[i]], 12);
      while (j < se_lds && small_threads_for(c, S.N[S.sched[j]]) == thr && S.N[S.sched[j]] * 10 <= n0 * 16) {
        maxn = std::max(maxn, S.N[S.sched[j]]);
        ++j;
      }
      c->small_launch[l].push_back({i, j - i, maxn, thr});
      i = j;
    }
    // A launch of few fronts is bound by the latency of ONE front (20-60 us), not by occupancy: merge the
    // size groups of a level when that costs no residency — all 64-thread groups if they total <= 2048
    // fronts (48^2 doubles = 18 KB LDS each: 8 per CU), all wider groups if they total <= 256 fronts.
    {
      std::vector<SmallLaunch>& G = c->small_launch[l];
      std::vector<SmallLaunch> merged;
      size_t k = 0;
      while (k < G.size()) {
        const bool narrow = G[k].threads == 64;
        size_t e = k;
        int total = 0, maxn = 0, thr = 0;
        while (e < G.size() && (G[e].threads == 64) == narrow) {
          total += G[e].count;
          maxn = std::max(maxn, G[e].max_n);
          thr = std::max(thr, G[e].threads);
          ++e;
        }
        if (total <= (narrow ? 2048 : 256)) {
          merged.push_back({G[k].begin, total, maxn, thr});
        } else {
          for (size_t q = k; q < e; ++q) merged.push_back(G[q]);
        }
        k = e;
      }
      G.swap(merged);
      // ... and when the whole level has at most 256 small fronts (one workgroup per CU even at the full LDS size) a
      // single launch: the level then costs the latency of its slowest front once, not once per size group
      int total = 0, maxn = 0;
      for (const SmallLaunch& g : G) {
        total += g.count;
        maxn = std::max(maxn, g.max_n);
      }
      if (G.size() > 1 && total <= 256) {
        const SmallLaunch one{G[0].begin, total, maxn, std::max(256, small_threads_for(c, maxn))};
        G.assign(1, one);
      }
      if (se_lds < se) {   // the level's medium fronts: one group
        SmallLaunch m{se_lds, se - se_lds, 0, 512};
        m.medium = true;
        for (int k = se_lds; k < se; ++k) {
          m.max_n = std::max(m.max_n, S.N[S.sched[k]]);
          m.max_panel = std::max(m.max_panel, S.N[S.sched[k]] * S.F[S.sched[k]]);
        }
        G.push_back(m);
      }
    }
  }
  // ---- the UPPER schedule (Symbolic::ulevel): what the level loop of the full factorization / back-substitution runs —
  //      per upper level the LDS-class fronts that are not tree fronts (whole-front-in-LDS ones, then medium ones: two
  //      launches at most) and the blocked fronts ----
  c->big_level.assign(S.n_ulevels, BigLevel());
  c->rest_launch.assign(S.n_ulevels, {});
  for (int l = 0; l < S.n_ulevels; ++l) {
    const int b0 = S.ulvl_ptr[l], se = S.ulvl_small_end[l];
    for (int pass = 0; pass < 2; ++pass) {
      SmallLaunch r{(int)rest_ids.size(), 0, 0, 0};
      r.medium = pass == 1;
      for (int k = b0; k < se; ++k) {
        const int f = S.usched[k];
        if ((S.med[f] != 0) != r.medium) continue;
        rest_ids.push_back(f);
        r.count++;
        r.max_n = std::max(r.max_n, S.N[f]);
        r.max_F = std::max(r.max_F, S.F[f]);
        r.max_panel = std::max(r.max_panel, S.N[f] * S.F[f]);
      }
      r.threads = r.medium ? 512 : small_threads_for(c, r.max_n);
      if (r.count) c->rest_launch[l].push_back(r);
    }
    BigLevel& B = c->big_level[l];
    B.begin = (int)c->big_descs.size();
    for (int k = se; k < S.ulvl_ptr[l + 1]; ++k) {
      const int f = S.usched[k];
      c->big_descs.push_back(BigDesc{(i64)S.off[f], (i64)S.off[f] + big_panel_offset(S.N[f]), S.N[f], S.F[f], f,
                                     S.parent[f]});
      c->big_max_n = std::max(c->big_max_n, S.N[f]);
      c->big_max_nfv = std::max(c->big_max_nfv, S.nfrontal_vars[f]);
    }
    B.count = (int)c->big_descs.size() - B.begin;
    plan_big_group(c->big_descs.data() + B.begin, B.count, B.plan);
  }
  plan_backsolve(S, c->bs_level_plan, c->bs_plan);
  HIPCHK(c, c->d_usched.upload(S.usched, st));
  HIPCHK(c, c->d_rest_ids.upload(rest_ids, st));
  // ---- hard constraints: the constrained fronts by upper level, their rows and work areas ----
  c->con_level.assign(S.n_ulevels, gsx_context::ConLevel());
  c->con_desc_of_front.assign(S.n_fronts, -1);
  c->CT = ConTables{};
  if (!S.con_fronts.empty()) {
    const int nc = (int)S.con_fronts.size();
    std::vector<int> perm(nc);   // desc position -> index in S.con_fronts
    for (int k = 0; k < nc; ++k) perm[k] = k;
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int a, int b) { return S.ulevel[S.con_fronts[a]] < S.ulevel[S.con_fronts[b]]; });
    std::vector<int> where(nc);
    for (int k = 0; k < nc; ++k) where[perm[k]] = k;
    std::vector<ConDesc> descs(nc);
    std::vector<int> child_list;
    i64 work = 0, iwork = 0;
    for (int k = 0; k < nc; ++k) {
      const int q = perm[k], f = S.con_fronts[q], l = S.ulevel[f];
      ConDesc& d = descs[k];
      d.off = S.off[f];
      d.N = S.N[f];
      d.F = S.F[f];
      d.K = S.con_in[q];
      d.n_fwd = S.con_fwd[q];
      d.work = work;
      work += 3 * (i64)d.K * d.N;
      d.fwd = work;
      work += (i64)d.n_fwd * (d.N - d.F);
      d.iwork = iwork;
      iwork += d.N + 2 * d.K + 1;
      d.own_begin = S.con_own_ptr[q];
      d.own_end = S.con_own_ptr[q + 1];
      d.child_begin = (int)child_list.size();
      for (int e = S.con_child_ptr[q]; e < S.con_child_ptr[q + 1]; ++e) child_list.push_back(where[S.con_child[e]]);
      d.child_end = (int)child_list.size();
      d.front = f;
      d.fwd_map = S.con_fwd_map_ptr[q];
      c->con_desc_of_front[f] = k;
      gsx_context::ConLevel& L = c->con_level[l];
      if (!L.count) L.first = k;
      L.count++;
      L.max_n = std::max(L.max_n, d.N);
    }
    if (child_list.empty()) child_list.push_back(0);
    HIPCHK(c, c->d_con_descs.upload(descs, st));
    HIPCHK(c, c->d_con_own_col_ptr.upload(S.con_own_col_ptr, st));
    HIPCHK(c, c->d_con_own_cols.upload(S.con_own_cols, st));
    HIPCHK(c, c->d_con_own_m.upload(S.con_own_m, st));
    std::vector<i64> oj(S.con_own_jac.begin(), S.con_own_jac.end());
    if (oj.empty()) oj.push_back(0);
    HIPCHK(c, c->d_con_own_jac.upload(oj, st));
    HIPCHK(c, c->d_con_child.upload(child_list, st));
    std::vector<int> fmap = S.con_fwd_map;
    if (fmap.empty()) fmap.push_back(-1);
    HIPCHK(c, c->d_con_fwd_map.upload(fmap, st));
    HIPCHK(c, c->d_con_work.alloc(std::max<i64>(work, 1)));
    HIPCHK(c, c->d_con_iwork.alloc(std::max<i64>(iwork, 1)));
    c->CT = ConTables{c->d_con_descs.p, c->d_con_own_col_ptr.p, c->d_con_own_cols.p, c->d_con_own_m.p, c->d_con_own_jac.p,
                      c->d_con_child.p, c->d_con_fwd_map.p, c->d_con_work.p, c->d_con_iwork.p};
  }
  {
    c->tree_tiers.clear();
    const int nb = (int)S.tree_bounds.size();
    static_assert(kMaxTreeTiers <= kTreeCursors, "a start-list cursor per tier");
    const int ntier = (int)S.tree_start_ptr.size() - 1;   // (symbolic.cpp keeps at most kMaxTreeTiers)
    if (ntier > kTreeCursors) {
      c->err = "more tree tiers than start-list cursors";
      return GSX_E_STATE;
    }
    for (int t = 0; t < ntier; ++t) {
      int maxn = 0;
      size_t lds = 0;   // the medium tier: doubles of LDS of its most demanding front
      for (int f = 0; f < S.n_fronts; ++f)
        if (S.tree_tier[f] == t) {
          maxn = std::max(maxn, S.N[f]);
          lds = std::max(lds, S.med[f] ? (size_t)S.N[f] * S.F[f] + S.N[f] : (size_t)S.N[f] * S.N[f] + S.N[f]);
        }
      c->tree_tiers.push_back({S.tree_start_ptr[t], S.tree_start_ptr[t + 1] - S.tree_start_ptr[t], maxn,
                               t < nb ? (S.tree_threads[t] > 0 ? S.tree_threads[t] : small_threads_for(c, maxn)) : 512,
                               t >= nb ? lds * sizeof(double) : (size_t)0});
    }
    HIPCHK(c, c->d_tree_start.upload(S.tree_start, st));
    HIPCHK(c, c->d_tree_up.upload(S.tree_up, st));
    HIPCHK(c, c->d_tree_npend.upload(S.tree_npend, st));
    HIPCHK(c, c->d_tree_pending.upload(S.tree_npend, st));
    HIPCHK(c, c->d_tree_cursor.upload(std::vector<int>(kTreeCursors, 0), st));
    // top-down: roots = tree fronts whose parent is not a tree front; per front its tree children, the deepest subtree
    // first (a workgroup goes on with that one itself); roots by depth as well: the long chains start first
    std::vector<int> roots, cptr(S.n_fronts + 1, 0), cidx, height(S.n_fronts, 0);
    for (int f = 0; f < S.n_fronts; ++f)   // children have smaller ids
      if (S.tree_tier[f] >= 0 && S.parent[f] >= 0 && S.tree_tier[S.parent[f]] >= 0)
        height[S.parent[f]] = std::max(height[S.parent[f]], height[f] + 1);
    int total = 0;
    for (int f = 0; f < S.n_fronts; ++f) {
      const size_t b = cidx.size();
      for (int k = S.child_ptr[f]; k < S.child_ptr[f + 1]; ++k)
        if (S.tree_tier[f] >= 0 && S.tree_tier[S.children[k]] >= 0) cidx.push_back(S.children[k]);
      std::stable_sort(cidx.begin() + b, cidx.end(), [&](int x, int y) { return height[x] > height[y]; });
      cptr[f + 1] = (int)cidx.size();
      if (S.tree_tier[f] < 0) continue;
      total += (int)(cidx.size() - b) > 1 ? (int)(cidx.size() - b) - 1 : 0;   // published entries
      if (S.parent[f] < 0 || S.tree_tier[S.parent[f]] < 0) roots.push_back(f);
    }
    std::stable_sort(roots.begin(), roots.end(), [&](int x, int y) { return height[x] > height[y]; });
    total += (int)roots.size();   // = tickets
    c->bst_roots = (int)roots.size();
    c->bst_total = total;
    HIPCHK(c, c->d_bst_roots.upload(roots, st));
    HIPCHK(c, c->d_bst_child_ptr.upload(cptr, st));
    HIPCHK(c, c->d_bst_children.upload(cidx, st));
    HIPCHK(c, c->d_bst_counters.upload(std::vector<int>(2, 0), st));
    HIPCHK(c, c->d_bst_ready.upload(std::vector<unsigned long long>((size_t)std::max(total - (int)roots.size(), 1), 0ull), st));
  }
  // front -> where it sits in the launch plan (for the filtered plans of gsx_relinearize_partial)
  c->fr_sched_pos.assign(S.n_fronts, -1);
  c->fr_group.assign(S.n_fronts, -1);
  for (size_t k = 0; k < S.sched.size(); ++k) c->fr_sched_pos[S.sched[k]] = (int)k;
  for (int l = 0; l < S.n_levels; ++l) {
    for (size_t g = 0; g < c->leaf_launch[l].size(); ++g)
      for (int k = c->leaf_launch[l][g].begin; k < c->leaf_launch[l][g].begin + c->leaf_launch[l][g].count; ++k)
        c->fr_group[S.sched[k]] = (int)g;
    for (size_t g = 0; g < c->small_launch[l].size(); ++g)
      for (int k = c->small_launch[l][g].begin; k < c->small_launch[l][g].begin + c->small_launch[l][g].count; ++k)
        c->fr_group[S.sched[k]] = (int)g;
  }
  for (size_t k = 0; k < c->big_descs.size(); ++k) c->fr_group[c->big_descs[k].front] = (int)k;
  {
    auto csr = [&](const std::vector<int>& task_of, const std::vector<int>& lvl_ptr, std::vector<int>& ptr,
                   std::vector<int>& items, std::vector<int>& level_of) {
      ptr.assign(S.n_fronts + 1, 0);
      level_of.assign(task_of.size(), 0);   // (the gather GROUP: an upper level, or n_ulevels = the side group)
      for (int l = 0; l + 1 < (int)lvl_ptr.size(); ++l)
        for (int i = lvl_ptr[l]; i < lvl_ptr[l + 1]; ++i) level_of[i] = l;
      for (int t : task_of) ptr[S.gt_front[t] + 1]++;
      for (int f = 0; f < S.n_fronts; ++f) ptr[f + 1] += ptr[f];
      items.resize(task_of.size());
      std::vector<int> fill(ptr.begin(), ptr.end() - 1);
      for (size_t i = 0; i < task_of.size(); ++i) items[fill[S.gt_front[task_of[i]]]++] = (int)i;
    };
    csr(S.gseg_task, S.gseg_lvl_ptr, c->fr_seg_ptr, c->fr_segs, c->seg_level);
    csr(S.gm_task, S.gm_lvl_ptr, c->fr_gm_ptr, c->fr_gms, c->gm_level);
  }
  HIPCHK(c, c->d_big.upload(c->big_descs, st));
  {
    // gather sources as absolute arena offsets + leading dimension (no dependent metadata loads in the kernel)
    std::vector<GatherSrc> srcs(S.gs_child.size());
    for (size_t i = 0; i < S.gs_child.size(); ++i) {
      const int ch = S.gs_child[i];
      if (S.N[ch] >= (1 << 24)) {
        c->err = "front with more than 2^24 rows";
        return GSX_E_INVALID;
      }
      const bool lean = S.gs_loc2[i] >= 0;
      srcs[i] = GatherSrc{(i64)S.off[ch] + S.gs_loc[i], lean ? S.gs_loc2[i] - S.gs_loc[i] : 0,
                          S.N[ch] | (lean ? S.F[ch] << 24 : 0)};
    }
    std::vector<GatherSeg> segs(S.gseg_task.size());
    for (size_t i = 0; i < segs.size(); ++i) {
      const int t = S.gseg_task[i];
      segs[i] = GatherSeg{(i64)S.gt_dst[t], (i64)S.gseg_begin[i], (int)(S.gseg_end[i] - S.gseg_begin[i]), S.gt_ld[t],
                          S.gt_dims[t], S.gseg_slot[i]};
    }
    HIPCHK(c, c->d_gt_dst.upload(std::vector<i64>(S.gt_dst.begin(), S.gt_dst.end()), st));
    HIPCHK(c, c->d_gt_ld.upload(S.gt_ld, st));
    HIPCHK(c, c->d_gt_dims.upload(S.gt_dims, st));
    HIPCHK(c, c->d_gsrcs.upload(srcs, st));
    c->h_gsegs = segs;
    HIPCHK(c, c->d_gsegs.upload(segs, st));
    HIPCHK(c, c->d_gm_task.upload(S.gm_task, st));
    HIPCHK(c, c->d_gm_slot.upload(S.gm_slot, st));
    HIPCHK(c, c->d_gm_nslots.upload(S.gm_nslots, st));
    HIPCHK(c, c->d_gscratch.alloc((size_t)std::max(S.g_max_slots, 1) * 256));
    HIPCHK(c, hipStreamSynchronize(st));
    c->GA = GatherArgs{c->d_gsegs.p, c->d_gsrcs.p, c->d_gt_dst.p, c->d_gt_ld.p, c->d_gt_dims.p, c->d_gm_task.p,
                       c->d_gm_slot.p, c->d_gm_nslots.p, c->d_gscratch.p};
  }
  // ---- star leaves: lean childless cliques of one star variable, every factor 2 rows at an even [A b] offset, the
  //      clique's rows those of the panel (own rows first) ----
  c->fused_star = false;
  c->leaf_split.clear();
  c->n_star_rest = 0;
  {
    int sgrp = -1;
    for (size_t g = 0; g < c->hgroups.size(); ++g)
      if (c->hgroups[g].threads == -1) sgrp = (int)g;
    if (c->opt.fused_star && sgrp >= 0 && !c->sharded() && !c->constrained() && S.n_levels > 0) {
      auto star_leaf = [&](const LeafRec& r) {
        const int v = S.fvars[S.fvar_ptr[r.front]];
        if (c->hv_group_of_var[v] != sgrp || r.nfv != 1 || !r.lean || r.F != r.dA || r.dA > kStarMaxD || r.loc != 0 ||
            r.n != r.rows)
          return false;
        const int64_t tb = S.term_ptr[v], te = S.term_ptr[v + 1];
        const int64_t nf = (te - tb) / 3;
        if (nf < 1 || nf >= 1024 || r.dA + nf * S.t_dB[tb + 1] + 1 != r.n) return false;
        for (int64_t t = tb; t < te; t += 3)
          if (S.t_m[t] != 2 || (S.t_jac[t] & 1)) return false;
        std::vector<char> seen(r.n, 0);
        for (int k = 0; k < r.n; ++k) {
          const int R = S.hmap[S.hmap_ptr[v] + k];
          if (R < 0 || R >= r.n || seen[R] || (k < r.dA && R != k)) return false;
          seen[R] = 1;
        }
        return true;
      };
      std::vector<char> fused_var(P.n_vars, 0);
      std::vector<StarLeafRec> srec;
      std::vector<int> prow;
      std::vector<LeafRec> rrec;
      for (const SmallLaunch& sl : c->leaf_launch[0]) {
        gsx_context::LeafSplit ls{(int)srec.size(), 0, (int)rrec.size(), 0, 0, 0};
        for (int k = sl.begin; k < sl.begin + sl.count; ++k) {
          const LeafRec& r = c->h_leaf_recs[k - c->leaf_base];
          if (!star_leaf(r)) {
            rrec.push_back(r);
            continue;
          }
          const int v = S.fvars[S.fvar_ptr[r.front]];
          const int64_t tb = S.term_ptr[v];
          const int nf = (int)((S.term_ptr[v + 1] - tb) / 3), dB = S.t_dB[tb + 1];
          fused_var[v] = 1;
          const int64_t stride = nf > 1 ? S.t_jac[tb + 3] - S.t_jac[tb] : 2;
          bool even = stride > 0 && stride <= (1 << 30);
          for (int q = 0; q < nf && even; ++q) even = S.t_jac[tb + 3 * q] == S.t_jac[tb] + q * stride;
          const int* hm = S.hmap.data() + S.hmap_ptr[v];
          const i64 prow_off = (i64)prow.size();
          for (int q = 0; q < nf; ++q)
            for (int i = 0; i < dB; ++i) prow.push_back(hm[S.t_dst[tb + 3 * q + 1] + i]);
          srec.push_back(StarLeafRec{r.off, r.h_off, (i64)tb, (i64)S.t_jac[tb], prow_off, r.n, nf, r.dA, r.toff,
                                     S.t_colA[tb], S.t_colB[tb + 1], S.t_colB[tb + 2], dB, r.front, even ? (int)stride : 0,
                                     hm[r.n - 1], 0});
        }
        ls.scount = (int)srec.size() - ls.sbegin;
        partition_star_leaves(srec.data() + ls.sbegin, ls.scount, c->opt.star_leaf_pack, ls.s16, ls.s32);
        ls.rcount = (int)rrec.size() - ls.rbegin;
        c->leaf_split.push_back(ls);
      }
      if (!srec.empty()) {
        std::vector<int> rest;
        const gsx_context::HGroup& g = c->hgroups[sgrp];
        for (int k = g.begin; k < g.begin + g.count; ++k)
          if (!fused_var[c->hv_list[k]]) rest.push_back(c->hv_list[k]);
        c->fused_star = true;
        c->n_star_rest = (int)rest.size();
        HIPCHK(c, c->d_star_recs.upload(srec, st));
        HIPCHK(c, c->d_star_prow.upload(prow, st));
        if (!rrec.empty()) HIPCHK(c, c->d_leaf_rest_recs.upload(rrec, st));
        if (!rest.empty()) HIPCHK(c, c->d_star_rest_vars.upload(rest, st));
      } else {
        c->leaf_split.clear();
      }
    }
  }
  DevSymbolic& D = c->DS;
  D.n_fronts = S.n_fronts;
  D.fr_off = c->d_fr_off.p; D.fr_N = c->d_fr_N.p; D.fr_F = c->d_fr_F.p; D.fr_nfv = c->d_fr_nfv.p;
  D.fr_fvar_ptr = c->d_fr_fvar_ptr.p; D.fvars = c->d_fvars.p; D.fr_parent = c->d_fr_parent.p;
  D.fr_lean = c->d_fr_lean.p;
  D.fr_child_ptr = c->d_fr_child_ptr.p; D.children = c->d_children.p;
  D.cmap_ptr = c->d_cmap_ptr.p; D.gidx_ptr = c->d_gidx_ptr.p; D.cmap = c->d_cmap.p; D.gidx = c->d_gidx.p;
  D.h_off = c->d_h_off.p; D.hmap_ptr = c->d_hmap_ptr.p; D.h_rows = c->d_h_rows.p; D.hmap = c->d_hmap.p;
  D.h_loc = c->d_h_loc.p;
  D.term_ptr = c->d_term_ptr.p; D.terms = c->d_terms.p;
  D.var_recs = c->d_var_recs.p; D.child_recs = c->d_child_recs.p;
  D.front_recs = c->d_front_recs.p; D.fvar_recs = c->d_fvar_recs.p;
  HIPCHK(c, hipStreamSynchronize(st));
  c->tree_replaced();
  return GSX_OK;
}

}  // namespace gsx
