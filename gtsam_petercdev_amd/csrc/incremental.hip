// incremental.hip — iSAM2's steps on a live handle: the partial ("wildfire") back-substitution, the partial
// relinearization and re-elimination, and gsx_update.
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

using namespace gsx;

extern "C" {

// ISAM2's partial ("wildfire") back-substitution (include/gsx.h; gtsam/nonlinear/ISAM2-impl.cpp:48-77,
// ISAM2Clique.cpp:203-287) on the resident undamped factorization.
gsx_status gsx_backsubstitute_wildfire(gsx_handle h, double threshold, double* delta_out, int64_t n,
                                       int64_t* n_vars_solved, uint64_t* bad_key) {
  if (!h || (delta_out && n != h->P.tan_size)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (h->sharded()) {
    h->err = "the partial back-substitution is not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (!h->linearized || !h->fact_valid || h->fact_lambda != 0.0) {
    h->err = "gsx_backsubstitute_wildfire needs the resident undamped factorization of the current linearization "
             "(gsx_solve with lambda = 0, or gsx_relinearize_partial after one, first)";
    return GSX_E_STATE;
  }
  const Symbolic& S = h->S;
  launch_begin_factorization(h->d_scalars.p, 0.0, h->d_status.p, nullptr, h->stream);  // status reset for the substitution
  h->sc_dirty |= kXFact;
  // (DeltaImpl::UpdateGaussNewtonDelta: threshold <= 0 = all cliques; so is a pass with every clique replaced)
  const bool full = !(threshold > 0.0) || !h->wf_delta_valid || h->wf_all_replaced;
  if (full) {
    dev_backsolve(h);
  } else {
    const size_t nf = (size_t)std::max(S.n_fronts, 1), nv = (size_t)std::max(h->P.n_vars, 1), nt = (size_t)h->P.tan_size;
    HIPCHK(h, h->wf_flags_ready(h->stream));
    if (h->d_wf_dirty.n < nf) HIPCHK(h, h->d_wf_dirty.alloc(nf));
    if (h->d_wf_changed.n < nv) HIPCHK(h, h->d_wf_changed.alloc(nv));
    if (h->d_wf_old.n < nt) HIPCHK(h, h->d_wf_old.alloc(std::max<size_t>(nt, 1)));
    HIPCHK(h, hipMemsetAsync(h->d_wf_changed.p, 0, nv, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_wf_old.p, h->d_delta.p, nt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    const WildfireArgs W{h->d_wf_replaced.p, h->d_wf_dirty.p, h->d_wf_changed.p, h->d_wf_old.p, h->d_status.p, threshold};
    h->DS.wf_dirty = h->d_wf_dirty.p;
    h->DS.wf_replaced = h->d_wf_replaced.p;
    h->DS.wf_changed = h->d_wf_changed.p;
    dev_backsolve(h, &W);
    h->DS.wf_dirty = nullptr;
  }
  st = readback(h);
  if (st != GSX_OK) return st;
  st = indeterminate(h, bad_key, true);
  if (st != GSX_OK) {
    h->delta_outdated();
    return st;
  }
  h->step_solved(true);
  if (n_vars_solved) *n_vars_solved = full ? (int64_t)h->P.n_vars : (int64_t)h->h_status->n_backsub;
  return download(h, h->d_delta.p, delta_out, n);
}

// ---- partial relinearization and re-elimination on a fixed graph ---------------------------------------------------
// The step at the heart of iSAM2's update (gtsam/nonlinear/ISAM2.cpp:419-484 relinearize the marked variables' factors,
// :725-783 re-eliminate the top of the tree that contains them), on a fixed structure: the Bayes tree, its
// factorization and every clean subtree's Schur complement stay resident in HBM; only what the moved variables touch
// is redone — their factors' Jacobians, the H panels of those factors' variables, and the cliques holding them plus all
// ancestors (a re-done clique is re-assembled from H and from ALL its children, whose stored contributions are intact).
namespace {
// The three stages of a partial update (gsx_relinearize_partial, gsx_update), each driven by explicit dirty lists.
// 1. Jacobians of the listed factors (graph order inside each family, as in the full lists)
gsx_status partial_linearize(gsx_handle h, std::vector<int>& dfac) {
  const HostProblem& P = h->P;
  hipStream_t sm = h->stream;
  gsx_context::PartialScratch& ps = h->ps;
  {
    std::sort(dfac.begin(), dfac.end());
    std::vector<int> lists[kNumTypeLists];
    for (int f : dfac) {
      const int k = factor_type_list(P, f);
      if (k >= 0) lists[k].push_back(f);
    }
    sort_absolute_list(P, lists[TL_ABSOLUTE]);
    const int* lp[kNumTypeLists];
    int cnt[kNumTypeLists];
    for (int k = 0; k < kNumTypeLists; ++k) {
      HIPCHK(h, ps.lists[k].stage(lists[k], sm));
      lp[k] = ps.lists[k].p;
      cnt[k] = (int)lists[k].size();
    }
    timer_begin(h, PH_LINEARIZE);
    h->smart_begin(true);
    launch_linearize(h->DP, lp, cnt, h->d_values.p, h->d_jac.p, h->d_status.p, sm, &h->SD);
    timer_end(h, PH_LINEARIZE);
  }
  h->some_blocks_written();
  return GSX_OK;
}
// 2. the H panels of the listed variables, group by group with the groups' own launch shapes
gsx_status partial_assemble(gsx_handle h, std::vector<int>& dvar) {
  hipStream_t sm = h->stream;
  gsx_context::PartialScratch& ps = h->ps;
  dev_ensure_hstar(h);   // (the filtered front_leaf launches of partial_factor read the star leaves' panels)
  {
    std::sort(dvar.begin(), dvar.end(), [&](int a, int b) { return h->hv_pos[a] < h->hv_pos[b]; });
    std::vector<std::pair<int, int>> ranges(h->hgroups.size(), {0, 0});
    for (size_t i = 0; i < dvar.size(); ++i) {
      std::pair<int, int>& r = ranges[h->hv_group_of_var[dvar[i]]];
      if (!r.second) r.first = (int)i;
      r.second++;
    }
    HIPCHK(h, ps.hv.stage(dvar, sm));
    timer_begin(h, PH_ASSEMBLE_H);
    for (size_t g = 0; g < h->hgroups.size(); ++g)
      if (ranges[g].second)
        launch_assemble_h_group(h->DP, h->DS, ps.hv.p + ranges[g].first, ranges[g].second, h->hgroups[g].threads,
                                h->hgroups[g].lds, h->hgroups[g].global, h->d_jac.p, h->d_H.p, sm);
    timer_end(h, PH_ASSEMBLE_H);
    h->panels_reassembled();
  }
  return GSX_OK;
}
// 3. the listed cliques, level by level, in the order and with the launch shapes of the full schedule (a re-done clique is
//    re-assembled from H and from ALL its children, whose Schur complements / L panels are resident in the arena)
gsx_status partial_factor(gsx_handle h, std::vector<int>& dfr) {
  if (!h->wf_all_replaced) {  // these cliques are "replaced" for the next wildfire pass
    HIPCHK(h, h->wf_flags_ready(h->stream));
    HIPCHK(h, h->d_wf_ids.stage(dfr, h->stream));
    launch_mark_fronts(h->d_wf_ids.p, (int)dfr.size(), h->d_wf_replaced.p, h->stream);
  }
  const Symbolic& S = h->S;
  hipStream_t sm = h->stream;
  gsx_context::PartialScratch& ps = h->ps;
  gsx_status st = GSX_OK;
  {
    std::sort(dfr.begin(), dfr.end(), [&](int a, int b) { return h->fr_sched_pos[a] < h->fr_sched_pos[b]; });
    std::vector<LeafRec> leaf;
    std::vector<int> ids;
    std::vector<BigDesc> big;
    std::vector<GatherSeg> segs;
    std::vector<int> gm_task, gm_slot, gm_nslots;
    struct LevelPlan {
      std::vector<std::array<int, 4>> leaf;   // begin, count, max_panel, threads
      std::vector<SmallLaunch> small;         // ranges of `ids`, with the launch shape of the full schedule's group
      int big_begin = 0, big_count = 0;
      std::vector<int> big_fronts;             // the level's dirty blocked fronts
      // ... by UPPER level: a blocked front is factored with the plan (chunk width, kernel shapes) of its launch group in
      // the full schedule — the group is an upper level — so that the same front takes the same rounds and the same
      // kernels whatever else is dirty (found at config-5 size: a plan made for the dirty subset alone picked another
      // chunk width, and the step differed from the full path's in the last bits)
      std::vector<std::array<int, 3>> big_sub; // begin, count, upper level
      // the gather segments of the level's dirty blocked fronts by gather group (launched one group after the other, in
      // the full schedule's order: the side / lean group before the stored children's — same sums, same bits)
      struct GroupPlan {
        int group;
        std::vector<int> seg_idx, gm_idx;
        int seg0 = 0, nseg = 0, m0 = 0, nm = 0;
      };
      std::vector<GroupPlan> groups;
      GroupPlan& group(int g) {
        for (GroupPlan& gp : groups)
          if (gp.group == g) return gp;
        groups.push_back(GroupPlan{g, {}, {}});
        return groups.back();
      }
    };
    std::vector<LevelPlan> plan(S.n_levels);
    int big_max_n = 0, big_max_nfv = 0;
    {
      int last_level = -1, last_cls = -1, last_group = -1;
      for (int f : dfr) {  // schedule order: level, then class, then launch group
        const int l = S.level[f], cls = S.cls[f], g = h->fr_group[f];
        LevelPlan& L = plan[l];
        const bool same = l == last_level && cls == last_cls && (cls == 2 || g == last_group);
        if (cls == 0) {
          const SmallLaunch& sl = h->leaf_launch[l][g];
          if (!same) L.leaf.push_back({(int)leaf.size(), 0, sl.max_panel, sl.threads});
          L.leaf.back()[1]++;
          leaf.push_back(h->h_leaf_recs[h->fr_sched_pos[f] - h->leaf_base]);
        } else if (cls == 1) {
          const SmallLaunch& sl = h->small_launch[l][g];
          if (!same) {
            L.small.push_back(sl);
            L.small.back().begin = (int)ids.size();
            L.small.back().count = 0;
          }
          L.small.back().count++;
          ids.push_back(f);
        } else {
          const BigDesc& d = h->big_descs[g];
          L.big_fronts.push_back(f);
          big_max_n = std::max(big_max_n, d.N);
          big_max_nfv = std::max(big_max_nfv, S.nfrontal_vars[f]);
          // its gather segments (sources: ALL its children, clean or not), at the level the full schedule runs them
          for (int k = h->fr_seg_ptr[f]; k < h->fr_seg_ptr[f + 1]; ++k)
            L.group(h->seg_level[h->fr_segs[k]]).seg_idx.push_back(h->fr_segs[k]);
          for (int k = h->fr_gm_ptr[f]; k < h->fr_gm_ptr[f + 1]; ++k)
            L.group(h->gm_level[h->fr_gms[k]]).gm_idx.push_back(h->fr_gms[k]);
        }
        last_level = l;
        last_cls = cls;
        last_group = g;
      }
    }
    for (int l = 0; l < S.n_levels; ++l) {
      LevelPlan& L = plan[l];
      std::stable_sort(L.big_fronts.begin(), L.big_fronts.end(), [&](int a, int b) { return S.ulevel[a] < S.ulevel[b]; });
      L.big_begin = (int)big.size();
      L.big_count = (int)L.big_fronts.size();
      for (int f : L.big_fronts) {
        const int ul = S.ulevel[f];
        if (L.big_sub.empty() || L.big_sub.back()[2] != ul) L.big_sub.push_back({(int)big.size(), 0, ul});
        L.big_sub.back()[1]++;
        big.push_back(h->big_descs[h->fr_group[f]]);
      }
      // group order: the side group (index n_ulevels) and group 0 hold the lean leaves' sums — first, as in the full
      // schedule; inside a group no particular order is needed (every segment adds into its own destination block or its
      // own scratch slot)
      std::stable_sort(L.groups.begin(), L.groups.end(), [&](const LevelPlan::GroupPlan& a, const LevelPlan::GroupPlan& b) {
        const int ka = a.group == S.n_ulevels ? -1 : a.group, kb = b.group == S.n_ulevels ? -1 : b.group;
        return ka < kb;
      });
      for (LevelPlan::GroupPlan& G : L.groups) {
        G.seg0 = (int)segs.size();
        for (int i : G.seg_idx) segs.push_back(h->h_gsegs[i]);
        G.nseg = (int)G.seg_idx.size();
        G.m0 = (int)gm_task.size();
        for (int i : G.gm_idx) {
          gm_task.push_back(S.gm_task[i]);
          gm_slot.push_back(S.gm_slot[i]);
          gm_nslots.push_back(S.gm_nslots[i]);
        }
        G.nm = (int)G.gm_idx.size();
      }
    }
    HIPCHK(h, ps.leaf.stage(leaf, sm));
    HIPCHK(h, ps.ids.stage(ids, sm));
    HIPCHK(h, ps.big.stage(big, sm));
    HIPCHK(h, ps.segs.stage(segs, sm));
    HIPCHK(h, ps.gm_task.stage(gm_task, sm));
    HIPCHK(h, ps.gm_slot.stage(gm_slot, sm));
    HIPCHK(h, ps.gm_nslots.stage(gm_nslots, sm));
    GatherArgs GA = h->GA;
    GA.segs = ps.segs.p;
    GA.gm_task = ps.gm_task.p;
    GA.gm_slot = ps.gm_slot.p;
    GA.gm_nslots = ps.gm_nslots.p;
    h->sc_dirty |= kXFact;
    timer_begin(h, PH_FACTORIZE);
    launch_begin_factorization(h->d_scalars.p, 0.0, h->d_status.p, nullptr, sm);
    dev_damping(h, 0, 0, 0);
    if (!big.empty())
      launch_big_init(h->DP, h->DS, ps.big.p, (int)big.size(), big_max_n, big_max_nfv, h->d_H.p, h->d_damp.p,
                      h->d_scalars.p, h->d_arena.p, sm);
    for (int l = 0; l < S.n_levels; ++l) {
      const LevelPlan& L = plan[l];
      for (const auto& g : L.leaf)
        launch_front_leaf(h->DP, h->DS, ps.leaf.p + g[0], g[1], g[2], g[3], h->d_H.p, h->d_damp.p, h->d_scalars.p,
                          h->d_arena.p, h->d_status.p, sm);
      for (const SmallLaunch& g : L.small)
        launch_lds_group(h->DP, h->DS, ps.ids.p + g.begin, g, h->d_H.p, h->d_damp.p, h->d_scalars.p, h->d_arena.p,
                         h->d_status.p, sm);
      if (L.big_count) {
        for (const LevelPlan::GroupPlan& G : L.groups)
          if (G.nseg) launch_big_gather(GA, G.seg0, G.nseg, G.m0, G.nm, h->d_arena.p, sm);
        if (h->constrained())   // (the clean children's leftover rows are still in the work area)
          for (int k = L.big_begin; k < L.big_begin + L.big_count; ++k) {
            const int cd = h->con_desc_of_front[big[k].front];
            if (cd >= 0)
              launch_constraint_fronts(h->DS, h->CT, cd, 1, big[k].N, h->d_jac.p, h->d_arena.p, h->d_status.p, sm);
          }
        for (const auto& sg : L.big_sub)
          dev_big_factor(h, ps.big.p + sg[0], sg[1], h->big_level[sg[2]].plan, sm, false);
      }
    }
    // (all cliques: the clean ones' pivots are resident and unchanged, the test is two loads a clique)
    launch_cond_check((int)S.cond_last.size(), h->d_cond_last.p, h->d_cond_prev.p, h->d_cond_front.p, h->d_arena.p,
                      h->d_status.p, sm);
    timer_end(h, PH_FACTORIZE);
  }
  h->delta_outdated();
  st = readback(h);  // (also keeps the temporary tables alive until the launches have run)
  if (st != GSX_OK) return st;
  return indeterminate(h, nullptr, false);
}
}  // namespace

static gsx_status gsx_relinearize_partial_impl(gsx_handle h, const uint64_t* keys, int32_t n_keys, const double* states,
                                   int64_t n_states, gsx_partial_stats* out) {
  if (!h || (n_keys > 0 && !keys) || n_keys < 0) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (h->sharded()) {
    h->err = "partial re-elimination is not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (!h->linearized || !h->h_ready || !h->fact_valid || h->fact_lambda != 0.0) {
    h->err = "gsx_relinearize_partial needs the resident undamped factorization of the current linearization "
             "(gsx_linearize + gsx_solve with lambda = 0 first)";
    return GSX_E_STATE;
  }
  const HostProblem& P = h->P;
  const Symbolic& S = h->S;
  hipStream_t sm = h->stream;
  // marked variables, and their new states
  std::vector<int> marked(n_keys), src_off(n_keys);
  std::vector<char> is_marked(P.n_vars, 0);
  int64_t need = 0;
  for (int k = 0; k < n_keys; ++k) {
    auto it = std::lower_bound(P.keys.begin(), P.keys.end(), keys[k]);
    if (it == P.keys.end() || *it != keys[k]) {
      h->err = "gsx_relinearize_partial: a key is not a variable of the graph";
      return GSX_E_INVALID;
    }
    const int v = (int)(it - P.keys.begin());
    if (is_marked[v]) return GSX_E_INVALID;
    is_marked[v] = 1;
    marked[k] = v;
    src_off[k] = (int)need;
    need += (v + 1 < P.n_vars ? P.state_off[v + 1] : (int)P.state_size) - P.state_off[v];
  }
  if (states && n_states != need) return GSX_E_INVALID;
  gsx_context::PartialScratch& ps = h->ps;
  if (states && n_keys > 0) {
    HIPCHK(h, ps.marked.stage(marked, sm));
    HIPCHK(h, ps.src_off.stage(src_off, sm));
    HIPCHK(h, ps.states.stage(std::vector<double>(states, states + need), sm));
    launch_scatter_states(h->DP, ps.marked.p, ps.src_off.p, n_keys, ps.states.p, h->d_values.p, sm);
    h->states_scattered();
  }
  // what is dirty: factors touching a marked variable; the H panels of all their variables; those variables' cliques and
  // every ancestor.  (Everything below is driven by the dirty lists, not by the size of the graph.)
  std::vector<char> f_dirty(P.n_factors, 0), v_dirty(P.n_vars, 0), fr_dirty(S.n_fronts, 0);
  std::vector<int> dfac, dvar, dfr;
  for (int v : marked)
    for (int k = S.vf_ptr[v]; k < S.vf_ptr[v + 1]; ++k) {
      const int f = S.vf[k];
      if (f_dirty[f]) continue;
      f_dirty[f] = 1;
      dfac.push_back(f);
      for (int q = P.f_key_ptr[f]; q < P.f_key_ptr[f + 1]; ++q) {
        const int u = P.f_vars[q];
        if (!v_dirty[u]) {
          v_dirty[u] = 1;
          dvar.push_back(u);
        }
      }
    }
  for (int v : dvar)
    for (int f = S.front_of_var[v]; f >= 0 && !fr_dirty[f]; f = S.parent[f]) {
      fr_dirty[f] = 1;
      dfr.push_back(f);
    }
  if (dfac.empty()) {
    if (out) *out = gsx_partial_stats{0, 0, 0, S.n_fronts};
    return GSX_OK;
  }
  {
    // When most of the extend-add work of the tree is dirty anyway (the big cliques near the root carry most gather
    // segments), filtering costs more on the host than it saves on the device: take the full path — same bits.
    int64_t dseg = 0;
    for (int f : dfr) dseg += h->fr_seg_ptr[f + 1] - h->fr_seg_ptr[f];
    if ((dseg * 10 > (int64_t)h->h_gsegs.size() * 3 && (int64_t)dfr.size() * 20 > S.n_fronts) ||
        (int64_t)dfr.size() * 100 > (int64_t)S.n_fronts * 15) {
      if (out) *out = gsx_partial_stats{P.n_factors, P.n_vars, S.n_fronts, S.n_fronts};
      dev_linearize(h);
      direct_solve(h, H_ALWAYS, 0, 0, 0, 0.0, false);
      st = readback(h);
      if (st != GSX_OK) return st;
      return indeterminate(h, nullptr, false);
    }
  }
  if (out) *out = gsx_partial_stats{(int)dfac.size(), (int)dvar.size(), (int)dfr.size(), S.n_fronts};
  st = partial_linearize(h, dfac);
  if (st != GSX_OK) return st;
  st = partial_assemble(h, dvar);
  if (st != GSX_OK) return st;
  return partial_factor(h, dfr);
}

// ISAM2::update's structural part on a live handle (include/gsx.h).  The numeric state that survives: the values of the
// kept variables and the [A b] blocks of the kept factors (iSAM2's fixed linearization point).
static gsx_status gsx_update_impl(gsx_handle h, const gsx_problem_desc* desc, const int32_t* factor_origin, const double* new_values,
                      int64_t n_new_values, gsx_update_stats* out) {
  if (!h || !desc || (desc->n_factors > 0 && !factor_origin)) return GSX_E_INVALID;
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  if (h->sharded()) {
    h->err = "gsx_update is not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (!h->has_symbolic || !h->values_set) {
    h->err = "gsx_update needs a handle with values and an ordering (gsx_set_values, gsx_set_ordering first)";
    return GSX_E_STATE;
  }
  hipSetDevice(h->device);
  HostProblem P2;
  st = lower_problem(desc, P2, h->err);
  if (st != GSX_OK) return st;
  const HostProblem& P1 = h->P;
  auto state_len = [](const HostProblem& P, int v) {
    return (v + 1 < P.n_vars ? (int64_t)P.state_off[v + 1] : P.state_size) - P.state_off[v];
  };
  // variables: kept by key
  std::vector<int> old_of(P2.n_vars, -1), new_of(P1.n_vars, -1);
  int64_t need = 0;
  int n_added = 0;
  for (int v = 0; v < P2.n_vars; ++v) {
    auto it = std::lower_bound(P1.keys.begin(), P1.keys.end(), P2.keys[v]);
    if (it != P1.keys.end() && *it == P2.keys[v]) {
      const int o = (int)(it - P1.keys.begin());
      if (P1.types[o] != P2.types[v] || P1.dims[o] != P2.dims[v]) {
        h->err = "gsx_update: a kept variable changed its type or dimension";
        return GSX_E_INVALID;
      }
      old_of[v] = o;
      new_of[o] = v;
    } else {
      need += state_len(P2, v);
      ++n_added;
    }
  }
  if (need != n_new_values || (need > 0 && !new_values)) {
    h->err = "gsx_update: new_values does not hold exactly the states of the new variables";
    return GSX_E_INVALID;
  }
  if (!P2.direction_vars.empty()) {  // the directions of the new Unit3 / EssentialMatrix states: unit, as gsx_set_values asks
    int64_t src = 0;
    for (int v = 0; v < P2.n_vars; ++v) {
      if (old_of[v] >= 0) continue;
      const int t = P2.types[v];
      if (is_direction_type(t) && !direction_state_ok(t, new_values + src)) {
        h->err = "gsx_update: new variable " + std::to_string(v) + " (key " + std::to_string((unsigned long long)P2.keys[v]) +
                 "), a " + direction_type_name(t) + ": its direction is not of unit length";
        return GSX_E_INVALID;
      }
      src += state_len(P2, v);
    }
  }
  // factors: kept by origin (same shape), and which variables the change touches
  std::vector<char> used(P1.n_factors, 0), affected(P2.n_vars, 0);
  int n_fadd = 0;
  for (int f = 0; f < P2.n_factors; ++f) {
    const int o = factor_origin[f];
    if (o < -1 || o >= P1.n_factors || (o >= 0 && used[o])) {
      h->err = "gsx_update: factor_origin is not an injective map into the current factors";
      return GSX_E_INVALID;
    }
    if (o >= 0) {
      bool same = P1.f_rows[o] == P2.f_rows[f] && P1.f_cols[o] == P2.f_cols[f] && P1.f_type[o] == P2.f_type[f] &&
                  P1.f_key_ptr[o + 1] - P1.f_key_ptr[o] == P2.f_key_ptr[f + 1] - P2.f_key_ptr[f];
      for (int q = 0; same && q < P2.f_key_ptr[f + 1] - P2.f_key_ptr[f]; ++q)
        same = old_of[P2.f_vars[P2.f_key_ptr[f] + q]] == P1.f_vars[P1.f_key_ptr[o] + q];
      if (!same) {
        h->err = "gsx_update: a kept factor changed its shape or its variables";
        return GSX_E_INVALID;
      }
      used[o] = 1;
    } else {
      ++n_fadd;
      for (int q = P2.f_key_ptr[f]; q < P2.f_key_ptr[f + 1]; ++q) affected[P2.f_vars[q]] = 1;
    }
  }
  int n_frem = 0, n_vrem = 0;
  for (int o = 0; o < P1.n_factors; ++o)
    if (!used[o]) {
      ++n_frem;
      for (int q = P1.f_key_ptr[o]; q < P1.f_key_ptr[o + 1]; ++q)
        if (new_of[P1.f_vars[q]] >= 0) affected[new_of[P1.f_vars[q]]] = 1;
    }
  for (int o = 0; o < P1.n_vars; ++o) n_vrem += new_of[o] < 0;
  for (int v = 0; v < P2.n_vars; ++v)
    if (old_of[v] < 0) affected[v] = 1;
  // the states: current ones of the kept variables + the given ones of the new variables
  std::vector<double> vals1(std::max<int64_t>(P1.state_size, 1)), vals2(std::max<int64_t>(P2.state_size, 1));
  {
    double tmp = 0;
    st = gsx_get_values(h, P1.state_size > 0 ? vals1.data() : &tmp, P1.state_size);
    if (st != GSX_OK) return st;
    int64_t src = 0;
    for (int v = 0; v < P2.n_vars; ++v) {
      const int64_t len = state_len(P2, v);
      if (old_of[v] >= 0) std::copy_n(vals1.data() + P1.state_off[old_of[v]], len, vals2.data() + P2.state_off[v]);
      else {
        std::copy_n(new_values + src, len, vals2.data() + P2.state_off[v]);
        src += len;
      }
    }
  }
  const bool keep_jac = h->linearized;
  // elimination order: unaffected variables in their current relative order, then the affected ones by static degree
  std::vector<int> ord;
  ord.reserve(P2.n_vars);
  for (int pos = 0; pos < P1.n_vars; ++pos) {
    const int v = new_of[h->S.order[pos]];
    if (v >= 0 && !affected[v]) ord.push_back(v);
  }
  {
    std::vector<int> deg(P2.n_vars, 0), aff;
    for (int f = 0; f < P2.n_factors; ++f) {
      const int nk = P2.f_key_ptr[f + 1] - P2.f_key_ptr[f];
      for (int q = P2.f_key_ptr[f]; q < P2.f_key_ptr[f + 1]; ++q) deg[P2.f_vars[q]] += nk - 1;
    }
    for (int v = 0; v < P2.n_vars; ++v)
      if (affected[v]) aff.push_back(v);
    std::stable_sort(aff.begin(), aff.end(), [&](int a, int b) { return deg[a] < deg[b]; });
    ord.insert(ord.end(), aff.begin(), aff.end());
  }
  // the new tree, on the host, before anything of the handle is touched: a failure up to here leaves the handle as it was
  const double relax = h->S.relax;
  const int relax_max_f = h->S.relax_max_f;
  const auto ta = std::chrono::steady_clock::now();
  Symbolic S2;
  st = symbolic_analysis(P2, ord, relax, relax_max_f, 0, 1, h->opt, S2, h->err);
  if (st != GSX_OK) return st;
  const double t_symbolic = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
  // switch the handle over (handle.h: problem_replaced — a failure from here on leaves every flag down)
  h->problem_replaced();
  HostProblem P_old = std::move(h->P);
  DevBuf<double> jac_old;
  std::swap(jac_old.p, h->d_jac.p);
  std::swap(jac_old.n, h->d_jac.n);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto t0 = std::chrono::steady_clock::now();
  h->P = std::move(P2);
  const HostProblem& P = h->P;
  h->n_smart = (int)std::count(P.f_type.begin(), P.f_type.end(), (int)GSX_F_SMART_PROJECTION);   // (the cache starts empty again)
  st = upload_problem(h);
  if (st != GSX_OK) return st;
  if (std::getenv("GSX_INJECT_UPDATE_FAILURE")) {   // (tests/test_gpu_update.py: a failure in the middle of the switch)
    h->err = "gsx_update: injected failure";
    return GSX_E_NOMEM;
  }
  HIPCHK(h, hipMemcpyAsync(h->d_values.p, vals2.data(), (size_t)P.state_size * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (keep_jac) {
    // kept [A b] blocks, device to device, contiguous runs merged
    int64_t src0 = 0, dst0 = 0, len0 = 0;
    auto flush = [&]() -> hipError_t {
      if (!len0) return hipSuccess;
      const hipError_t e = hipMemcpyAsync(h->d_jac.p + dst0, jac_old.p + src0, (size_t)len0 * sizeof(double),
                                          hipMemcpyDeviceToDevice, h->stream);
      len0 = 0;
      return e;
    };
    for (int f = 0; f < P.n_factors; ++f) {
      const int o = factor_origin[f];
      if (o < 0) continue;
      const int64_t s0 = P_old.f_jac_off[o], d0 = P.f_jac_off[f], len = (int64_t)P.f_rows[f] * P.f_cols[f];
      if (len0 && s0 == src0 + len0 && d0 == dst0 + len0) len0 += len;
      else {
        HIPCHK(h, flush());
        src0 = s0;
        dst0 = d0;
        len0 = len;
      }
    }
    HIPCHK(h, flush());
  }
  const auto t1 = std::chrono::steady_clock::now();
  h->relax = relax;
  h->relax_max_f = relax_max_f;
  h->S = std::move(S2);
  h->order = ord;
  st = upload_symbolic(h);
  if (st != GSX_OK) return st;
  const auto t2 = std::chrono::steady_clock::now();
  h->problem_uploaded();   // (partial_linearize below needs the tables; `linearized` follows at the very end)
  bool relinearized = false;
  if (keep_jac) {
    std::vector<int> dfac;
    for (int f = 0; f < P.n_factors; ++f)
      if (factor_origin[f] < 0) dfac.push_back(f);
    hipMemsetAsync(&h->d_status.p->n_cheirality, 0, sizeof(int), h->stream);
    st = partial_linearize(h, dfac);
    if (st != GSX_OK) {
      h->problem_replaced();
      return st;
    }
    h->sc_dirty |= kXLin;
    relinearized = true;  // every factor has its [A b]: the kept ones at their old linearization point
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) {
    h->problem_replaced();
    h->err = "gsx_update: device failure";
    return GSX_E_NO_DEVICE;
  }
  h->update_finished(relinearized);
  const auto t3 = std::chrono::steady_clock::now();
  if (out) {
    int n_aff = 0;
    for (char a : affected) n_aff += a;
    auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double>(b - a).count();
    };
    *out = gsx_update_stats{n_added, n_vrem, n_fadd, n_frem, n_aff, h->S.n_fronts, t_symbolic + sec(t1, t2), sec(t0, t1) + sec(t2, t3)};
  }
  return GSX_OK;
}

gsx_status gsx_update(gsx_handle h, const gsx_problem_desc* desc, const int32_t* factor_origin, const double* new_values,
                      int64_t n_new_values, gsx_update_stats* out) {
  GSX_GUARD(h, gsx_update_impl(h, desc, factor_origin, new_values, n_new_values, out));
}
gsx_status gsx_relinearize_partial(gsx_handle h, const uint64_t* keys, int32_t n_keys, const double* states,
                                   int64_t n_states, gsx_partial_stats* out) {
  GSX_GUARD(h, gsx_relinearize_partial_impl(h, keys, n_keys, states, n_states, out));
}

}  // extern "C"
