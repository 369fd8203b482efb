// solver.hip — the device pipeline of a handle (level-scheduled multifrontal factorization and back-substitution, PCG
// glue), the solve steps shared by the drivers, and the plain entry points of the C-ABI of include/gsx.h.  Product code: no
// oracle, no CPU fallback — every numeric entry point returns GSX_E_NO_DEVICE when there is no usable GPU.
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

namespace gsx {

// an LDS-class launch group: the whole-front-in-LDS kernel, or the medium-front one
void launch_lds_group(const DevProblem& P, const DevSymbolic& S, const int* ids, const SmallLaunch& g, const double* H,
                      const double* damp, const double* scalars, double* arena, DevStatus* status, hipStream_t st) {
  if (g.medium) launch_front_medium(P, S, ids, g.count, g.max_panel, g.max_n, H, damp, scalars, arena, status, st);
  else launch_front_small(P, S, ids, g.count, g.max_n, g.threads, H, damp, scalars, arena, status, st);
}

static const char* kPhaseNames[PH_COUNT] = {"linearize", "assemble_hessian", "factorize", "backsolve", "linear_error",
                                     "retract", "error", "factor_small", "factor_big", "factor_leaf",
                                     "big_schur", "big_rows", "big_diag", "big_gather", "backsolve_launch",
                                     "all_marginals", "marg_prep", "marg_kt", "marg_sf", "marg_ff", "marg_emit",
                                     "marg_leaf"};

void timer_begin(gsx_context* c, int ph) {
  if (c->profiling < 0) return;  // (an event record costs ~5 us of stream time: gsx_set_profiling(h, -1) switches them off)
  Timer& t = c->timers[ph];
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!t.pool.empty()) {
    ev = t.pool.back();
    t.pool.pop_back();
  } else {
    hipEventCreate(&ev.first);
    hipEventCreate(&ev.second);
  }
  hipEventRecord(ev.first, c->stream);
  t.pending.push_back(ev);
}
void timer_end(gsx_context* c, int ph) {
  if (c->profiling < 0) return;
  hipEventRecord(c->timers[ph].pending.back().second, c->stream);
}
static void timers_resolve(gsx_context* c) {
  hipStreamSynchronize(c->stream);
  for (int ph = 0; ph < PH_COUNT; ++ph) {
    Timer& t = c->timers[ph];
    for (auto& ev : t.pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
        t.ms += ms;
        t.count++;
      }
      t.pool.push_back(ev);
    }
    t.pending.clear();
  }
}

// in-place sum of device memory over the ranks of a sharded problem (gsx_set_shard); a failure is latched and reported
// by the next readback
static void shard_allreduce(gsx_context* c, double* dptr, int64_t n) {
  if (!c->sharded() || n <= 0) return;
  // A rank whose own stream has failed still ENTERS the collective — its peers are in it, and skipping it would leave
  // them blocked until the backend's timeout — with its share poisoned by NaNs, so that every rank sees the failure in
  // the sum (non-finite pivots / solution => GSX_E_INDETERMINATE there, the latched failure here).
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    c->shard_failed = true;
    (void)hipGetLastError();
    (void)hipMemset(dptr, 0xFF, (size_t)n * sizeof(double));   // (all-ones bytes are a NaN)
  }
  if (c->shard_cb(c->shard_user, dptr, n) != 0) c->shard_failed = true;
}

// ---- device pipeline pieces (all asynchronous) -------------------------------------------------------
void dev_linearize(gsx_context* c) {
  timer_begin(c, PH_LINEARIZE);
  hipMemsetAsync(&c->d_status.p->n_cheirality, 0, sizeof(int), c->stream);
  c->smart_begin(true);
  const int* lists[kNumTypeLists];
  for (int k = 0; k < kNumTypeLists; ++k) lists[k] = c->d_type_list[k].p;
  launch_linearize(c->DP, lists, c->type_count, c->d_values.p, c->d_jac.p, c->d_status.p, c->stream, &c->SD);
  timer_end(c, PH_LINEARIZE);
  c->sc_dirty |= kXLin;
  c->blocks_written(true);
}

void dev_assemble_h(gsx_context* c) {
  timer_begin(c, PH_ASSEMBLE_H);
  // the star bundles (landmarks) and the diagonal-panel variables (cameras) share one launch when both exist
  const gsx_context::HGroup *gs = nullptr, *gd = nullptr;
  for (const auto& g : c->hgroups) {
    if (g.threads == -1 && c->n_star_bundles) gs = &g;
    if (g.threads == 0 && g.count > 0) gd = &g;
  }
  // (star leaves: their panels are formed by the factorization itself — front_star_leaf_kernel; dev_ensure_hstar)
  const bool fs = c->fused_star;
  const bool fused = gs && gd && !fs;
  if (fused)
    launch_assemble_h_diag_star(c->DP, c->DS, c->d_hvars.p + gd->begin, gd->count, c->d_hvars.p + gs->begin,
                                c->d_star_bundles.p, c->n_star_bundles, c->d_jac.p, c->d_H.p, c->stream);
  for (const auto& g : c->hgroups) {
    if (fused && (&g == gs || &g == gd)) continue;
    if (fs && g.threads == -1) {
      if (c->n_star_rest)
        launch_assemble_h_group(c->DP, c->DS, c->d_star_rest_vars.p, c->n_star_rest, -1, 0, false, c->d_jac.p, c->d_H.p,
                                c->stream);
      continue;
    }
    if (g.threads == -1 && c->n_star_bundles) {  // the whole star group, a wave per bundle of variables
      launch_assemble_h_star_bundles(c->DP, c->DS, c->d_hvars.p + g.begin, c->d_star_bundles.p, c->n_star_bundles,
                                     c->d_jac.p, c->d_H.p, c->stream);
      continue;
    }
    launch_assemble_h_group(c->DP, c->DS, c->d_hvars.p + g.begin, g.count, g.threads, g.lds, g.global, c->d_jac.p,
                            c->d_H.p, c->stream);
  }
  timer_end(c, PH_ASSEMBLE_H);
  c->h_assembled(!fs);
}

// The complete H panels of the star group, for the readers other than the factorization (diag(H), the gradient, the
// filtered front_leaf launches of gsx_relinearize_partial) after an assembly that left the star leaves' panels out.
void dev_ensure_hstar(gsx_context* c) {
  if (c->hstar_ready) return;
  for (const auto& g : c->hgroups) {
    if (g.threads != -1) continue;
    if (c->n_star_bundles)
      launch_assemble_h_star_bundles(c->DP, c->DS, c->d_hvars.p + g.begin, c->d_star_bundles.p, c->n_star_bundles,
                                     c->d_jac.p, c->d_H.p, c->stream);
    else
      launch_assemble_h_group(c->DP, c->DS, c->d_hvars.p + g.begin, g.count, g.threads, g.lds, g.global, c->d_jac.p,
                              c->d_H.p, c->stream);
  }
  c->hstar_completed();
}

static void dev_hessian_diag(gsx_context* c) {
  if (c->hdiag_ready) return;
  dev_ensure_hstar(c);
  launch_hessian_diag(c->DP, c->DS, c->d_H.p, c->d_hdiag.p, c->stream);
  if (c->con_hd_n)
    launch_constraint_hdiag(c->con_hd_n, c->d_con_hd_tan.p, c->d_con_hd_ptr.p, c->d_con_hd_jidx.p, c->d_con_hd_w.p,
                            c->d_jac.p, c->d_hdiag.p, c->stream);
  if (c->sharded()) {
    // a subtree variable's diagonal lives on its owner, a cap variable's is the sum of every rank's terms
    launch_mask_copy(c->d_hdiag.p, c->d_sched_tan.p, c->P.tan_size, c->d_hdiag.p, c->stream);
    shard_allreduce(c, c->d_hdiag.p, c->P.tan_size);
  }
  c->hdiag_extracted();
}

void dev_damping(gsx_context* c, int diagonal, double mind, double maxd) {
  if (c->damping_is(diagonal, mind, maxd)) return;
  if (diagonal) dev_hessian_diag(c);
  launch_make_damping((int)c->P.tan_size, c->d_hdiag.p, diagonal, mind, maxd, c->d_damp.p, c->stream);
  // (a cap variable is damped once: by rank 0's share of the exchange)
  if (c->sharded()) launch_mask_copy(c->d_damp.p, c->d_own_tan.p, c->P.tan_size, c->d_damp.p, c->stream);
  c->damping_made(diagonal, mind, maxd);
}

// the blocked fronts of one launch group: per round of frontal columns L11 (one workgroup per front), the rows of
// L21 (one per 32 rows), the Schur complement (one per lower tile pair) — bigfront.hip
void dev_big_factor(gsx_context* c, const BigDesc* descs, int count, const BigPlan& plan, hipStream_t st, bool prof) {
  for (int r = 0; r < plan.rounds(); ++r) {
    if (prof) timer_begin(c, PH_K_POTRF0);  // (one HIP-event pair per kernel launch)
    launch_big_diag(descs, count, plan, r, c->d_arena.p, c->d_status.p, st);
    if (prof) timer_end(c, PH_K_POTRF0);
    if (prof) timer_begin(c, PH_K_TRSM);
    launch_big_rows(descs, count, plan, r, c->d_arena.p, c->d_status.p, st);
    if (prof) timer_end(c, PH_K_TRSM);
    if (prof) timer_begin(c, PH_K_SYRK);
    launch_big_schur(descs, count, plan, r, c->d_arena.p, st);
    if (prof) timer_end(c, PH_K_SYRK);
  }
}

// GSX_DEBUG_LAUNCH=1: synchronise after the launches of the dependency-driven kernels and say what came back
static void debug_sync(gsx_context* c, const char* what, int a, int b) {
  static const bool on = std::getenv("GSX_DEBUG_LAUNCH") != nullptr;
  if (!on) return;
  fprintf(stderr, "[gsx] %s (%d, %d) ...", what, a, b);
  fflush(stderr);
  const hipError_t e = hipStreamSynchronize(c->stream);
  const hipError_t e2 = hipGetLastError();
  fprintf(stderr, " %s / %s\n", hipGetErrorString(e), hipGetErrorString(e2));
  fflush(stderr);
}

// one launch group of the leaf-kernel cliques: its star leaves fused (front_star_leaf_kernel), the others by front_leaf
static void dev_leaf_group(gsx_context* c, size_t g, hipStream_t st) {
  const SmallLaunch& sl = c->leaf_launch[0][g];
  if (c->fused_star && c->leaf_split[g].scount) {
    const gsx_context::LeafSplit& ls = c->leaf_split[g];
    launch_front_star_leaf(c->DS, c->d_star_recs.p + ls.sbegin, ls.s16, ls.s32, ls.scount - ls.s16 - ls.s32,
                           c->d_star_prow.p, c->d_jac.p, c->d_damp.p, c->d_scalars.p, c->d_H.p, c->d_arena.p,
                           c->d_status.p, st);
    if (ls.rcount)
      launch_front_leaf(c->DP, c->DS, c->d_leaf_rest_recs.p + ls.rbegin, ls.rcount, sl.max_panel, sl.threads, c->d_H.p,
                        c->d_damp.p, c->d_scalars.p, c->d_arena.p, c->d_status.p, st);
    return;
  }
  launch_front_leaf(c->DP, c->DS, c->d_leaf_recs.p + (sl.begin - c->leaf_base), sl.count, sl.max_panel, sl.threads, c->d_H.p,
                    c->d_damp.p, c->d_scalars.p, c->d_arena.p, c->d_status.p, st);
}

// the low-priority queue of the side work (created on first use)
static bool bulk_ready(gsx_context* c) {
  if (c->bulk) return true;
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return false;
  if (hipStreamCreateWithPriority(&c->bulk, hipStreamNonBlocking, least) != hipSuccess) {
    c->bulk = nullptr;
    return false;
  }
  if (hipEventCreateWithFlags(&c->bulk_go, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->bulk_done, hipEventDisableTiming) != hipSuccess)
    return false;
  return true;
}

static void dev_factorize(gsx_context* c, double lambda) {
  const Symbolic& S = c->S;
  c->factorization_queued(lambda);
  c->sc_dirty |= kXFact;
  timer_begin(c, PH_FACTORIZE);
  launch_begin_factorization(c->d_scalars.p, lambda, c->d_status.p, c->d_tree_cursor.p, c->stream);
  if (!c->big_descs.empty())
    launch_big_init(c->DP, c->DS, c->d_big.p, (int)c->big_descs.size(), c->big_max_n, c->big_max_nfv, c->d_H.p,
                    c->d_damp.p, c->d_scalars.p, c->d_arena.p, c->stream);
  // ---- the leaf-kernel cliques (all childless: one group of launches) ----
  // The SIDE work (Symbolic::side_*): the lean leaves whose parents sit above the first blocked level, and their
  // product-form gather, on the low-priority queue — beside the latency-bound blocked chain of the lower levels
  // instead of in front of it.  (With per-launch timers everything stays on the one timed queue.)
  const int sg = S.n_ulevels;   // the side gather group
  const bool have_side = S.side_level0 >= 0;
  const bool use_bulk = have_side && c->profiling <= 0 && bulk_ready(c);
  if (S.n_levels > 0) {
    const std::vector<SmallLaunch>& LL = c->leaf_launch[0];
    const size_t n_main_leaf = c->leaf_side_group0 != (size_t)-1 ? c->leaf_side_group0 : LL.size();
    if (use_bulk) {
      // (Forked right behind the zeroing / H terms of the blocked fronts.  Measured on BAL-1723, ms per LM iteration: no
      //  second queue 1.924; forked here 1.880; forked behind the main queue's own leaves and gather 1.904 — the side work then
      //  runs beside the first blocked level only, whose 11-workgroup big_rows launch goes from 63 to 153 us under it.  The
      //  low stream priority does not keep the side kernels off the CUs: what is gained is the blocked chain starting
      //  earlier, what is lost is every kernel running beside them running slower.)
      hipEventRecord(c->bulk_go, c->stream);
      hipStreamWaitEvent(c->bulk, c->bulk_go, 0);
      for (size_t g = n_main_leaf; g < LL.size(); ++g) dev_leaf_group(c, g, c->bulk);
      launch_big_gather(c->GA, S.gseg_lvl_ptr[sg], S.gseg_lvl_ptr[sg + 1] - S.gseg_lvl_ptr[sg], S.gm_lvl_ptr[sg],
                        S.gm_lvl_ptr[sg + 1] - S.gm_lvl_ptr[sg], c->d_arena.p, c->bulk);
      hipEventRecord(c->bulk_done, c->bulk);
      c->bulk_pending = true;
    }
    for (size_t g = 0; g < (use_bulk ? n_main_leaf : LL.size()); ++g) {
      if (c->profiling > 0) timer_begin(c, PH_FACTOR_LEAF);
      dev_leaf_group(c, g, c->stream);
      if (c->profiling > 0) timer_end(c, PH_FACTOR_LEAF);
    }
  }
  // ---- the tree fronts of every level: one launch per tier (their leaf-kernel children were the launches above) ----
  for (size_t t = 0; t < c->tree_tiers.size(); ++t) {
    const gsx_context::TreeTier& tt = c->tree_tiers[t];
    if (!tt.nstart) continue;
    if (c->profiling > 0) timer_begin(c, PH_FACTOR_SMALL);
    const TreeArgs ta{c->d_tree_start.p + tt.start0, tt.nstart, c->d_tree_cursor.p + t, c->d_tree_pending.p,
                      c->d_tree_up.p, c->d_tree_npend.p};
    if (tt.med_lds)
      launch_front_tree_med(c->DP, c->DS, ta, tt.med_lds, c->d_H.p, c->d_damp.p, c->d_scalars.p, c->d_arena.p,
                            c->d_status.p, c->stream);
    else
      launch_front_tree(c->DP, c->DS, ta, tt.max_n, tt.threads, c->d_H.p, c->d_damp.p, c->d_scalars.p, c->d_arena.p,
                        c->d_status.p, c->stream);
    debug_sync(c, tt.med_lds ? "front_tree_med" : "front_tree", tt.nstart, (int)tt.med_lds);
    if (c->profiling > 0) timer_end(c, PH_FACTOR_SMALL);
  }
  // ---- the upper levels (Symbolic::ulevel): everything below them is complete ----
  for (int l = 0; l < S.n_ulevels; ++l) {
    for (const SmallLaunch& sl : c->rest_launch[l]) {
      if (c->profiling > 0) timer_begin(c, PH_FACTOR_SMALL);
      launch_lds_group(c->DP, c->DS, c->d_rest_ids.p + sl.begin, sl, c->d_H.p, c->d_damp.p, c->d_scalars.p, c->d_arena.p,
                       c->d_status.p, c->stream);
      debug_sync(c, sl.medium ? "front_medium (level)" : "front_small (level)", sl.count, sl.medium ? sl.max_panel : sl.max_n);
      if (c->profiling > 0) timer_end(c, PH_FACTOR_SMALL);
    }
    // the fronts above the first blocked level take the side leaves' contributions: those must have landed (and they
    // come first in every destination block's sum, as in the one-queue order)
    if (have_side && l == S.side_level0 + 1 && c->bulk_pending) {
      hipStreamWaitEvent(c->stream, c->bulk_done, 0);
      c->bulk_pending = false;
    }
    const BigLevel& B = c->big_level[l];
    const bool prof = c->profiling > 0;
    if (prof && B.count) timer_begin(c, PH_FACTOR_BIG);
    // deterministic extend-add into this level's blocked fronts: the children are complete.  (Group 0 also holds the
    // product-form contributions of the lean leaves — of all levels, or of the levels up to the first blocked one when
    // the others are side work.)
    if (S.gseg_lvl_ptr[l + 1] > S.gseg_lvl_ptr[l]) {
      if (prof) timer_begin(c, PH_K_GATHER);
      launch_big_gather(c->GA, S.gseg_lvl_ptr[l], S.gseg_lvl_ptr[l + 1] - S.gseg_lvl_ptr[l], S.gm_lvl_ptr[l],
                        S.gm_lvl_ptr[l + 1] - S.gm_lvl_ptr[l], c->d_arena.p, c->stream);
      if (prof) timer_end(c, PH_K_GATHER);
    }
    if (l == 0 && have_side && !use_bulk && S.gseg_lvl_ptr[sg + 1] > S.gseg_lvl_ptr[sg]) {   // (no second queue: in line)
      if (prof) timer_begin(c, PH_K_GATHER);
      launch_big_gather(c->GA, S.gseg_lvl_ptr[sg], S.gseg_lvl_ptr[sg + 1] - S.gseg_lvl_ptr[sg], S.gm_lvl_ptr[sg],
                        S.gm_lvl_ptr[sg + 1] - S.gm_lvl_ptr[sg], c->d_arena.p, c->stream);
      if (prof) timer_end(c, PH_K_GATHER);
    }
    if (B.count) {
      // sharded: every rank's share of the cap (H terms, damping, its subtrees' Schur complements) is in; their sum
      // is the assembled cap, which all ranks now factor alike
      if (l == S.cap_ulevel0) shard_allreduce(c, c->d_arena.p + S.cap_begin, S.cap_end - S.cap_begin);
      // hard constraints: the assembled fronts that hold constraint rows become unconstrained fronts with the same
      // conditionals and Schur complement (constraint.hip)
      if (c->con_level[l].count)
        launch_constraint_fronts(c->DS, c->CT, c->con_level[l].first, c->con_level[l].count, c->con_level[l].max_n,
                                 c->d_jac.p, c->d_arena.p, c->d_status.p, c->stream);
      dev_big_factor(c, c->d_big.p + B.begin, B.count, B.plan, c->stream, prof);
      if (prof) timer_end(c, PH_FACTOR_BIG);
    }
  }
  // choleskyPartial's conditioning test, per clique of the reference tree (cholesky.cpp:145-158)
  launch_cond_check((int)S.cond_last.size(), c->d_cond_last.p, c->d_cond_prev.p, c->d_cond_front.p, c->d_arena.p,
                    c->d_status.p, c->stream);
  timer_end(c, PH_FACTORIZE);
}

// All leaf-kernel cliques of a level in one launch: from the partitioned copy where narrow cliques share a wave
// (handle.h: d_leaf_bs_recs — the leaf cliques are childless, all of level 0), else a wave each in schedule order.
static void backsolve_leaves(gsx_context* c, int l) {
  const Symbolic& S = c->S;
  const int n = S.lvl_leaf_end[l] - S.lvl_ptr[l];
  if (l == 0 && c->leaf_bs_n[0] + c->leaf_bs_n[1] > 0)
    launch_backsolve_leaf(c->DS, c->d_leaf_bs_recs.p, c->leaf_bs_n[0], c->leaf_bs_n[1], c->leaf_bs_n[2], c->leaf_max_F[0],
                          c->d_arena.p, c->d_delta.p, c->d_status.p, c->stream);
  else
    launch_backsolve_leaf(c->DS, c->d_leaf_recs.p + (S.lvl_ptr[l] - c->leaf_base), 0, 0, n, c->leaf_max_F[l], c->d_arena.p,
                          c->d_delta.p, c->d_status.p, c->stream);
}

// One launch of a back-substitution plan (handle.h: BsLaunch; upload.hip: plan_backsolve); sched: the device copy of the
// schedule the plan is over.
static void run_bs_launch(gsx_context* c, const int* sched, const BsLaunch& b) {
  static const char* const names[] = {"backsolve_big", "backsolve_small", "backsolve", "backsolve_leaf", "backsolve_tree"};
  const bool timed = c->profiling > 0 && b.kind != BS_LEAF;   // (the leaf cliques' launch never had a timer of its own)
  if (timed) timer_begin(c, PH_K_BACKSOLVE);
  switch (b.kind) {
    case BS_BIG:
      launch_backsolve_big(c->DS, sched + b.begin, b.count, b.max_n, b.max_F, c->d_arena.p, c->d_delta.p, c->d_status.p,
                           c->stream);
      break;
    case BS_SMALL:
      launch_backsolve_small(c->DS, sched + b.begin, b.count, b.max_F, c->d_arena.p, c->d_delta.p, c->d_status.p, c->stream);
      break;
    case BS_GENERIC:
      launch_backsolve(c->DS, sched + b.begin, b.count, b.threads, b.max_n, c->d_arena.p, c->d_delta.p, c->d_status.p,
                       c->stream);
      break;
    case BS_LEAF:
      backsolve_leaves(c, b.level);
      break;
    case BS_TREE:
      launch_backsolve_tree(c->DS,
                            BacksolveTreeArgs{c->d_bst_roots.p, c->bst_roots, c->bst_total, c->d_bst_child_ptr.p,
                                              c->d_bst_children.p, c->d_bst_ready.p, c->d_bst_counters.p,
                                              c->d_bst_counters.p + 1, c->bst_epoch},
                            c->d_arena.p, c->d_delta.p, c->d_status.p, c->stream);
      break;
  }
  if (timed) timer_end(c, PH_K_BACKSOLVE);
  debug_sync(c, names[b.kind], b.count, b.kind == BS_GENERIC ? b.threads : b.max_n);
}

// The level-by-level back-substitution over ALL fronts.  wf: ISAM2's partial back-substitution — the kernels skip the
// cliques no change reaches (DS.wf_*), and a bookkeeping pass follows every level (nullptr: all cliques).
static void dev_backsolve_levels(gsx_context* c, const WildfireArgs* wf) {
  const Symbolic& S = c->S;
  timer_begin(c, PH_BACKSOLVE);
  c->delta_overwritten();  // (the callers that leave a complete undamped solution behind say so: step_solved)
  const std::vector<BsLaunch>& plan = c->bs_level_plan;
  size_t i = 0;
  for (int l = S.n_levels - 1; l >= 0; --l) {
    for (; i < plan.size() && plan[i].level == l; ++i) run_bs_launch(c, c->d_sched.p, plan[i]);
    if (wf) {  // the leaf cliques (F <= 16) a thread each, the others a wave each
      const int b = S.lvl_ptr[l], le = S.lvl_leaf_end[l];
      launch_wildfire_post(c->DS, c->d_sched.p + b, le - b, false, *wf, c->d_delta.p, c->stream);
      launch_wildfire_post(c->DS, c->d_sched.p + le, S.lvl_ptr[l + 1] - le, true, *wf, c->d_delta.p, c->stream);
    }
  }
  timer_end(c, PH_BACKSOLVE);
}

// OptimizeClique top-down (gtsam/linear/linearAlgorithms-inst.h:49-117): the upper fronts level by level (Symbolic::ulevel),
// then the tree fronts of all levels in one launch, then the leaf-kernel cliques.
void dev_backsolve(gsx_context* c, const WildfireArgs* wf) {
  if (wf != nullptr || !c->opt.bs_tree) {
    dev_backsolve_levels(c, wf);
    return;
  }
  timer_begin(c, PH_BACKSOLVE);
  c->delta_overwritten();  // (the callers that leave a complete undamped solution behind say so: step_solved)
  for (const BsLaunch& b : c->bs_plan) {
    if (b.kind == BS_TREE) {   // its ticket counters start at zero, and its epoch tells this launch's entries from stale ones
      hipMemsetAsync(c->d_bst_counters.p, 0, 2 * sizeof(int), c->stream);
      if (++c->bst_epoch == 0) c->bst_epoch = 1;
    }
    run_bs_launch(c, c->d_usched.p, b);
  }
  timer_end(c, PH_BACKSOLVE);
}

// solved_step: d_delta is the solution of the damped system just factored (the LM trial) — the two linearized errors then
// come from the right-hand sides and the step (kernels.hip: lin0_kernel / model_error_kernel), no pass over [A b];
// otherwise (an arbitrary point: Dogleg, gsx_linear_error) the direct evaluation
void dev_linear_error(gsx_context* c, bool solved_step) {
  // (hard constraints: the step solves the KKT system, not (H + lambda D) delta = g — the identity below does not hold)
  const bool direct_only = !c->opt.linerr_from_step || c->constrained() || c->use_pcg();  // (PCG: the step is not exact either)
  timer_begin(c, PH_LINERR);
  if (solved_step && !direct_only && c->h_ready) {
    if (!c->lin0_ready) {
      launch_lin0(c->DP, c->d_jac.p, c->d_partials.p, gsx_context::kPartials, c->d_scalars.p, c->stream);
      c->lin0_computed();
    }
    launch_model_error(c->DP, c->DS, c->d_hvars.p, (int)c->hv_list.size(), c->d_H.p, c->d_delta.p, c->d_damp.p,
                       c->d_partials.p, gsx_context::kPartials, c->d_scalars.p, c->stream);
  } else {
    launch_linear_error(c->DP, c->d_jac.p, c->d_delta.p, c->d_partials.p, gsx_context::kPartials, c->d_scalars.p,
                        c->lin_err_slice, c->stream);
  }
  c->sc_dirty |= (1u << SC_LIN0) | (1u << SC_LIND);
  timer_end(c, PH_LINERR);
}
void dev_retract(gsx_context* c, const double* d_delta) {
  timer_begin(c, PH_RETRACT);
  launch_retract(c->DP, c->d_values.p, d_delta, c->d_trial.p, c->stream);
  timer_end(c, PH_RETRACT);
}
void dev_error(gsx_context* c, const double* d_vals, int slot) {
  timer_begin(c, PH_ERROR);
  const int* lists[kNumTypeLists];
  for (int k = 0; k < kNumTypeLists; ++k) lists[k] = c->d_type_list[k].p;
  c->smart_begin(false);
  launch_error(c->DP, lists, c->type_count, d_vals, c->d_partials.p, gsx_context::kPartials, c->d_scalars.p, slot, c->stream,
               &c->SD);
  c->sc_dirty |= 1u << slot;
  timer_end(c, PH_ERROR);
}
gsx_status readback(gsx_context* c) {
  if (c->sharded() && c->sc_dirty) {
    // partial sums and status counters of this rank's share -> the whole problem's, identical on every rank
    launch_shard_pack(c->d_scalars.p, c->d_status.p, c->sc_dirty, c->d_xscal.p, c->stream);
    shard_allreduce(c, c->d_xscal.p, kXScalars);
    launch_shard_unpack(c->d_xscal.p, c->sc_dirty, c->d_scalars.p, c->d_status.p, c->stream);
  }
  c->sc_dirty = 0;
  if (c->shard_failed) {
    c->shard_failed = false;
    c->err = "the all-reduce callback of a sharded handle failed";
    return GSX_E_NO_DEVICE;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_scalars, c->d_scalars.p, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_status, c->d_status.p, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  c->n_cheirality = c->h_status->n_cheirality;
  c->factorization_judged(c->h_status->n_fail > 0 || c->h_status->n_nonfinite > 0);
  return GSX_OK;
}

bool factorization_ok(const gsx_context* c) { return c->h_status->n_fail == 0 && c->h_status->n_nonfinite == 0; }
}  // namespace gsx
// (for tests/test_gpu_star_leaf_packed.py; not part of the C ABI of include/gsx.h.)  The fronts that reported a failed
// pivot in the factorization last read back (DevStatus::n_fail), -1 without a device.
extern "C" int gsxtest_last_fail_count(gsx_context* c) { return c && c->has_device && c->h_status ? c->h_status->n_fail : -1; }
namespace gsx {

static uint64_t failing_key(gsx_context* c) {
  const DevStatus& s = *c->h_status;
  if (s.n_fail > 0 && s.first_front >= 0 && s.first_front < c->S.n_fronts)
    return c->P.keys[c->S.fvars[c->S.fvar_ptr[s.first_front]]];
  return c->P.n_vars ? c->P.keys[c->S.order.empty() ? 0 : c->S.order[0]] : 0;
}

gsx_status need_device(gsx_context* c) {
  if (!c->has_device) {
    c->err = "no usable gfx950 device (the hot path has no CPU fallback)";
    return GSX_E_NO_DEVICE;
  }
  return GSX_OK;
}

static gsx_status ensure_ready(gsx_context* c, bool need_values, bool need_symbolic) {
  gsx_status st = need_device(c);
  if (st != GSX_OK) return st;
  if (need_values && !c->values_set && c->P.state_size > 0) {
    c->err = "values not set";
    return GSX_E_STATE;
  }
  if (need_symbolic && !c->has_symbolic) {
    c->err = "ordering not set";
    return GSX_E_STATE;
  }
  return GSX_OK;
}
// what a numeric entry point starts with, behind its argument checks: the handle can serve the call, its device is current
gsx_status begin_call(gsx_context* c, bool need_values, bool need_symbolic) {
  gsx_status st = ensure_ready(c, need_values, need_symbolic);
  if (st != GSX_OK) return st;
  hipSetDevice(c->device);
  return GSX_OK;
}

// The verdict on the status counters the last readback brought: GSX_E_INDETERMINATE when a front failed (also_nonfinite:
// or a pivot / the solution is not finite — the sites that go on to use the step ask for that, the ones that only keep
// the factorization resident, do not, as before), else GSX_OK.  `solved` is the caller's: the sites that had a step of
// their own say delta_outdated(); where a linearize or re-elimination came first it is down already; the marginals'
// re-factorization leaves it alone when it fails, as before.
gsx_status indeterminate(gsx_context* c, uint64_t* bad_key, bool also_nonfinite) {
  if (!(c->h_status->n_fail > 0 || (also_nonfinite && c->h_status->n_nonfinite > 0))) return GSX_OK;
  if (bad_key) *bad_key = failing_key(c);
  c->factorization_failed();
  c->err = "indeterminate linear system";
  return GSX_E_INDETERMINATE;
}

// n doubles of device memory to the caller (out may be null: nothing asked for)
gsx_status download(gsx_context* c, const double* src, double* out, int64_t n) {
  if (!out || n <= 0) return GSX_OK;
  HIPCHK(c, hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GSX_OK;
}

// ---- the iterative linear solver (pcg.hip) -------------------------------------------------------------------------
static const char* pcg_params_error(const gsx_pcg_params& p) {
  if (p.max_iterations < 0 || p.min_iterations < 0) return "PCG: negative iteration bound";
  if (p.reset < 1) return "PCG: reset must be at least 1 (the reference takes k % reset)";
  if (!(p.epsilon_rel >= 0.0) || !(p.epsilon_abs >= 0.0)) return "PCG: a negative or NaN epsilon";
  if (p.preconditioner != GSX_PRECOND_DUMMY && p.preconditioner != GSX_PRECOND_BLOCK_JACOBI)
    return "PCG: unknown preconditioner (the subgraph preconditioner is not offered)";
  return nullptr;
}
// what keeps a handle from solving by PCG at all
static gsx_status pcg_refusal(gsx_context* c) {
  if (c->sharded()) {
    c->err = "the PCG solver is not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (!c->P.con_factor.empty()) {
    c->err = "the PCG solver is not available on a problem with hard constraints (the step there is a KKT solve)";
    return GSX_E_STATE;
  }
  return GSX_OK;
}
// (J'J + lambda D) delta = J'b by PCG into d_delta, D from the handle's damping vector (dev_damping first).  Synchronises.
// GSX_E_INDETERMINATE leaves the handle usable (solved = false).
static gsx_status pcg_solve(gsx_context* c, double lambda, const gsx_pcg_params& prm, gsx_pcg_stats* stats, uint64_t* bad_key) {
  gsx_status rs = pcg_refusal(c);   // (also here: gsx_update may have brought constraint rows in since the solver was chosen)
  if (rs != GSX_OK) return rs;
  if (pcg_max_dim(c->P) > kPcgMaxDim) {   // (pcg.hip: the per-wave LDS arrays and lane maps of both preconditioners' kernels)
    c->err = "PCG takes variables of tangent dimension up to 32";
    return GSX_E_INVALID;
  }
  if (!c->pcg) HIPCHK(c, pcg_work_create(c->P, c->stream, &c->pcg));
  PcgScalars sc{};
  HIPCHK(c, pcg_run(c->pcg, c->d_jac.p, c->d_damp.p, lambda, prm, c->d_delta.p, c->d_status.p, c->stream, &sc));
  c->delta_overwritten();   // d_delta no longer holds the direct solution a wildfire pass starts from
  c->pcg_iterations += sc.k;
  c->pcg_run_iterations += sc.k;
  c->pcg_solves++;
  if (stats) {
    stats->iterations = sc.k;
    stats->converged = sc.gamma <= sc.threshold ? 1 : 0;
    stats->gamma_initial = sc.gamma0;
    stats->gamma_final = sc.gamma;
    stats->threshold = sc.threshold;
  }
  if (sc.fail) {
    c->delta_outdated();   // (the resident factorization, if any, is not PCG's: it stays)
    if (sc.fail == 2) {
      if (bad_key && sc.bad_var >= 0 && sc.bad_var < c->P.n_vars) *bad_key = c->P.keys[sc.bad_var];
      c->err = "indeterminate linear system: a diagonal block of the damped Hessian has no Cholesky factor";
    } else {
      c->err = "indeterminate linear system: p'Ap is not positive in the conjugate-gradient iteration";
    }
    return GSX_E_INDETERMINATE;
  }
  c->step_solved(false);
  return GSX_OK;
}

// ---- the solve steps of the drivers and entry points -------------------------------------------------------------------
// the direct solve: ensure H, damping, factorize, optionally back-substitute (all asynchronous: the caller reads back)
void direct_solve(gsx_context* c, HMode hm, int diagonal, double mind, double maxd, double lambda, bool backsolve) {
  if (hm == H_ALWAYS || (hm == H_IF_STALE && !c->h_ready)) dev_assemble_h(c);
  dev_damping(c, diagonal, mind, maxd);
  dev_factorize(c, lambda);
  if (backsolve) dev_backsolve(c);
}
// A damped step into d_delta by the handle's solver.  The direct solver is asynchronous (GSX_OK; the caller's readback and
// indeterminate() judge it); PCG synchronises and answers itself.
gsx_status damped_step(gsx_context* c, HMode hm, int diagonal, double mind, double maxd, double lambda) {
  if (!c->use_pcg()) {
    direct_solve(c, hm, diagonal, mind, maxd, lambda, true);
    return GSX_OK;
  }
  // (a PCG handle reads H only for diag(J'J), the weights of diagonal damping)
  if (diagonal && (hm == H_ALWAYS || (hm == H_IF_STALE && !c->h_ready))) dev_assemble_h(c);
  dev_damping(c, diagonal, mind, maxd);
  return pcg_solve(c, lambda, c->pcg_params, nullptr, nullptr);
}

gsx_status compute_error_sync(gsx_context* c, double* out) {
  dev_error(c, c->d_values.p, SC_ERR);
  gsx_status st = readback(c);
  if (st != GSX_OK) return st;
  *out = c->h_scalars[SC_ERR];
  return GSX_OK;
}

}  // namespace gsx

// ==================================================================================================
// C ABI
// ==================================================================================================
extern "C" {

const char* gsx_version(void) { return "gsx 0.1.0 (gfx950)"; }

int32_t gsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

gsx_status gsx_create(const gsx_problem_desc* desc, int32_t device, gsx_handle* out) {
  if (!out) return GSX_E_INVALID;
  *out = nullptr;
  gsx::call_error().clear();
  gsx_context* c = new gsx_context();
  gsx_status st = lower_problem(desc, c->P, c->err);
  if (st != GSX_OK) {
    std::fprintf(stderr, "gsx_create: %s\n", c->err.c_str());
    gsx::call_error() = "gsx_create: " + c->err;   // (no handle to ask: gsx_last_error(NULL))
    delete c;
    return st;
  }
  c->n_smart = (int)std::count(c->P.f_type.begin(), c->P.f_type.end(), (int)GSX_F_SMART_PROJECTION);
  c->device = device;
  c->opt = schedule_options_from_env();
  int n = 0;
  if (hipGetDeviceCount(&n) == hipSuccess && n > 0 && device >= 0 && device < n && hipSetDevice(device) == hipSuccess &&
      hipStreamCreate(&c->stream) == hipSuccess) {
    c->has_device = true;
    st = upload_problem(c);
    if (st != GSX_OK) {
      std::fprintf(stderr, "gsx_create: %s\n", c->err.c_str());
      delete c;
      return st;
    }
  }
  *out = c;
  return GSX_OK;
}

gsx_status gsx_destroy(gsx_handle h) {
  if (!h) return GSX_OK;
  if (h->has_device) {
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    for (auto& t : h->timers) {
      for (auto& ev : t.pending) t.pool.push_back(ev);
      for (auto& ev : t.pool) {
        hipEventDestroy(ev.first);
        hipEventDestroy(ev.second);
      }
    }
    if (h->bulk) {
      hipStreamSynchronize(h->bulk);
      hipStreamDestroy(h->bulk);
      if (h->bulk_go) hipEventDestroy(h->bulk_go);
      if (h->bulk_done) hipEventDestroy(h->bulk_done);
    }
    if (h->h_scalars) hipHostFree(h->h_scalars);
    if (h->h_status) hipHostFree(h->h_status);
    pcg_work_destroy(h->pcg);
    h->pcg = nullptr;
  }
  hipStream_t st = h->stream;
  const bool dev = h->has_device;
  delete h;
  if (dev && st) hipStreamDestroy(st);
  return GSX_OK;
}

const char* gsx_last_error(gsx_handle h) { return h ? h->err.c_str() : gsx::call_error().c_str(); }

gsx_status gsx_set_ordering(gsx_handle h, const uint64_t* keys, int32_t n) {
  if (!h || (!keys && n > 0)) return GSX_E_INVALID;
  if (n != h->P.n_vars) {
    h->err = "ordering size differs from the number of variables";
    return GSX_E_BAD_ORDERING;
  }
  std::map<uint64_t, int> idx;
  for (int v = 0; v < h->P.n_vars; ++v) idx[h->P.keys[v]] = v;
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) {
    auto it = idx.find(keys[i]);
    if (it == idx.end()) {
      h->err = "ordering contains a key that is not a variable of the graph";
      return GSX_E_BAD_ORDERING;
    }
    ord[i] = it->second;
  }
  if (h->sharded() && h->n_smart) {
    h->err = "a sharded handle takes no smart projection factors (their re-triangulation cache is per handle)";
    return GSX_E_STATE;
  }
  gsx_status st = symbolic_analysis(h->P, ord, h->relax, h->relax_max_f, h->shard_rank, h->shard_world, h->opt, h->S, h->err);
  if (st != GSX_OK) return st;
  h->order = ord;
  h->has_symbolic = true;
  if (h->has_device) {
    hipSetDevice(h->device);
    st = upload_symbolic(h);
    if (st != GSX_OK) return st;
  } else {
    plan_hessian_groups(h);   // (upload_symbolic makes this plan on a handle with a device: gsx_get_hessian_groups reads it)
  }
  return GSX_OK;
}

gsx_status gsx_compute_ordering(gsx_handle h, int32_t kind, uint64_t* keys_out) {
  if (!h || !keys_out || kind < 0 || kind > 4) return GSX_E_INVALID;
  std::vector<int> ord;
  compute_ordering(h->P, kind, h->opt, ord);
  for (int i = 0; i < h->P.n_vars; ++i) keys_out[i] = h->P.keys[ord[i]];
  return GSX_OK;
}

gsx_status gsx_set_amalgamation(gsx_handle h, double relax, int32_t max_frontal_dim) {
  if (!h || relax != relax || (relax >= 0.0 && max_frontal_dim < 1)) return GSX_E_INVALID;
  h->relax = relax;
  h->relax_max_f = max_frontal_dim;
  return GSX_OK;
}

gsx_status gsx_set_shard(gsx_handle h, int32_t rank, int32_t world, gsx_allreduce_fn allreduce, void* user) {
  if (!h || world < 1 || rank < 0 || rank >= world || (world > 1 && !allreduce)) return GSX_E_INVALID;
  if (h->has_symbolic) {
    h->err = "gsx_set_shard must precede gsx_set_ordering";
    return GSX_E_STATE;
  }
  if (world > 1 && h->use_pcg()) {
    h->err = "the PCG solver is not available on a sharded handle";
    return GSX_E_STATE;
  }
  h->shard_rank = rank;
  h->shard_world = world;
  h->shard_cb = allreduce;
  h->shard_user = user;
  return GSX_OK;
}

gsx_status gsx_get_shard(gsx_handle h, gsx_shard_info* info, int32_t* front_owner, int32_t* factor_owned) {
  if (!h || !h->has_symbolic) return GSX_E_STATE;
  const Symbolic& S = h->S;
  if (info) {
    info->rank = S.shard_rank;
    info->world = S.shard_world;
    info->n_cap_fronts = S.n_cap;
    info->n_own_fronts = 0;
    for (int f = 0; f < S.n_fronts; ++f) info->n_own_fronts += S.owner[f] == S.shard_rank;
    info->cap_level0 = S.cap_level0;
    info->n_own_factors = 0;
    for (char o : S.f_owned) info->n_own_factors += o != 0;
    info->cap_doubles = S.cap_end - S.cap_begin;
    info->cap_flops = S.cap_cost;
    info->own_flops = S.own_cost;
    info->total_flops = S.total_cost;
  }
  if (front_owner)
    for (int f = 0; f < S.n_fronts; ++f) front_owner[f] = S.owner[f];
  if (factor_owned)
    for (int f = 0; f < h->P.n_factors; ++f) factor_owned[f] = S.f_owned[f];
  return GSX_OK;
}

gsx_status gsx_get_front_classes(gsx_handle h, int32_t* classes) {
  if (!h || !classes) return GSX_E_INVALID;
  if (!h->has_symbolic) return GSX_E_STATE;
  const Symbolic& S = h->S;
  for (int f = 0; f < S.n_fronts; ++f)
    classes[f] = (S.med[f] ? 3 : S.cls[f]) | (S.tree_tier[f] >= 0 ? 4 : 0) | (S.lean[f] ? 8 : 0);
  return GSX_OK;
}

gsx_status gsx_get_gather_plan(gsx_handle h, int32_t* n_segments, int64_t* n_sources, int32_t* n_combines, int64_t* segments,
                               int32_t* sources, int32_t* combines) {
  if (!h) return GSX_E_INVALID;
  if (!h->has_symbolic) return GSX_E_STATE;
  const Symbolic& S = h->S;
  const int nseg = (int)S.gseg_task.size(), nm = (int)S.gm_task.size();
  if (n_segments) *n_segments = nseg;
  if (n_sources) *n_sources = (int64_t)S.gs_child.size();
  if (n_combines) *n_combines = nm;
  // (the side group is the last gather group, index n_ulevels: reported as -1)
  auto group_of = [&](const std::vector<int>& ptr, int i) {
    int l = 0;
    while (l < S.n_ulevels && i >= ptr[l + 1]) ++l;
    return l == S.n_ulevels ? -1 : l;
  };
  if (segments)
    for (int i = 0; i < nseg; ++i) {
      const int t = S.gseg_task[i], p = S.gt_front[t], dims = S.gt_dims[t];
      // the block's two parent variables, back from its arena offset: row r, column c of the front
      const int64_t rel = S.gt_dst[t] - S.off[p];
      const int rc[2] = {(int)(rel % S.N[p]), (int)(rel / S.N[p])};
      int var[2] = {-1, -1};   // -1: the right-hand side (row N - 1)
      for (int q = 0; q < 2; ++q) {
        int o = 0;
        for (int k = S.fvar_ptr[p]; k < S.fvar_ptr[p + 1] && var[q] < 0; ++k) {
          if (o == rc[q]) var[q] = S.fvars[k];
          o += h->P.dims[S.fvars[k]];
        }
      }
      int64_t* o = segments + (int64_t)i * 11;
      o[0] = group_of(S.gseg_lvl_ptr, i);
      o[1] = t;
      o[2] = p;
      o[3] = var[0];
      o[4] = var[1];
      o[5] = dims & 255;
      o[6] = (dims >> 8) & 255;
      o[7] = dims >> 16;
      o[8] = S.gseg_slot[i];
      o[9] = S.gseg_begin[i];
      o[10] = S.gseg_end[i];
    }
  if (sources)
    for (size_t i = 0; i < S.gs_child.size(); ++i) {
      sources[2 * i] = S.gs_child[i];
      sources[2 * i + 1] = S.gs_loc2[i] >= 0 ? S.F[S.gs_child[i]] : 0;
    }
  if (combines)
    for (int i = 0; i < nm; ++i) {
      combines[4 * i] = group_of(S.gm_lvl_ptr, i);
      combines[4 * i + 1] = S.gm_task[i];
      combines[4 * i + 2] = S.gm_slot[i];
      combines[4 * i + 3] = S.gm_nslots[i];
    }
  return GSX_OK;
}

gsx_status gsx_get_hessian_groups(gsx_handle h, int32_t* classes, int32_t* group, int32_t* position, int32_t* bundle,
                                  int32_t* bundle_size, int32_t* fused_diag_star) {
  if (!h) return GSX_E_INVALID;
  if (!h->has_symbolic) {
    h->err = "ordering not set";
    return GSX_E_STATE;
  }
  const int n = h->P.n_vars;
  // star variable at position p of its group -> its bundle
  std::vector<int> bundle_at;
  for (size_t b = 0; b < h->h_star_bundles.size(); ++b) bundle_at.insert(bundle_at.end(), h->h_star_bundles[b].y, (int)b);
  bool has_bundled_star = false, has_diag = false;
  for (int v = 0; v < n; ++v) {
    const int g = h->hv_group_of_var[v];
    int cls = -1, pos = -1, bi = -1, bn = 0;
    if (g >= 0) {
      const gsx_context::HGroup& G = h->hgroups[g];
      cls = G.threads == -2 ? GSX_H_TILE : G.threads == -1 ? GSX_H_STAR : G.threads == 0 ? GSX_H_DIAG
            : G.global ? GSX_H_HUGE : G.threads == 64 ? GSX_H_LIGHT : GSX_H_HEAVY;
      pos = h->hv_pos[v] - G.begin;
      if (cls == GSX_H_STAR && pos < (int)bundle_at.size()) {   // (the bundles tile the group in order, or there are none)
        bi = bundle_at[pos];
        bn = h->h_star_bundles[bi].y;
      }
      has_bundled_star |= cls == GSX_H_STAR && h->n_star_bundles > 0;
      has_diag |= cls == GSX_H_DIAG;
    }
    if (classes) classes[v] = cls;
    if (group) group[v] = g;
    if (position) position[v] = pos;
    if (bundle) bundle[v] = bi;
    if (bundle_size) bundle_size[v] = bn;
  }
  if (fused_diag_star) *fused_diag_star = has_bundled_star && has_diag && !h->fused_star;   // (dev_assemble_h)
  return GSX_OK;
}

gsx_status gsx_get_hessian_panel(gsx_handle h, uint64_t key, int32_t* rows, int32_t* dim, double* out, int32_t* row_var,
                                 int32_t* row_scalar) {
  if (!h) return GSX_E_INVALID;
  if (!h->has_symbolic) {
    h->err = "ordering not set";
    return GSX_E_STATE;
  }
  const HostProblem& P = h->P;
  const Symbolic& S = h->S;
  int v = -1;
  for (int k = 0; k < P.n_vars && v < 0; ++k)
    if (P.keys[k] == key) v = k;
  if (v < 0) {
    h->err = "no variable has this key";
    return GSX_E_INVALID;
  }
  if (!S.scheduled[S.front_of_var[v]]) {
    h->err = "the variable belongs to another rank's subtree: its panel is not assembled on this handle";
    return GSX_E_STATE;
  }
  const int d = P.dims[v], nrows = S.h_rows[v];
  if (rows) *rows = nrows;
  if (dim) *dim = d;
  if (!out) return GSX_OK;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (!h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  if (row_var && row_scalar) {
    // the panel's rows: the variable, its later-eliminated neighbours in elimination order, the right-hand side
    std::vector<int> nb;
    for (int f = 0; f < P.n_factors; ++f) {
      bool has = false;
      for (int q = P.f_key_ptr[f]; q < P.f_key_ptr[f + 1]; ++q) has |= P.f_vars[q] == v;
      for (int q = P.f_key_ptr[f]; has && q < P.f_key_ptr[f + 1]; ++q)
        if (S.pos[P.f_vars[q]] > S.pos[v]) nb.push_back(P.f_vars[q]);
    }
    std::sort(nb.begin(), nb.end(), [&](int a, int b) { return S.pos[a] < S.pos[b]; });
    nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
    nb.insert(nb.begin(), v);
    int r = 0;
    for (int u : nb)
      for (int k = 0; k < P.dims[u] && r < nrows - 1; ++k, ++r) row_var[r] = u, row_scalar[r] = k;
    if (r != nrows - 1) {
      h->err = "internal: the panel's rows are not those of the variable's later neighbours";
      return GSX_E_INVALID;
    }
    row_var[r] = -1;
    row_scalar[r] = 0;
  }
  if (!h->h_ready) dev_assemble_h(h);
  dev_ensure_hstar(h);   // (the star leaves' panels: the factorization forms them in registers)
  return download(h, h->d_H.p + S.h_off[v], out, (int64_t)nrows * d);
}

gsx_status gsx_scratch_buffer(gsx_handle h, double** device_ptr, int64_t* count) {
  if (!h || !device_ptr || !count) return GSX_E_INVALID;
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  *device_ptr = h->d_partials.p;   // (rewritten from scratch by every reduction that uses it)
  *count = gsx_context::kPartials;
  return GSX_OK;
}

gsx_status gsx_get_ordering(gsx_handle h, uint64_t* keys_out) {
  if (!h || !h->has_symbolic) return GSX_E_STATE;
  for (int i = 0; i < h->P.n_vars; ++i) keys_out[i] = h->P.keys[h->order[i]];
  return GSX_OK;
}

gsx_status gsx_get_tree(gsx_handle h, int32_t* n_fronts, int64_t* n_sep_total, int32_t* parent, int32_t* frontal_ptr,
                        int32_t* frontal_vars, int32_t* sep_ptr, int32_t* sep_vars) {
  if (!h || !h->has_symbolic) return GSX_E_STATE;
  const Symbolic& S = h->S;
  if (n_fronts) *n_fronts = S.n_fronts;
  if (n_sep_total) *n_sep_total = (int64_t)S.fvars.size() - h->P.n_vars;
  if (!parent) return GSX_OK;
  int fp = 0, sp = 0;
  for (int f = 0; f < S.n_fronts; ++f) {
    parent[f] = S.parent[f];
    frontal_ptr[f] = fp;
    sep_ptr[f] = sp;
    for (int k = S.fvar_ptr[f]; k < S.fvar_ptr[f + 1]; ++k) {
      if (k - S.fvar_ptr[f] < S.nfrontal_vars[f]) frontal_vars[fp++] = S.fvars[k];
      else sep_vars[sp++] = S.fvars[k];
    }
  }
  frontal_ptr[S.n_fronts] = fp;
  sep_ptr[S.n_fronts] = sp;
  return GSX_OK;
}

int64_t gsx_state_size(gsx_handle h) { return h ? h->P.state_size : 0; }
int64_t gsx_tangent_size(gsx_handle h) { return h ? h->P.tan_size : 0; }
int64_t gsx_jacobian_size(gsx_handle h) { return h ? h->P.jac_size : 0; }

// the copy of gsx_set_values without its check of the directions: for the zeros a handle of GSX_F_LINEAR factors is given
// (gsx_solve_gfg, gsx_solve_gfg_h), which reads no state
static gsx_status set_values_unchecked(gsx_handle h, const double* packed, int64_t n) {
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  hipSetDevice(h->device);
  if (n > 0) {
    HIPCHK(h, hipMemcpyAsync(h->d_values.p, packed, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->values_written();
  return GSX_OK;
}

gsx_status gsx_set_values(gsx_handle h, const double* packed, int64_t n) {
  if (!h || n != h->P.state_size || (!packed && n > 0)) return GSX_E_INVALID;
  if (!h->P.direction_vars.empty() && check_direction_states(h->P, packed, h->err) != GSX_OK) return GSX_E_INVALID;
  return set_values_unchecked(h, packed, n);
}

gsx_status gsx_get_values(gsx_handle h, double* packed, int64_t n) {
  if (!h || n != h->P.state_size || (!packed && n > 0)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  if (h->sharded() && !h->values_synced && h->has_symbolic) {
    // every variable from its owner: the ranks only kept their own subtrees (and the cap) current
    launch_mask_copy(h->d_values.p, h->d_own_state.p, n, h->d_trial.p, h->stream);
    shard_allreduce(h, h->d_trial.p, n);
    h->values_gathered();
    if (h->shard_failed) {
      h->shard_failed = false;
      h->err = "the all-reduce callback of a sharded handle failed";
      return GSX_E_NO_DEVICE;
    }
  }
  return download(h, h->d_values.p, packed, n);
}

gsx_status gsx_error(gsx_handle h, double* out) {
  if (!h || !out) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  return compute_error_sync(h, out);
}

gsx_status gsx_linearize(gsx_handle h) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  dev_linearize(h);
  return readback(h);
}

gsx_status gsx_get_jacobians(gsx_handle h, double* out, int64_t n) {
  if (!h || n != h->P.jac_size || (!out && n > 0)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  if (!h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  return download(h, h->d_jac.p, out, n);
}

gsx_status gsx_hessian_diagonal(gsx_handle h, double* out, int64_t n) {
  if (!h || n != h->P.tan_size || (!out && n > 0)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (!h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  if (!h->h_ready) dev_assemble_h(h);
  dev_hessian_diag(h);
  return download(h, h->d_hdiag.p, out, n);
}

gsx_status gsx_solve(gsx_handle h, double lambda, int32_t diagonal_damping, double min_diagonal, double max_diagonal,
                     double* delta_out, int64_t n, uint64_t* bad_key) {
  if (!h || (delta_out && n != h->P.tan_size)) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (!h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  if (!h->h_ready) dev_assemble_h(h);
  // (the undamped factorization of this very linearization may already be resident: after gsx_relinearize_partial,
  // a marginal query or a previous lambda = 0 solve; then only the back-substitution runs)
  if (!(lambda == 0.0 && h->fact_valid && h->fact_lambda == 0.0)) {
    direct_solve(h, H_KEEP, diagonal_damping, min_diagonal, max_diagonal, lambda, false);
  } else {
    launch_begin_factorization(h->d_scalars.p, 0.0, h->d_status.p, nullptr, h->stream);  // status reset for the substitution
    h->sc_dirty |= kXFact;
  }
  dev_backsolve(h);
  st = readback(h);
  if (st != GSX_OK) return st;
  st = indeterminate(h, bad_key, true);
  if (st != GSX_OK) {
    h->delta_outdated();
    return st;
  }
  h->step_solved(lambda == 0.0 && !h->sharded());  // a complete undamped solution: what a later wildfire pass starts from
  const double* src = h->d_delta.p;
  if (delta_out && n > 0 && h->sharded()) {
    launch_mask_copy(h->d_delta.p, h->d_own_tan.p, n, h->d_udelta.p, h->stream);
    shard_allreduce(h, h->d_udelta.p, n);
    src = h->d_udelta.p;
  }
  return download(h, src, delta_out, n);
}

void gsx_pcg_params_default(gsx_pcg_params* p) {
  // ConjugateGradientParameters() — gtsam/linear/ConjugateGradientSolver.h:45-51: minIterations 1, maxIterations 500,
  // reset 501, epsilon_rel 1e-3, epsilon_abs 1e-3
  if (p) *p = gsx_pcg_params{500, 1, 501, 1e-3, 1e-3, GSX_PRECOND_BLOCK_JACOBI};
}

gsx_status gsx_set_linear_solver(gsx_handle h, int32_t kind, const gsx_pcg_params* params) {
  if (!h || (kind != GSX_SOLVER_MULTIFRONTAL && kind != GSX_SOLVER_PCG)) return GSX_E_INVALID;
  if (kind == GSX_SOLVER_MULTIFRONTAL) {
    h->solver_kind = kind;
    return GSX_OK;
  }
  gsx_pcg_params prm;
  gsx_pcg_params_default(&prm);
  if (params) prm = *params;
  if (const char* what = pcg_params_error(prm)) {
    h->err = what;
    return GSX_E_INVALID;
  }
  gsx_status st = pcg_refusal(h);
  if (st != GSX_OK) return st;
  h->solver_kind = kind;
  h->pcg_params = prm;
  return GSX_OK;
}

gsx_status gsx_solve_pcg(gsx_handle h, double lambda, int32_t diagonal_damping, double min_diagonal, double max_diagonal,
                         const gsx_pcg_params* params, double* delta_out, int64_t n, gsx_pcg_stats* stats_out,
                         uint64_t* bad_key) {
  if (!h || !params || !(lambda >= 0.0) || (delta_out && n != h->P.tan_size)) return GSX_E_INVALID;
  if (const char* what = pcg_params_error(*params)) {
    h->err = what;
    return GSX_E_INVALID;
  }
  gsx_status st = begin_call(h, true, diagonal_damping != 0);
  if (st != GSX_OK) return st;
  st = pcg_refusal(h);
  if (st != GSX_OK) return st;
  if (!h->linearized) {
    h->err = "linearize first";
    return GSX_E_STATE;
  }
  if (diagonal_damping && !h->h_ready) dev_assemble_h(h);   // diag(J'J) is read from the H panels
  dev_damping(h, diagonal_damping, min_diagonal, max_diagonal);
  st = pcg_solve(h, lambda, *params, stats_out, bad_key);
  if (st != GSX_OK) return st;
  return download(h, h->d_delta.p, delta_out, n);
}

gsx_status gsx_linear_error(gsx_handle h, double* e0, double* ed) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  if (!h->linearized || (ed && !h->solved)) {
    h->err = "linearize (and solve) first";
    return GSX_E_STATE;
  }
  dev_linear_error(h);
  st = readback(h);
  if (st != GSX_OK) return st;
  if (e0) *e0 = h->h_scalars[SC_LIN0];
  if (ed) *ed = h->h_scalars[SC_LIND];
  return GSX_OK;
}

gsx_status gsx_retract(gsx_handle h, const double* delta, int64_t n, int32_t commit, double* trial_error) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = begin_call(h, true, false);
  if (st != GSX_OK) return st;
  const double* dd = h->d_delta.p;
  if (delta) {
    if (n != h->P.tan_size) return GSX_E_INVALID;
    if (n > 0) HIPCHK(h, hipMemcpyAsync(h->d_udelta.p, delta, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    dd = h->d_udelta.p;
  } else if (!h->solved) {
    h->err = "no delta: solve first";
    return GSX_E_STATE;
  }
  dev_retract(h, dd);
  if (trial_error) dev_error(h, h->d_trial.p, SC_TRIAL_ERR);
  st = readback(h);
  if (st != GSX_OK) return st;
  if (trial_error) *trial_error = h->h_scalars[SC_TRIAL_ERR];
  if (commit) h->trial_accepted(false);
  return GSX_OK;
}

// Marginals::marginalCovariance(key) — gtsam/nonlinear/Marginals.cpp:107-136 — from the undamped factorization of the
// current linearization (the block of H^-1 in the variable's tangent space), out: dA x dA column-major.
namespace {
// the undamped factorization of the current linearization, resident in the arena (shared by the marginal entry points)
gsx_status marginals_prepare(gsx_handle h) {
  gsx_status st = begin_call(h, true, true);
  if (st != GSX_OK) return st;
  if (h->sharded()) {
    h->err = "marginals are not available on a sharded handle";
    return GSX_E_STATE;
  }
  if (!h->linearized) dev_linearize(h);
  if (!h->h_ready) dev_assemble_h(h);
  if (!h->fact_valid || h->fact_lambda != 0.0) {
    direct_solve(h, H_KEEP, 0, 0, 0, 0.0, false);
    st = readback(h);
    if (st != GSX_OK) return st;
    st = indeterminate(h, nullptr, false);
    if (st != GSX_OK) return st;
    h->delta_outdated();  // the back-substitution of a previous solve no longer matches the arena
  }
  return GSX_OK;
}
int find_var(gsx_handle h, uint64_t key) {
  auto it = std::lower_bound(h->P.keys.begin(), h->P.keys.end(), key);
  return (it == h->P.keys.end() || *it != key) ? -1 : (int)(it - h->P.keys.begin());
}
}  // namespace

// Marginals::jointMarginalCovariance — gtsam/nonlinear/Marginals.cpp:138-189 (there: eliminate down to the joint, take
// the information, invert).  Here: the columns (L^-1)_{:,v} of every requested variable are kept, and block (a, b) of
// the joint covariance is their product.
gsx_status gsx_joint_marginal_covariance(gsx_handle h, const uint64_t* keys, int32_t n_keys, double* out, int64_t n_out) {
  if (!h || !keys || !out || n_keys < 1 || n_keys > 64) return GSX_E_INVALID;
  gsx_status st = marginals_prepare(h);
  if (st != GSX_OK) return st;
  const Symbolic& S = h->S;
  if (h->constrained()) {
    // (the rewritten fronts give a constraint pivot unit variance where the reference's conditional has sigma 0)
    h->err = "marginal covariances are not available on a problem with hard constraints";
    return GSX_E_STATE;
  }
  // column groups: a variable's unit columns go through the path kernel at most 16 at a time (fewer when the cliques on its
  // path to the root are tall: the kernel keeps two (rows x columns) panels in LDS) — Marginals.cpp:107-136 has no limit on
  // the dimension of a variable, and neither has this entry point
  struct Group {
    int var, col0, width, off;   // off: first row / column of the group in the joint matrix
  };
  std::vector<Group> groups;
  std::vector<int> vars(n_keys);
  int D = 0;
  constexpr size_t kLds = 160 * 1024 - 4096 - 4096;
  for (int k = 0; k < n_keys; ++k) {
    vars[k] = find_var(h, keys[k]);
    if (vars[k] < 0) {
      h->err = "joint marginal of a key that is not a variable of the graph";
      return GSX_E_INVALID;
    }
    for (int q = 0; q < k; ++q)
      if (vars[q] == vars[k]) return GSX_E_INVALID;
    int max_n = 0;
    for (int f = S.front_of_var[vars[k]]; f >= 0; f = S.parent[f]) max_n = std::max(max_n, S.N[f]);
    const int fit = (int)std::min<size_t>(16, kLds / ((size_t)2 * max_n * sizeof(double)));
    if (fit < 1) {
      h->err = "marginal: the cliques on the path to the root are too large for the one-workgroup kernel";
      return GSX_E_NOMEM;
    }
    const int d = h->P.dims[vars[k]];
    for (int c0 = 0; c0 < d; c0 += fit) groups.push_back({vars[k], c0, std::min(fit, d - c0), D + c0});
    D += d;
  }
  if (n_out != (int64_t)D * D) return GSX_E_INVALID;
  const int64_t nt = std::max<int64_t>(h->P.tan_size, 1);
  DevBuf<double> d_Y, d_blk, d_sig;
  DevBuf<int> d_path;
  HIPCHK(h, d_Y.alloc((size_t)nt * D));
  HIPCHK(h, d_blk.alloc((size_t)16 * 16));
  HIPCHK(h, d_sig.alloc(256));
  HIPCHK(h, hipMemsetAsync(d_Y.p, 0, (size_t)nt * D * sizeof(double), h->stream));
  for (const Group& g : groups) {
    std::vector<int> path;
    int max_n = 0;
    for (int f = S.front_of_var[g.var]; f >= 0; f = S.parent[f]) {
      path.push_back(f);
      max_n = std::max(max_n, S.N[f]);
    }
    HIPCHK(h, d_path.upload(path, h->stream));
    launch_marginal_path(h->DS, d_path.p, (int)path.size(), S.h_loc[g.var] + g.col0, g.width, max_n, h->d_arena.p, d_sig.p,
                         d_Y.p + (size_t)g.off * nt, nt, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (d_path is reused)
  }
  std::vector<double> blk((size_t)16 * 16);
  for (size_t a = 0; a < groups.size(); ++a)
    for (size_t b = a; b < groups.size(); ++b) {
      const int dA = groups[a].width, dB = groups[b].width, oa = groups[a].off, ob = groups[b].off;
      launch_joint_cross(d_Y.p + (size_t)oa * nt, d_Y.p + (size_t)ob * nt, nt, dA, dB, d_blk.p, h->stream);
      HIPCHK(h, hipMemcpyAsync(blk.data(), d_blk.p, (size_t)dA * dB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      for (int i = 0; i < dA; ++i)
        for (int j = 0; j < dB; ++j) {
          const double x = blk[i + (size_t)j * dA];
          out[(size_t)(oa + i) * D + ob + j] = x;
          out[(size_t)(ob + j) * D + oa + i] = x;
        }
    }
  HIPCHK(h, hipGetLastError());
  return GSX_OK;
}

gsx_status gsx_marginal_covariance(gsx_handle h, uint64_t key, double* out, int64_t n_out) {
  if (!h || !out) return GSX_E_INVALID;
  const int v = find_var(h, key);
  if (v < 0) {
    h->err = "marginal of a key that is not a variable of the graph";
    return GSX_E_INVALID;
  }
  const int dA = h->P.dims[v];
  if (n_out != (int64_t)dA * dA) return GSX_E_INVALID;
  gsx_status st = marginals_prepare(h);
  if (st != GSX_OK) return st;
  const Symbolic& S = h->S;
  if (h->constrained()) {
    h->err = "marginal covariances are not available on a problem with hard constraints";
    return GSX_E_STATE;
  }
  std::vector<int> path;
  int max_n = 0;
  for (int f = S.front_of_var[v]; f >= 0; f = S.parent[f]) {
    path.push_back(f);
    max_n = std::max(max_n, S.N[f]);
  }
  // a wide variable, or tall cliques on its path: the variable's columns in groups (the joint entry point splits them)
  if (dA > 16 || (size_t)2 * max_n * dA * sizeof(double) > 160 * 1024 - 4096 - 4096)
    return gsx_joint_marginal_covariance(h, &key, 1, out, n_out);
  DevBuf<int> d_path;
  DevBuf<double> d_out;
  HIPCHK(h, d_path.upload(path, h->stream));
  HIPCHK(h, d_out.alloc((size_t)dA * dA));
  launch_marginal_path(h->DS, d_path.p, (int)path.size(), S.h_loc[v], dA, max_n, h->d_arena.p, d_out.p, nullptr, 0,
                       h->stream);
  HIPCHK(h, hipMemcpyAsync(out, d_out.p, (size_t)dA * dA * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  return GSX_OK;
}

namespace {
// the covariance arena of the current tree: a block and a work area per front of class 1 or 2 (kernels.h: MargArgs)
gsx_status marg_arena_ready(gsx_context* c) {
  if (c->marg_arena) return GSX_OK;
  const Symbolic& S = c->S;
  std::vector<i64> slot(std::max(S.n_fronts, 1), -1), work(std::max(S.n_fronts, 1), -1);
  i64 cur = 0;
  for (int f = 0; f < S.n_fronts; ++f) {
    if (S.cls[f] == 0) continue;
    const i64 m = S.N[f] - 1;
    slot[f] = cur;
    cur += m * m;
    work[f] = cur;
    cur += (i64)S.F[f] * m;
  }
  HIPCHK(c, c->d_marg_slot.upload(slot, c->stream));
  HIPCHK(c, c->d_marg_work.upload(work, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->d_marg_cov.alloc((size_t)std::max<i64>(cur, 1)) != hipSuccess) {
    (void)hipGetLastError();
    c->d_marg_cov.p = nullptr;
    c->d_marg_cov.n = 0;
    c->err = "marginal covariances: the covariance arena (" + std::to_string(8.0 * (double)cur / 1e9) + " GB) does not fit";
    return GSX_E_NOMEM;
  }
  c->marg_cov_doubles = cur;
  c->marg_arena = true;
  return GSX_OK;
}

// Work lists for the variables `vars` (output order); all: every variable, else only the fronts on their paths to the root.
gsx_status marg_build_plan(gsx_context* c, const std::vector<int>& vars, bool all, gsx_context::MargPlan& plan) {
  const Symbolic& S = c->S;
  const HostProblem& P = c->P;
  plan.release();
  std::vector<i64> out_off(std::max(P.n_vars, 1), -1);
  for (int v : vars) {
    out_off[v] = plan.total;
    plan.total += (int64_t)P.dims[v] * P.dims[v];
  }
  std::vector<char> need(S.n_fronts, all ? 1 : 0);
  if (!all)
    for (int v : vars)
      for (int f = S.front_of_var[v]; f >= 0 && !need[f]; f = S.parent[f]) need[f] = 1;
  int n_levels = 0;
  for (int f = 0; f < S.n_fronts; ++f) n_levels = std::max(n_levels, S.level[f] + 1);
  std::vector<std::vector<int>> by_level(n_levels);
  for (int f = 0; f < S.n_fronts; ++f)
    if (need[f] && S.cls[f] != 0) by_level[S.level[f]].push_back(f);
  std::vector<int2> emit;
  std::vector<int> leaves;
  {
    std::vector<char> listed(S.n_fronts, 0);
    for (int v : vars) {
      const int f = S.front_of_var[v];
      if (S.cls[f] != 0) emit.push_back(make_int2(v, f));
      else if (!listed[f]) {
        listed[f] = 1;
        leaves.push_back(f);
      }
    }
  }
  std::vector<MargItem> items, step[4];
  for (int lvl = n_levels - 1; lvl >= 0; --lvl) {
    if (by_level[lvl].empty()) continue;
    for (auto& sv : step) sv.clear();
    for (int f : by_level[lvl]) {
      const int F = S.F[f], s = S.N[f] - 1 - F;
      const int tf = (F + 31) / 32, ts = (s + 31) / 32;
      step[0].push_back(MargItem{f, -1, 0, 0});
      for (int ti = 0; ti < ts; ++ti) step[0].push_back(MargItem{f, ti, 0, 0});
      for (int tj = 0; tj < tf; ++tj)
        for (int ti = 0; ti < ts; ++ti) {
          step[1].push_back(MargItem{f, ti, tj, 0});
          step[2].push_back(MargItem{f, ti, tj, 0});
        }
      for (int tj = 0; tj < tf; ++tj)
        for (int ti = tj; ti < tf; ++ti) step[3].push_back(MargItem{f, ti, tj, 0});
    }
    gsx_context::MargLevel L;
    for (int k = 0; k < 4; ++k) {
      L.begin[k] = (int)items.size();
      L.count[k] = (int)step[k].size();
      items.insert(items.end(), step[k].begin(), step[k].end());
    }
    plan.levels.push_back(L);
  }
  if (items.size() > (size_t)INT_MAX) {
    c->err = "marginal covariances: too many tiles";
    return GSX_E_NOMEM;
  }
  plan.n_emit = (int)emit.size();
  plan.n_leaves = (int)leaves.size();
  HIPCHK(c, plan.d_items.upload(items, c->stream));
  HIPCHK(c, plan.d_emit.upload(emit, c->stream));
  HIPCHK(c, plan.d_leaves.upload(leaves, c->stream));
  HIPCHK(c, plan.d_out_off.upload(out_off, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host vectors go out of scope)
  plan.ready = true;
  return GSX_OK;
}

extern "C++" {
template <class Fn>
void marg_timed(gsx_context* c, int ph, Fn launch) {
  if (c->profiling > 0) timer_begin(c, ph);
  launch();
  if (c->profiling > 0) timer_end(c, ph);
}
}

gsx_status marg_run(gsx_context* c, const gsx_context::MargPlan& plan, double* out) {
  DevBuf<double> d_out;
  HIPCHK(c, d_out.alloc((size_t)std::max<int64_t>(plan.total, 1)));
  const MargArgs M{c->d_marg_slot.p, c->d_marg_work.p, c->d_marg_cov.p, c->d_arena.p, plan.d_out_off.p, c->d_var_dim.p, d_out.p};
  hipStream_t st = c->stream;
  const MargItem* items = plan.d_items.p;
  timer_begin(c, PH_MARGINALS);
  for (const gsx_context::MargLevel& L : plan.levels) {
    marg_timed(c, PH_M_PREP, [&] { launch_marg_prep(c->DS, M, items + L.begin[0], L.count[0], st); });
    marg_timed(c, PH_M_KT, [&] { launch_marg_kt(c->DS, M, items + L.begin[1], L.count[1], st); });
    marg_timed(c, PH_M_SF, [&] { launch_marg_sf(c->DS, M, items + L.begin[2], L.count[2], st); });
    marg_timed(c, PH_M_FF, [&] { launch_marg_ff(c->DS, M, items + L.begin[3], L.count[3], st); });
  }
  marg_timed(c, PH_M_EMIT, [&] { launch_marg_emit(c->DS, M, plan.d_emit.p, plan.n_emit, st); });
  marg_timed(c, PH_M_LEAF, [&] { launch_marg_leaf(c->DS, M, plan.d_leaves.p, plan.n_leaves, st); });
  timer_end(c, PH_MARGINALS);
  if (plan.total) HIPCHK(c, hipMemcpyAsync(out, d_out.p, (size_t)plan.total * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return GSX_OK;
}

// the variables of a key list (nullptr: all, ascending key order = variable order); -1 for an unknown or repeated key
int64_t marg_key_vars(gsx_context* c, const uint64_t* keys, int32_t n_keys, std::vector<int>* vars) {
  const HostProblem& P = c->P;
  int64_t total = 0;
  if (!keys) {
    for (int v = 0; v < P.n_vars; ++v) {
      if (vars) vars->push_back(v);
      total += (int64_t)P.dims[v] * P.dims[v];
    }
    return total;
  }
  if (n_keys < 0) return -1;
  std::vector<char> seen(std::max(P.n_vars, 1), 0);
  for (int k = 0; k < n_keys; ++k) {
    const int v = find_var(c, keys[k]);
    if (v < 0 || seen[v]) return -1;
    seen[v] = 1;
    if (vars) vars->push_back(v);
    total += (int64_t)P.dims[v] * P.dims[v];
  }
  return total;
}

static gsx_status gsx_marginal_covariances_impl(gsx_handle h, const uint64_t* keys, int32_t n_keys, double* out, int64_t n_out) {
  if (!h || (!out && n_out != 0)) return GSX_E_INVALID;
  std::vector<int> vars;
  const int64_t total = marg_key_vars(h, keys, n_keys, &vars);
  if (total < 0) {
    h->err = "marginals of a key list with an unknown or repeated key";
    return GSX_E_INVALID;
  }
  if (n_out != total) {
    h->err = "marginals: n_out differs from gsx_marginal_blocks_size";
    return GSX_E_INVALID;
  }
  gsx_status st = marginals_prepare(h);
  if (st != GSX_OK) return st;
  if (h->constrained()) {
    h->err = "marginal covariances are not available on a problem with hard constraints";
    return GSX_E_STATE;
  }
  st = marg_arena_ready(h);
  if (st != GSX_OK) return st;
  if (!keys) {
    if (!h->marg_all.ready) {
      st = marg_build_plan(h, vars, true, h->marg_all);
      if (st != GSX_OK) return st;
    }
    return marg_run(h, h->marg_all, out);
  }
  gsx_context::MargPlan plan;
  st = marg_build_plan(h, vars, false, plan);
  if (st != GSX_OK) return st;
  return marg_run(h, plan, out);
}
}  // namespace

int64_t gsx_marginal_blocks_size(gsx_handle h, const uint64_t* keys, int32_t n_keys) {
  if (!h) return -1;
  try {
    return marg_key_vars(h, keys, n_keys, nullptr);
  } catch (const std::exception&) {
    return -1;
  }
}

static gsx_status gsx_set_block_jacobians_impl(gsx_handle h, int32_t first_factor, int32_t n_factors, const double* values,
                                   int64_t n_values) {
  if (!h || !values || first_factor < 0 || n_factors < 0 || (int64_t)first_factor + (int64_t)n_factors > (int64_t)h->P.n_factors) return GSX_E_INVALID;
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  const HostProblem& P = h->P;
  int64_t need = 0;
  for (int f = first_factor; f < first_factor + n_factors; ++f) {
    if (P.f_type[f] != GSX_F_LINEAR) {
      h->err = "gsx_set_block_jacobians: not a GSX_F_LINEAR factor";
      return GSX_E_INVALID;
    }
    need += (int64_t)P.f_rows[f] * P.f_cols[f];
  }
  if (need != n_values) return GSX_E_INVALID;
  if (n_factors == 0) return GSX_OK;
  hipSetDevice(h->device);
  // the factors' blocks are consecutive in the Jacobian pool when the factors are: one staging buffer, one copy per run
  std::vector<double>& stage = h->jac_stage;
  stage.resize((size_t)need);
  int64_t src = 0;
  for (int f = first_factor; f < first_factor + n_factors; ++f) {
    whiten_linear_factor(P, f, values + src, stage.data() + src);
    src += (int64_t)P.f_rows[f] * P.f_cols[f];
  }
  src = 0;
  for (int f = first_factor; f < first_factor + n_factors;) {
    int e = f;
    int64_t len = 0;
    while (e < first_factor + n_factors && P.f_jac_off[e] == P.f_jac_off[f] + len) {
      len += (int64_t)P.f_rows[e] * P.f_cols[e];
      ++e;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_jac.p + P.f_jac_off[f], stage.data() + src, (size_t)len * sizeof(double),
                             hipMemcpyHostToDevice, h->stream));
    src += len;
    f = e;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (the staging buffer is reused by the next call)
  h->blocks_written(false);   // H must be re-assembled from the new blocks
  return GSX_OK;
}

gsx_status gsx_solve_gfg_h(gsx_handle h, const double* blocks, int64_t n_blocks, double* delta_out, int64_t n,
                           uint64_t* bad_key) {
  if (!h || !delta_out) return GSX_E_INVALID;
  for (int f = 0; f < h->P.n_factors; ++f)
    if (h->P.f_type[f] != GSX_F_LINEAR) {
      h->err = "gsx_solve_gfg_h: the handle must hold GSX_F_LINEAR factors only";
      return GSX_E_INVALID;
    }
  gsx_status st = GSX_OK;
  if (blocks) st = gsx_set_block_jacobians(h, 0, h->P.n_factors, blocks, n_blocks);
  if (st != GSX_OK) return st;
  if (!h->values_set) {
    std::vector<double> zeros(h->P.state_size, 0.0);
    st = set_values_unchecked(h, zeros.data(), h->P.state_size);
    if (st != GSX_OK) return st;
  }
  h->linear_graph_given();
  return gsx_solve(h, 0.0, 0, 0, 0, delta_out, n, bad_key);
}

static gsx_status gsx_get_conditional_impl(gsx_handle h, int32_t front, int32_t* n_frontal, int32_t* n_cols, double* out,
                               int64_t n_out) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = begin_call(h, false, true);
  if (st != GSX_OK) return st;
  const Symbolic& S = h->S;
  if (front < 0 || front >= S.n_fronts) return GSX_E_INVALID;
  const int F = S.F[front], N = S.N[front];  // N = F + separator + 1 (rhs)
  if (n_frontal) *n_frontal = F;
  if (n_cols) *n_cols = N;
  if (!out) return GSX_OK;
  if (n_out != (int64_t)F * N) return GSX_E_INVALID;
  if (!h->fact_valid) {
    h->err = "gsx_get_conditional: no factorization resident (solve first)";
    return GSX_E_STATE;
  }
  if (h->sharded() && !S.scheduled[front]) {
    h->err = "gsx_get_conditional: the clique belongs to another rank";
    return GSX_E_STATE;
  }
  // the front keeps L = [R S d]' column by column: L[r][c] at r + c N; blocked (big) fronts keep the rows below each
  // 32 x 32 diagonal tile in their L-panel area (kernels.h: BigDesc)
  const bool big = S.cls[front] == 2;
  const i64 cols = (i64)N * F;
  std::vector<double> sq((size_t)cols), xp;
  HIPCHK(h, hipMemcpyAsync(sq.data(), h->d_arena.p + S.off[front], (size_t)cols * sizeof(double), hipMemcpyDeviceToHost,
                           h->stream));
  if (big) {
    xp.resize((size_t)cols);
    HIPCHK(h, hipMemcpyAsync(xp.data(), h->d_arena.p + S.off[front] + big_panel_offset(N), (size_t)cols * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int c = 0; c < F; ++c)        // column c of L = row c of [R S d]
    for (int r = 0; r < N; ++r) {
      double v = 0.0;
      if (r >= c) {
        const bool in_tile = big && r < F && (r / kTile) == (c / kTile);
        v = (big && !in_tile) ? xp[(size_t)r + (size_t)c * N] : sq[(size_t)r + (size_t)c * N];
      }
      out[(size_t)c + (size_t)r * F] = v;  // F x N column-major: entry (row c, column r)
    }
  return GSX_OK;
}

gsx_status gsx_solve_gfg(const gsx_problem_desc* desc, const uint64_t* ordering, int32_t device, double* delta_out,
                         int64_t n, uint64_t* bad_key) {
  if (!desc || !delta_out) return GSX_E_INVALID;
  for (int f = 0; f < desc->n_factors; ++f)
    if (desc->f_type[f] != GSX_F_LINEAR) return GSX_E_INVALID;
  gsx_handle h = nullptr;
  gsx_status st = gsx_create(desc, device, &h);
  if (st != GSX_OK) return st;
  std::vector<uint64_t> ord(desc->n_vars);
  if (ordering) std::copy(ordering, ordering + desc->n_vars, ord.begin());
  else st = gsx_compute_ordering(h, GSX_ORDER_MINDEGREE, ord.data());
  if (st == GSX_OK) st = gsx_set_ordering(h, ord.data(), desc->n_vars);
  std::vector<double> zeros(h->P.state_size, 0.0);
  if (st == GSX_OK) st = set_values_unchecked(h, zeros.data(), h->P.state_size);
  if (st == GSX_OK) st = gsx_linearize(h);
  if (st == GSX_OK) st = gsx_solve(h, 0.0, 0, 0, 0, delta_out, n, bad_key);
  gsx_destroy(h);
  return st;
}

gsx_status gsx_cholesky_partial(double* abc, int32_t n, int32_t nfrontal, int32_t device, int32_t* ok) {
  if (!abc || n <= 0 || nfrontal < 0 || nfrontal > n || !ok) return GSX_E_INVALID;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 || device >= nd || hipSetDevice(device) != hipSuccess)
    return GSX_E_NO_DEVICE;
  *ok = 1;
  if (nfrontal == 0) return GSX_OK;
  // lower (ours) = transpose of upper (reference)
  std::vector<double> a((size_t)n * n);
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) a[(size_t)c * n + r] = (r >= c) ? abc[(size_t)r * n + c] : 0.0;
  double* d = nullptr;
  DevStatus* ds = nullptr;
  hipStream_t st;
  if (hipStreamCreate(&st) != hipSuccess) return GSX_E_NO_DEVICE;
  if (hipMalloc((void**)&d, a.size() * sizeof(double)) != hipSuccess) return GSX_E_NOMEM;
  hipMalloc((void**)&ds, sizeof(DevStatus));
  DevStatus init{0, INT_MAX, 0, 0};
  hipMemcpyAsync(ds, &init, sizeof(init), hipMemcpyHostToDevice, st);
  hipMemcpyAsync(d, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice, st);
  launch_dense_partial(d, n, nfrontal, ds, st);
  hipMemcpyAsync(a.data(), d, a.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(&init, ds, sizeof(init), hipMemcpyDeviceToHost, st);
  hipError_t e = hipStreamSynchronize(st);
  hipFree(d);
  hipFree(ds);
  hipStreamDestroy(st);
  if (e != hipSuccess) return GSX_E_NO_DEVICE;
  *ok = init.n_fail == 0 ? 1 : 0;
  for (int c = 0; c < n; ++c)
    for (int r = 0; r <= c; ++r) abc[(size_t)c * n + r] = a[(size_t)r * n + c];
  return GSX_OK;
}
gsx_status gsx_set_block_jacobians(gsx_handle h, int32_t first_factor, int32_t n_factors, const double* values,
                                   int64_t n_values) {
  GSX_GUARD(h, gsx_set_block_jacobians_impl(h, first_factor, n_factors, values, n_values));
}
gsx_status gsx_marginal_covariances(gsx_handle h, const uint64_t* keys, int32_t n_keys, double* out, int64_t n_out) {
  GSX_GUARD(h, gsx_marginal_covariances_impl(h, keys, n_keys, out, n_out));
}
gsx_status gsx_get_conditional(gsx_handle h, int32_t front, int32_t* n_frontal, int32_t* n_cols, double* out,
                               int64_t n_out) {
  GSX_GUARD(h, gsx_get_conditional_impl(h, front, n_frontal, n_cols, out, n_out));
}

gsx_status gsx_get_stats(gsx_handle h, gsx_stats* out) {
  if (!h || !out) return GSX_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  if (h->has_symbolic) {
    const Symbolic& S = h->S;
    out->n_fronts = S.n_fronts;
    out->n_levels = S.n_levels;
    out->max_front_dim = S.max_F;
    out->max_front_rows = S.max_rows;
    out->n_small_fronts = S.n_small;
    out->n_big_fronts = S.n_big;
    out->n_upper_levels = S.n_ulevels;
    out->n_medium_fronts = 0;
    for (int f = 0; f < S.n_fronts; ++f) {
      out->n_medium_fronts += S.med[f] && S.cls[f] == 1;
      out->n_tree_fronts += S.tree_tier[f] >= 0;
    }
    out->n_constrained_fronts = (int64_t)S.con_fronts.size();
    out->factor_flops = S.flops;
    out->front_bytes = S.front_bytes;
    out->lpanel_bytes = S.lpanel_bytes;
    out->hessian_bytes = 8.0 * (double)S.h_size;
  }
  out->n_constraint_rows = (int64_t)h->P.con_factor.size();
  out->jacobian_bytes = 8.0 * (double)h->P.jac_size;
  out->total_dim = (double)h->P.tan_size;
  if (h->has_device) {
    hipSetDevice(h->device);
    timers_resolve(h);
  }
  out->ms_linearize = h->timers[PH_LINEARIZE].ms;
  out->ms_assemble_hessian = h->timers[PH_ASSEMBLE_H].ms;
  out->ms_factorize = h->timers[PH_FACTORIZE].ms;
  out->ms_backsolve = h->timers[PH_BACKSOLVE].ms;
  out->ms_linear_error = h->timers[PH_LINERR].ms;
  out->ms_retract = h->timers[PH_RETRACT].ms;
  out->ms_error = h->timers[PH_ERROR].ms;
  out->n_linearize = h->timers[PH_LINEARIZE].count;
  out->n_factorize = h->timers[PH_FACTORIZE].count;
  out->n_backsolve = h->timers[PH_BACKSOLVE].count;
  out->n_error = h->timers[PH_ERROR].count;
  out->n_cheirality = h->n_cheirality;
  out->n_pcg_iterations = h->pcg_iterations;
  out->n_pcg_solves = h->pcg_solves;
  if (h->has_device && h->n_smart) {   // (the stream is idle: timers_resolve above waited for it)
    int cnt[2] = {0, 0};
    if (hipMemcpy(cnt, h->d_smart_counters.p, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess) {
      out->n_smart_invalid = cnt[0];
      out->n_smart_retriangulated = cnt[1];
    }
  }
  out->amalgamation_relax = h->S.relax;
  out->amalgamation_max_frontal_dim = h->S.relax_max_f;
  return GSX_OK;
}

gsx_status gsx_smart_points(gsx_handle h, double* points_out, int32_t* status_out, int64_t n) {
  if (!h || n != h->n_smart) return GSX_E_INVALID;
  if (n == 0) return GSX_OK;
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  hipSetDevice(h->device);
  if (points_out)
    HIPCHK(h, hipMemcpyAsync(points_out, h->d_smart_point.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (status_out)
    HIPCHK(h, hipMemcpyAsync(status_out, h->d_smart_status.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GSX_OK;
}

gsx_status gsx_reset_stats(gsx_handle h) {
  if (!h) return GSX_E_INVALID;
  if (h->has_device) {
    hipSetDevice(h->device);
    timers_resolve(h);
  }
  for (auto& t : h->timers) {
    t.ms = 0;
    t.count = 0;
  }
  h->pcg_iterations = h->pcg_solves = 0;
  return GSX_OK;
}

gsx_status gsx_synchronize(gsx_handle h) {
  if (!h) return GSX_E_INVALID;
  gsx_status st = need_device(h);
  if (st != GSX_OK) return st;
  hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GSX_OK;
}

gsx_status gsx_set_profiling(gsx_handle h, int32_t level) {
  if (!h) return GSX_E_INVALID;
  h->profiling = level;
  return GSX_OK;
}

gsx_status gsx_kernel_time(gsx_handle h, const char* name, double* avg_ms, int64_t* launches) {
  if (!h || !name || !avg_ms) return GSX_E_INVALID;
  if (h->has_device) {
    hipSetDevice(h->device);
    timers_resolve(h);
  }
  for (int ph = 0; ph < PH_COUNT; ++ph)
    if (std::strcmp(name, kPhaseNames[ph]) == 0) {
      *avg_ms = h->timers[ph].count ? h->timers[ph].ms / (double)h->timers[ph].count : 0.0;
      if (launches) *launches = h->timers[ph].count;
      return GSX_OK;
    }
  return GSX_E_INVALID;
}

}  // extern "C"

// ---- seams of initialize.hip (gsx_internal.h) --------------------------------------------------------------------------
namespace gsx {
double* handle_jacobian_pool(gsx_context* h) { return h->d_jac.p; }
double* handle_values(gsx_context* h) { return h->d_values.p; }
double* handle_delta(gsx_context* h) { return h->d_delta.p; }
void* handle_stream(gsx_context* h) { return (void*)h->stream; }
const HostProblem& handle_problem(gsx_context* h) { return h->P; }
void handle_blocks_written(gsx_context* h) {
  h->blocks_written(false);
  h->linear_graph_given();
}
void handle_values_written(gsx_context* h) { h->values_written(); }
}  // namespace gsx
