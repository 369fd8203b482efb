// handle.h — the solver handle (gsx_context): its device tables and buffers, and the one owner of its validity flags.
// Private to the library's host code that works on a handle; initialize.hip and lago.hip go through the seams of
// gsx_internal.h instead.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gsx_internal.h"
#include "kernels.h"

#define HIPCHK(ctx, expr)                                                                  \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess) {                                                               \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                     \
      return GSX_E_NO_DEVICE;                                                              \
    }                                                                                      \
  } while (0)

namespace gsx {

template <class Tp>
struct DevBuf {
  Tp* p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    return hipMalloc((void**)&p, count * sizeof(Tp));
  }
  hipError_t upload(const std::vector<Tp>& v, hipStream_t st) {
    hipError_t e = alloc(v.size() ? v.size() : 1);
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(p, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice, st);
  }
  // reuse the allocation when it is large enough (scratch tables rebuilt at every call)
  hipError_t stage(const std::vector<Tp>& v, hipStream_t st) {
    if (v.size() > n || !p) {
      hipError_t e = alloc(std::max<size_t>(std::max<size_t>(v.size(), 2 * n), 64));
      if (e != hipSuccess) return e;
    }
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(p, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice, st);
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

struct SmallLaunch {
  int begin, count, max_n, threads;
  int max_panel = 0;  // leaf launches: largest n*F of the group (LDS doubles)
  int max_F = 0;      // rest launches: largest frontal dimension
  bool medium = false;  // MEDIUM fronts (gsx_internal.h): front_medium_kernel, max_panel = largest n*F
};
struct BigLevel {
  int begin = 0, count = 0;
  BigPlan plan;  // rounds of the level's blocked fronts (bigfront.hip)
};
// One launch of the back-substitution (upload.hip: plan_backsolve makes them, solver.hip: run_bs_launch runs them).
enum BsKind {
  BS_BIG,      // blocked fronts whose L11 tiles fit in LDS: backsolve_big_kernel
  BS_SMALL,    // LDS-class fronts of at most 64 frontal columns: backsolve_small_kernel, or small2 when max_F > 32
  BS_GENERIC,  // backsolve_kernel with `threads` threads a front: what the two above refuse
  BS_LEAF,     // all leaf-kernel cliques of the level (the handle's leaf tables say how: leaf_bs_n, leaf_max_F)
  BS_TREE      // the tree fronts of all levels in one dependency-driven launch (the handle's bst_* tables)
};
struct BsLaunch {
  BsKind kind;
  int level;
  int begin, count;  // range of the schedule the plan is over (S.sched or S.usched; BS_LEAF: of S.sched; BS_TREE: the number of tree fronts)
  int max_n, max_F;  // largest rows / frontal columns in the range
  int threads;       // BS_GENERIC: 64, 256 or 1024; the other kernels have a block size of their own (0)
};

enum Phase { PH_LINEARIZE, PH_ASSEMBLE_H, PH_FACTORIZE, PH_BACKSOLVE, PH_LINERR, PH_RETRACT, PH_ERROR,
             PH_FACTOR_SMALL, PH_FACTOR_BIG, PH_FACTOR_LEAF, PH_K_SYRK, PH_K_TRSM, PH_K_POTRF0, PH_K_GATHER,
             PH_K_BACKSOLVE, PH_MARGINALS, PH_M_PREP, PH_M_KT, PH_M_SF, PH_M_FF, PH_M_EMIT, PH_M_LEAF, PH_COUNT };

struct Timer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, pool;
  double ms = 0;
  int64_t count = 0;
};

}  // namespace gsx

namespace gsx {

// the handle's members; gsx_context (below) is this struct under the name of the C ABI
struct Context {
  std::string err;
  int device = 0;
  bool has_device = false;
  hipStream_t stream = nullptr;
  HostProblem P;
  ScheduleOptions opt;   // the schedule switches, read by gsx_create and kept for the handle's life
  Symbolic S;
  bool has_symbolic = false;
  double relax = GSX_AMALGAMATION_AUTO;  // relaxed amalgamation (gsx_set_amalgamation); 0 = the reference's cliques, < 0 = the library's choice
  int relax_max_f = 128;
  std::vector<int> order;

  // device problem
  DevBuf<int> d_var_type, d_var_dim, d_var_state_off, d_var_tan_off, d_f_type, d_f_rows, d_f_key_ptr, d_f_vars,
      d_f_noise_kind, d_f_cols;
  DevBuf<i64> d_f_meas_off, d_f_noise_off, d_f_jac_off;
  DevBuf<double> d_meas, d_noise;
  DevBuf<FactorRec> d_frec;
  DevBuf<int> d_type_list[kNumTypeLists];
  int type_count[kNumTypeLists] = {};
  DevProblem DP{};
  // smart projection factors (kernels.h: SmartDev; smart.hip): the cameras of the call in progress and the
  // re-triangulation cache, per smart factor in graph order.  Made — with an empty cache — by upload_problem, that is at
  // gsx_create and gsx_update.
  int n_smart = 0;   // (counted on the host: known without a device)
  DevBuf<int> d_smart_slot, d_smart_status, d_smart_counters;
  DevBuf<double> d_smart_cams, d_smart_cache, d_smart_point;
  SmartDev SD{};
  // counters of a call that evaluates the smart factors: [0] is the linearize's, [1] every call's
  void smart_begin(bool linearize) {
    if (n_smart) hipMemsetAsync(d_smart_counters.p + (linearize ? 0 : 1), 0, (linearize ? 2 : 1) * sizeof(int), stream);
  }
  // device symbolic
  DevBuf<i64> d_fr_off, d_cmap_ptr, d_gidx_ptr, d_h_off, d_hmap_ptr, d_term_ptr;
  DevBuf<TermRec> d_terms;
  DevBuf<VarRec> d_var_recs;
  DevBuf<ChildRec> d_child_recs;
  DevBuf<FrontRec> d_front_recs;
  DevBuf<i64> d_cond_last, d_cond_prev;   // conditioning test per reference clique (Symbolic::cond_*)
  DevBuf<int> d_cond_front;
  DevBuf<VarRec> d_fvar_recs;
  DevBuf<LeafRec> d_leaf_recs;   // leaf-kernel cliques of level 0, in schedule order
  int leaf_base = 0;             // schedule position of d_leaf_recs[0]
  // The back-substitution solves narrow leaf cliques several to a wave (kernels.hip: backsolve_leaf_packed): its own copy
  // of d_leaf_recs, partitioned into the 16-lane, 32-lane and wave classes with the order inside a class kept
  // (leaf_bs_n: their sizes; all 0: no clique shares a wave and d_leaf_recs serves).  ScheduleOptions::bs_leaf_pack off:
  // a wave per clique.
  DevBuf<LeafRec> d_leaf_bs_recs;
  int leaf_bs_n[3] = {0, 0, 0};
  int lin_err_slice = 0;         // LDS doubles per wave of the staged linear-error kernel (0: blocks too large, direct kernel)
  DevBuf<int> d_fr_N, d_fr_F, d_fr_nfv, d_fr_fvar_ptr, d_fvars, d_fr_parent, d_fr_lean, d_fr_child_ptr, d_children, d_cmap,
      d_gidx, d_h_rows, d_hmap, d_h_loc, d_sched, d_hvars;
  DevBuf<BigDesc> d_big;
  DevSymbolic DS{};
  // schedule
  std::vector<std::vector<SmallLaunch>> small_launch;  // per level
  std::vector<std::vector<SmallLaunch>> leaf_launch;   // per level (panel-only leaf kernel)
  std::vector<int> leaf_max_F;                         // per level: largest F among its leaf-kernel fronts
  // the full factorization runs the tree fronts (Symbolic::tree_*) in one launch per tier and only the other LDS-class
  // fronts level by level (rest_launch: ranges of d_rest_ids); small_launch keeps ALL of them for the filtered plans of
  // gsx_relinearize_partial
  std::vector<std::vector<SmallLaunch>> rest_launch;
  DevBuf<int> d_usched, d_rest_ids, d_tree_start, d_tree_up, d_tree_npend, d_tree_pending, d_tree_cursor;
  // back-substitution of the tree fronts in one launch (bigfront.hip: backsolve_tree_kernel)
  DevBuf<int> d_bst_roots, d_bst_child_ptr, d_bst_children, d_bst_counters;
  DevBuf<unsigned long long> d_bst_ready;
  int bst_roots = 0, bst_total = 0;
  unsigned bst_epoch = 0;
  struct TreeTier {
    int start0, nstart, max_n, threads;
    size_t med_lds;   // > 0: the tier of the medium fronts (front_tree_med_kernel), bytes of LDS
  };
  std::vector<TreeTier> tree_tiers;
  // the back-substitution's launches (plan_backsolve).  bs_level_plan: every front level by level, top-down, over d_sched —
  // the wildfire pass and a handle with ScheduleOptions::bs_tree off.  bs_plan: the upper levels top-down over d_usched, the tree launch, the leaves.
  std::vector<BsLaunch> bs_level_plan, bs_plan;
  DevBuf<i64> d_gt_dst;  // gather tasks / segments for big parents
  DevBuf<GatherSeg> d_gsegs;
  DevBuf<GatherSrc> d_gsrcs;
  DevBuf<int> d_gt_ld, d_gt_dims, d_gm_task, d_gm_slot, d_gm_nslots;
  DevBuf<double> d_gscratch;
  GatherArgs GA{};
  std::vector<BigLevel> big_level;
  // hard constraints (Symbolic::con_*, constraint.hip): descs in (upper level, front) order
  struct ConLevel {
    int first = 0, count = 0, max_n = 0;
  };
  std::vector<ConLevel> con_level;      // per upper level
  std::vector<int> con_desc_of_front;   // front -> its record, -1
  DevBuf<ConDesc> d_con_descs;
  DevBuf<int> d_con_own_col_ptr, d_con_own_cols, d_con_own_m, d_con_child, d_con_fwd_map, d_con_iwork;
  DevBuf<i64> d_con_own_jac;
  DevBuf<double> d_con_work;
  ConTables CT{};
  // the constraint rows' entries by tangent scalar (constraint_hdiag_kernel): built with the problem tables
  int con_hd_n = 0;
  DevBuf<int> d_con_hd_tan, d_con_hd_ptr;
  DevBuf<i64> d_con_hd_jidx;
  DevBuf<double> d_con_hd_w;
  bool constrained() const { return !S.con_fronts.empty(); }
  std::vector<BigDesc> big_descs;
  int big_max_n = 0, big_max_nfv = 0;
  struct HGroup {
    int begin, count, threads, lds;
    bool global;
  };
  std::vector<HGroup> hgroups;
  DevBuf<int2> d_star_bundles;   // bundles of the star group (positions relative to the group's variable list)
  std::vector<int2> h_star_bundles;   // the host's copy (gsx_get_hessian_groups)
  int n_star_bundles = 0;
  // STAR LEAVES (kernels.hip: front_star_leaf_kernel): the star variables whose clique is a lean leaf are eliminated
  // straight from [A b] by the factorization, and their H panels are not assembled — only their rhs rows are written (by
  // that kernel).  ScheduleOptions::fused_star off: the two-step path (star assembly, then front_leaf).
  bool fused_star = false;       // this tree has star leaves and the handle eliminates them fused
  // Several star leaves share a wave (kernels.h: star_leaf_pack_class): the star records of a launch group are a stable
  // partition into the cliques of 16 lanes, of 32 lanes and of a wave.  ScheduleOptions::star_leaf_pack off: a wave each.
  struct LeafSplit {
    int sbegin, scount;          // the launch group's star leaves: range of d_star_recs
    int rbegin, rcount;          // its other leaves: range of d_leaf_rest_recs
    int s16, s32;                // of scount, the leading cliques of 16 lanes and the next of 32 (the others: a wave)
  };
  std::vector<LeafSplit> leaf_split;   // per launch group of leaf_launch[0] (fused_star only)
  DevBuf<StarLeafRec> d_star_recs;
  DevBuf<int> d_star_prow;       // clique row of every partner row of every star leaf (StarLeafRec::prow_off)
  DevBuf<LeafRec> d_leaf_rest_recs;
  DevBuf<int> d_star_rest_vars;  // star variables without a star leaf: assembled as before, one wave each
  int n_star_rest = 0;
  // marginal covariances of all variables (gsx_marginal_covariances; marginals.hip): the covariance arena and the work
  // lists of the whole tree, made on first use and dropped whenever the tree changes (upload_symbolic)
  struct MargLevel {
    int begin[4], count[4];          // ranges of d_items per step: prep, kt, sf, ff
  };
  struct MargPlan {
    std::vector<MargLevel> levels;   // top level first
    DevBuf<MargItem> d_items;
    DevBuf<int2> d_emit;             // (variable, front) of the asked variables whose front owns a block
    DevBuf<int> d_leaves;            // the leaf-kernel cliques with an asked variable
    DevBuf<i64> d_out_off;
    int n_emit = 0, n_leaves = 0;
    int64_t total = 0;
    bool ready = false;
    void release() {
      levels.clear();
      d_items.release();
      d_emit.release();
      d_leaves.release();
      d_out_off.release();
      n_emit = n_leaves = 0;
      total = 0;
      ready = false;
    }
  };
  MargPlan marg_all;
  DevBuf<i64> d_marg_slot, d_marg_work;
  DevBuf<double> d_marg_cov;
  bool marg_arena = false;
  int64_t marg_cov_doubles = 0;
  void marg_release() {
    marg_all.release();
    d_marg_slot.release();
    d_marg_work.release();
    d_marg_cov.release();
    marg_arena = false;
    marg_cov_doubles = 0;
  }
  // numeric buffers
  DevBuf<double> d_values, d_trial, d_delta, d_udelta, d_jac, d_H, d_arena, d_hdiag, d_damp, d_partials, d_scalars;
  DevBuf<double> d_dlu, d_dld;  // Dogleg: steepest-descent point, dog-leg point (allocated on first use)
  DevBuf<DevStatus> d_status;
  double* h_scalars = nullptr;  // pinned
  DevStatus* h_status = nullptr;
  static constexpr int kPartials = 4096;
  // the iterative linear solver (gsx_set_linear_solver / gsx_solve_pcg; pcg.hip): the tables and vectors are made on first
  // use and dropped whenever the problem changes (upload_problem)
  int solver_kind = GSX_SOLVER_MULTIFRONTAL;
  gsx_pcg_params pcg_params{};
  PcgWork* pcg = nullptr;
  int64_t pcg_iterations = 0, pcg_solves = 0;   // since the last gsx_reset_stats
  int64_t pcg_run_iterations = 0;               // of the driver call in progress
  bool use_pcg() const { return solver_kind == GSX_SOLVER_PCG; }
  // LM state
  double lm_lambda = 0, lm_factor = 0, lm_error = 0;
  int lm_iterations = 0, lm_inner = 0;
  // stats
  Timer timers[PH_COUNT];
  int profiling = -1;  // -1: no event timers (default), 0: phase timers, 1: + every front launch (gsx_set_profiling)
  int64_t n_cheirality = 0;
  // host copies of the launch tables, for the filtered plans of gsx_relinearize_partial
  std::vector<LeafRec> h_leaf_recs;
  std::vector<GatherSeg> h_gsegs;
  std::vector<int> hv_list, hv_group_of_var, hv_pos;
  std::vector<int> fr_sched_pos, fr_group;        // front -> position in the schedule; launch group / big-desc index
  std::vector<int> fr_seg_ptr, fr_segs, seg_level; // destination front -> its gather segments; segment -> gather group
  std::vector<int> fr_gm_ptr, fr_gms, gm_level;    // ... and its multi-segment combine entries
  struct PartialScratch {                          // device tables of gsx_relinearize_partial, reused between calls
    DevBuf<int> marked, src_off, lists[kNumTypeLists], hv, ids, gm_task, gm_slot, gm_nslots;
    DevBuf<double> states;
    DevBuf<LeafRec> leaf;
    DevBuf<BigDesc> big;
    DevBuf<GatherSeg> segs;
  } ps;
  // the SIDE work of a factorization (Symbolic::side_*): a low-priority queue of its own
  hipStream_t bulk = nullptr;
  hipEvent_t bulk_go = nullptr, bulk_done = nullptr;
  size_t leaf_side_group0 = 0;   // leaf_launch[0][leaf_side_group0 ..) are the side leaves' launches
  bool bulk_pending = false;     // side work of the factorization in flight that the main queue has not waited for yet
  // sharding (gsx_set_shard)
  int shard_rank = 0, shard_world = 1;
  gsx_allreduce_fn shard_cb = nullptr;
  void* shard_user = nullptr;
  bool shard_failed = false;    // an exchange callback failed since the last readback
  unsigned sc_dirty = 0;        // scalar slots / status counters written since the last exchange (kernels.h)
  DevBuf<int> d_f_active;
  DevBuf<unsigned char> d_own_tan, d_sched_tan, d_own_state;
  DevBuf<double> d_xscal;
  std::vector<double> jac_stage;   // host staging of gsx_set_block_jacobians
  bool sharded() const { return shard_world > 1; }
  // partial ("wildfire") back-substitution (gsx_backsubstitute_wildfire): the flags wf_* below
  DevBuf<unsigned char> d_wf_replaced, d_wf_dirty, d_wf_changed;
  DevBuf<double> d_wf_old;
  DevBuf<int> d_wf_ids;
  // ==== validity flags and their transitions =======================================================================
  // What the flags say (a flag is written by the transitions below and nowhere else):
  //   values_set        d_values holds Values (gsx_set_values, a seam of the initializers, or gsx_update)
  //   values_synced     sharded: every rank holds every variable's current value (read by gsx_get_values only)
  //   linearized        d_jac holds the [A b] blocks of every factor at the current values
  //   lin0_ready        scalars[SC_LIN0_LOCAL] = 1/2 sum |b|^2 of the current [A b] blocks
  //   h_ready           d_H holds the H panels of the current [A b] blocks ...
  //   hstar_ready       ... those of the star group included (false after an assembly that left the star leaves to the
  //                     factorization: kernels.hip, front_star_leaf_kernel)
  //   hdiag_ready       d_hdiag = diag(H) of the current panels
  //   damp_ready        d_damp holds the damping weights of damp_kind (0: lambda I, 1: diag(H) clamped to damp_min/max)
  //   fact_pending      a factorization is queued whose status the host has not read yet (readback decides)
  //   fact_valid        the arena holds a SUCCESSFUL factorization, at fact_lambda, of the [A b] blocks and tree it was
  //                     made for.  It is dropped when blocks or tree change, but NOT when only the values move: every
  //                     reader but one also tests `linearized` or relinearizes first; gsx_get_conditional tests fact_valid
  //                     alone and serves the factorization of the previous linearization until LM drops it
  //   solved            d_delta holds the step of the last solve on the current linearization
  //   wf_delta_valid    d_delta holds a COMPLETE UNDAMPED solution on the current tree (what a wildfire pass starts from)
  //   wf_all_replaced   every clique was re-eliminated since that solution (host flag; else the device flags
  //                     d_wf_replaced, marked by gsx_relinearize_partial) ...
  //   wf_clear_pending  ... which are zeroed lazily: before their next use
  // Order of the transitions: values_written | trial_accepted -> blocks_written(true) -> h_assembled -> [hstar_completed]
  // -> [hdiag_extracted] -> damping_made -> factorization_queued -> delta_overwritten -> factorization_judged ->
  // step_solved | delta_outdated (+ factorization_failed).  lin0_computed may follow any blocks_written.  tree_replaced and
  // problem_replaced may come at any point and send the handle back in front of h_assembled / values_written;
  // gsx_update goes problem_replaced -> problem_uploaded -> [some_blocks_written] -> update_finished.  The partial update
  // starts from a judged undamped factorization: [states_scattered] -> some_blocks_written -> panels_reassembled ->
  // delta_outdated -> factorization_judged.  values_gathered (gsx_get_values on a sharded handle) touches nothing else.
  bool values_set = false, linearized = false, h_ready = false, hdiag_ready = false, solved = false, damp_ready = false;
  bool lin0_ready = false;
  bool fact_valid = false;
  double fact_lambda = 0.0;
  bool fact_pending = false;
  int damp_kind = -1;
  double damp_min = 0, damp_max = 0;
  bool hstar_ready = true;
  bool values_synced = true;
  bool wf_all_replaced = true, wf_clear_pending = true;
  bool wf_delta_valid = false;
  // d_values was written from outside (gsx_set_values, a seam of the initializers), every rank alike
  void values_written() {
    values_set = true;
    values_synced = true;
    linearized = h_ready = solved = false;
  }
  // gsx_relinearize_partial scattered the moved variables' states into d_values; it goes on to redo what they touch
  void states_scattered() { values_synced = true; }
  // a sharded handle gathered every variable from its owner into d_trial: that copy becomes the current one
  void values_gathered() {
    std::swap(d_values.p, d_trial.p);
    values_synced = true;
  }
  // The trial values become the current ones (gsx_retract with commit, GN, Dogleg, LM's accepted trial).  The arena is
  // not touched: GN, Dogleg and gsx_retract leave the factorization servable by gsx_get_conditional (the one reader
  // that does not ask for `linearized`); LM drops it with the values it accepted (drop_factorization).
  // (Dogleg used not to write values_synced; it refuses sharded handles, the only ones that read the flag.)
  void trial_accepted(bool drop_factorization) {
    std::swap(d_values.p, d_trial.p);
    values_synced = false;
    trial_discarded();
    if (drop_factorization) fact_valid = false;
  }
  // Dogleg's zero step: the iteration ends at the values it started from, its linearization is dropped all the same
  void trial_discarded() { linearized = h_ready = solved = false; }
  // The [A b] blocks were rewritten: by a linearization at the current values (dev_linearize), or the GSX_F_LINEAR blocks
  // by the caller (gsx_set_block_jacobians, the seam of the initializers).  (lambda I weights do not depend on the blocks:
  // kept.  A linearization leaves hdiag_ready to the assembly that has to follow it.)
  void blocks_written(bool is_linearization) {
    if (is_linearization) linearized = true;
    else hdiag_ready = false;
    h_ready = false;
    lin0_ready = false;
    fact_valid = false;
    solved = false;
    if (damp_kind != 0) damp_ready = false;
  }
  // the blocks of SOME factors were re-linearized (gsx_relinearize_partial, gsx_update): the caller redoes what they touch
  void some_blocks_written() { lin0_ready = false; }
  // a linear graph IS its linearization (gsx_solve_gfg_h, the seam of the initializers)
  void linear_graph_given() { linearized = true; }
  void lin0_computed() { lin0_ready = true; }
  // diag(H) is extracted on demand: lambda * I damping never needs it
  void h_assembled(bool star_complete) {
    h_ready = true;
    hstar_ready = star_complete;
    hdiag_ready = false;
  }
  void hstar_completed() { hstar_ready = true; }
  void hdiag_extracted() { hdiag_ready = true; }
  void panels_reassembled() { hdiag_ready = false; }   // (some of them: gsx_relinearize_partial)
  bool damping_is(int kind, double mind, double maxd) const {
    return damp_ready && damp_kind == kind && (kind == 0 || (damp_min == mind && damp_max == maxd));
  }
  void damping_made(int kind, double mind, double maxd) {
    damp_ready = true;
    damp_kind = kind;
    damp_min = mind;
    damp_max = maxd;
  }
  // a full factorization is queued: valid once the read-back shows no failed front; every clique re-eliminated
  void factorization_queued(double lambda) {
    fact_valid = false;
    fact_pending = true;
    fact_lambda = lambda;
    wf_all_replaced = true;
  }
  // the factorization in the arena is only trusted (solve at the same lambda, marginals, partial re-elimination) once its
  // status has been seen clean
  void factorization_judged(bool bad) {
    if (fact_pending) fact_valid = !bad;
    else if (bad) fact_valid = false;
    fact_pending = false;
  }
  void factorization_failed() { fact_valid = false; }
  // d_delta is being rewritten (a back-substitution, PCG): no longer the complete undamped solution a wildfire pass starts
  // from, until step_solved says so again
  void delta_overwritten() { wf_delta_valid = false; }
  // d_delta no longer matches the arena / the system (a failed solve, a re-elimination)
  void delta_outdated() { solved = false; }
  void step_solved(bool complete_undamped) {
    solved = true;
    if (complete_undamped) {
      wf_delta_valid = true;
      wf_all_replaced = false;
      wf_clear_pending = true;
    }
  }
  // a new tree: the arena and H were re-allocated for it — nothing computed for the old one may be reused
  void tree_replaced() {
    h_ready = false;
    solved = false;
    fact_valid = fact_pending = false;
    wf_all_replaced = true;
    wf_delta_valid = false;
    damp_ready = hdiag_ready = false;   // (sharded: the damping weights carry the ownership mask)
    if (sharded()) linearized = false;  // the owned factor set changed with the partition
  }
  // gsx_update switches the handle over to another graph.  From there on a failure (an allocation, a copy) leaves device
  // tables of two different graphs behind: every state flag is dropped first and set again only after the last upload, so
  // that a failed update makes every later numeric call answer GSX_E_STATE until gsx_set_values + gsx_set_ordering
  // rebuild the handle — never kernels on mismatched tables.
  void problem_replaced() {
    has_symbolic = values_set = linearized = h_ready = solved = false;
    fact_valid = fact_pending = hdiag_ready = damp_ready = lin0_ready = false;
    wf_delta_valid = false;
    wf_all_replaced = true;
  }
  void problem_uploaded() {   // (the tables of the new graph and tree are in place, and its values)
    has_symbolic = true;
    values_set = true;
    values_synced = true;
  }
  void update_finished(bool kept_linearization) { linearized = kept_linearization; }
  // (device flags per front, allocated on first use for the current tree, zeroed when a clear is pending)
  hipError_t wf_flags_ready(hipStream_t st) {
    const size_t nf = (size_t)std::max(S.n_fronts, 1);
    if (d_wf_replaced.n != nf) {
      hipError_t e = d_wf_replaced.alloc(nf);
      if (e != hipSuccess) return e;
      wf_clear_pending = true;
    }
    if (wf_clear_pending) {
      hipError_t e = hipMemsetAsync(d_wf_replaced.p, 0, nf, st);
      if (e != hipSuccess) return e;
      wf_clear_pending = false;
    }
    return hipSuccess;
  }
  // ==== end of the flags ==============================================================================================
};

// ---- what the files that work on a handle share ------------------------------------------------------------------------
// upload.hip
int factor_type_list(const HostProblem& P, int f);
// the ABS_* sub-kind of a TL_ABSOLUTE factor (kernels.h), 0 for every other factor; and a TL_ABSOLUTE list put in the order
// its kernels want: by sub-kind, graph order inside a kind
int factor_absolute_kind(const HostProblem& P, int f);
void sort_absolute_list(const HostProblem& P, std::vector<int>& list);
void whiten_linear_factor(const HostProblem& P, int f, const double* src, double* J);
gsx_status upload_problem(gsx_context* c);
gsx_status upload_symbolic(gsx_context* c);
void plan_hessian_groups(gsx_context* c);   // host only: hgroups, hv_*, h_star_bundles from the symbolic analysis
void plan_backsolve(const Symbolic& S, std::vector<BsLaunch>& level_plan, std::vector<BsLaunch>& plan);
// solver.hip: the device pipeline (all asynchronous up to readback) ...
void launch_lds_group(const DevProblem& P, const DevSymbolic& S, const int* ids, const SmallLaunch& g, const double* H,
                      const double* damp, const double* scalars, double* arena, DevStatus* status, hipStream_t st);
void timer_begin(gsx_context* c, int ph);
void timer_end(gsx_context* c, int ph);
void dev_linearize(gsx_context* c);
void dev_assemble_h(gsx_context* c);
void dev_ensure_hstar(gsx_context* c);
void dev_damping(gsx_context* c, int diagonal, double mind, double maxd);
void dev_big_factor(gsx_context* c, const BigDesc* descs, int count, const BigPlan& plan, hipStream_t st, bool prof);
void dev_backsolve(gsx_context* c, const WildfireArgs* wf = nullptr);
void dev_linear_error(gsx_context* c, bool solved_step = false);
void dev_retract(gsx_context* c, const double* d_delta);
void dev_error(gsx_context* c, const double* d_vals, int slot);
gsx_status readback(gsx_context* c);
bool factorization_ok(const gsx_context* c);
gsx_status compute_error_sync(gsx_context* c, double* out);
// ... the pieces of an entry point ...
gsx_status need_device(gsx_context* c);
gsx_status begin_call(gsx_context* c, bool need_values, bool need_symbolic);
gsx_status indeterminate(gsx_context* c, uint64_t* bad_key, bool also_nonfinite);
gsx_status download(gsx_context* c, const double* src, double* out, int64_t n);
// ... and the solve steps.  Whether a step assembles H first: never (the caller did), when the panels are stale, always
// (the caller just linearized)
enum HMode { H_KEEP, H_IF_STALE, H_ALWAYS };
void direct_solve(gsx_context* c, HMode hm, int diagonal, double mind, double maxd, double lambda, bool backsolve);
gsx_status damped_step(gsx_context* c, HMode hm, int diagonal, double mind, double maxd, double lambda);

}  // namespace gsx

struct gsx_context : gsx::Context {};

// No exception crosses the C boundary (include/gsx.h): the entry points whose work is sized by caller input (host vectors
// of the plans, staging buffers) answer an allocation failure with a status, like the readers in io.cpp.
#define GSX_GUARD(h, call)                          \
  try {                                             \
    return (call);                                  \
  } catch (const std::bad_alloc&) {                 \
    if (h) (h)->err = "out of host memory";         \
    return GSX_E_NOMEM;                             \
  } catch (const std::exception& e) {               \
    if (h) (h)->err = e.what();                     \
    return GSX_E_INVALID;                           \
  }
