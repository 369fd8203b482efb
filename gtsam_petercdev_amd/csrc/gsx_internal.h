// gsx_internal.h — host-side data structures of libgsx (product; never includes oracle/).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gsx.h"
#include "unit3_math.h"

struct gsx_context;
// what gsx_dataset_get hands out (io.cpp: the file readers; translation_graph.cpp: gsx_translation_recovery_problem)
struct gsx_dataset {
  std::vector<uint64_t> var_keys;
  std::vector<int32_t> var_types, var_dims, f_type, f_rows, f_key_ptr, f_vars, f_noise_kind;
  std::vector<int64_t> f_meas_ptr, f_noise_ptr;
  std::vector<double> meas, noise, values;
  std::string err;
};

namespace gsx {

// Size classes of fronts: S* are eliminated inside LDS by one workgroup, BIG by the blocked
// global-memory path.  n = frontal + separator + 1 (rhs) scalar rows.
constexpr int kSmallMaxN = 140;     // 140^2 * 8 B = 156.8 KB <= 160 KB LDS
constexpr int kTile = 32;           // tile edge of the blocked big-front path
constexpr int kGatherChunk = 64;    // sources per gather segment: one wave, one source record per lane
constexpr int kMaxTreeTiers = 8;    // tiers of the tree kernels, the medium tier included (one start-list cursor each)
constexpr int kLeafMaxF = 16;      // leaf cliques with at most this many frontal scalars use the panel-only kernel
constexpr int kLeafMaxPanel = 8192; // doubles of LDS (n x F) a lean leaf may use: 64 KB
// MEDIUM fronts: more rows than fit LDS as a square, but whose n x F frontal panel does.  One workgroup eliminates such a
// front with the panel in LDS and the trailing block in the arena (front_medium_body, kernels.hip); storage and class
// (cls 1) are those of an LDS front, so parents, back-substitution, marginals read them unchanged.
constexpr int kMedMaxN = 512;       // rows (two staged row maps of that many ints)
constexpr int kMedMaxPanel = 18432; // doubles of LDS for the panel: 144 KB
constexpr int kMedMaxLeafKids = 8;  // a front with more childless small children than this stays blocked: its leaves are
                                    // LEAN only under a blocked parent (every BAL camera front: hundreds of landmarks)

// The schedule switches of one handle: which kernels and what launch geometry its plans choose.  gsx_create reads them from
// the environment once (schedule_options_from_env: the only reader) and the handle keeps them — every later analysis,
// ordering and plan of that handle, gsx_update's included, takes them from there.  The defaults are what an empty
// environment gives: the measured best.
struct ScheduleOptions {
  // GSX_TREE_TIERS ("rows:threads,...", e.g. "45:128,79:256,140:512"; "0": no tiers — the tree kernels off, level launches
  // only): tier -> largest n of its fronts, workgroup size (0: the host's default for that n).
  // two tiers: fronts of at most 67 rows (four to a CU's 160 KB of LDS) and the rest.  Swept on the 100 000-pose
  // graphs (tools/sweep_tree.sh): every further tier adds its own tail — the last few chains of a launch run alone
  // on the chip — and costs more than the LDS it frees: 45/79/140 +16 %, 53/98/140 +13 %, one tier +67 %.
  std::vector<int> tree_bounds = {67, kSmallMaxN};
  std::vector<int> tree_threads = {256, 512};
  // GSX_MEDIUM set: fronts of 141-512 rows go to front_medium_body.
  // MEASURED AND SWITCHED OFF (tests/test_gpu_parity.py keeps the path honest): a medium front
  // takes ~53 us in its one workgroup (pose3_100k, mean n = 170, F = 45: children 13, panel 15, trailing update 18) and
  // the medium fronts of a pose graph form a chain a dozen deep, while the level schedule of the blocked path gives up
  // only six of its seventeen levels for them (the top fronts are wide in F): pose3_100k 2.94 -> 3.46 ms, pose2_100k
  // 1.65 -> 1.99 ms with the medium tier on.
  bool medium = false;
  bool side = true;              // GSX_SIDE_OFF set: no second queue for the side leaves
  // the side leaves are worth a second queue only when it moves real work: a tenth of the lean leaves, and thousands of them
  // (GSX_SIDE_MIN lowers the count for experiments and for tests that reach the side group on a small graph)
  int side_min = 4096;
  int nd_leaf = 0;               // GSX_ND_LEAF: leaf size of the nested dissection; 0: the ordering kind's own (ordering.cpp)
  // GSX_SMALL_THREADS_SHIFT: threads of the front_small launches as a shift of the row-per-thread count.
  // (twice the threads the row-per-thread panel needed: the assembly and the stores of a front are a handful of memory
  //  round trips that more lanes shorten, and the tile phases of the factorization split over the waves; measured -2 %
  //  on the 100 000-pose graphs, nothing beyond 2x)
  int small_threads_shift = 1;
  bool h_tile = true;            // GSX_H_TILE_OFF set: H panels by the generic kernel, not assemble_h_tile_kernel (measurements)
  bool fused_star = true;        // GSX_FUSED_STAR=0: star leaves by the two-step path (star assembly, then front_leaf)
  bool star_leaf_pack = true;    // GSX_STAR_LEAF_PACK=0: every star leaf eliminated by a wave of its own
  bool bs_leaf_pack = true;      // GSX_BS_LEAF_PACK=0: leaf back-substitution a wave per clique
  bool bs_tree = true;           // GSX_BS_TREE_OFF set: back-substitution by level launches only, no tree launch
  bool linerr_from_step = true;  // GSX_LINERR_DIRECT set: the LM trial's linearized error by direct evaluation
};
ScheduleOptions schedule_options_from_env();   // (schedule_options.cpp)

struct HostProblem {
  int n_vars = 0, n_factors = 0;
  std::vector<uint64_t> keys;
  std::vector<int> types, dims, state_off, tan_off;
  int64_t state_size = 0, tan_size = 0, jac_size = 0;
  // factors (graph order)
  std::vector<int> f_type, f_rows, f_key_ptr, f_vars, f_noise_kind;
  std::vector<int64_t> f_meas_ptr, f_noise_ptr, f_jac_off;
  std::vector<double> meas, noise;
  std::vector<int> f_cols;           // sum d + 1
  // hard-constraint rows (zero sigma), by (factor, row) in graph order, with the weight mu of the error functions; on the
  // device they are rows of sigma 1 / sqrt(mu) (problem.cpp) that the factorization eliminates by constraint pivots
  std::vector<int> con_factor, con_row;
  std::vector<double> con_mu;
  // the variables whose state holds a unit direction (GSX_VAR_UNIT3, GSX_VAR_ESSENTIAL): empty for every other graph
  std::vector<int> direction_vars;
};

// Symbolic factorization for one ordering.
struct Symbolic {
  double relax = 0.0;                // relaxed amalgamation threshold (0 = the reference's cliques)
  int relax_max_f = 128;             // ... and the largest merged frontal dimension
  int n_fronts = 0;
  std::vector<int> order;            // position -> var
  std::vector<int> pos;              // var -> position
  std::vector<int> front_of_var;     // var -> front in which it is frontal
  std::vector<int> parent;           // front -> parent front (-1 root)
  std::vector<int> fvar_ptr, fvars;  // CSR: front -> local variable list (frontals first, then separator by position)
  std::vector<int> nfrontal_vars;    // front -> number of frontal variables
  std::vector<int> F, S, N;          // frontal dim, separator dim, n = F+S+1
  std::vector<int64_t> off;          // arena offset (doubles) of the n x n column-major front
  std::vector<int> level;            // 0 = leaves
  std::vector<char> cls, lean;       // size class (0 leaf kernel, 1 small, 2 big); lean leaf (no Schur complement stored)
  std::vector<char> med;             // cls 1 with n > kSmallMaxN: a MEDIUM front (panel in LDS, trailing block in the arena)
  std::vector<int> child_ptr, children;  // CSR front -> children (in the reference's child order)
  // scalar row maps
  std::vector<int64_t> cmap_ptr;     // front -> offset in cmap of its (S+1) update-row -> parent-row map
  std::vector<int> cmap;
  std::vector<int64_t> gidx_ptr;     // front -> offset in gidx of its (F+S) row -> global tangent index map
  std::vector<int> gidx;
  // H panels (per variable, in elimination order of rows)
  std::vector<int64_t> h_off;        // var -> offset of its panel in the H pool
  std::vector<int> h_rows;           // var -> panel rows (d_A + sum later-neighbour dims + 1)
  std::vector<int64_t> hmap_ptr;     // var -> offset in hmap of panel-row -> front-row map
  std::vector<int> hmap;
  std::vector<int> h_loc;            // var -> local scalar column offset of the variable in its front
  int64_t h_size = 0, arena_size = 0;
  // H assembly term lists: per variable, terms (one per (factor, destination block))
  std::vector<int64_t> term_ptr;     // var -> range in the term arrays
  std::vector<int64_t> t_jac;        // offset of the factor's [A b]
  std::vector<int> t_m, t_colA, t_colB, t_dB, t_dst;
  // schedule: fronts sorted by (level, class); per level the ranges of each class
  std::vector<int> sched;            // front ids
  std::vector<int> lvl_ptr;          // level -> range in sched (size n_levels+1)
  std::vector<int> lvl_small_end;    // level -> end of the small (LDS) fronts inside the level range
  std::vector<int> lvl_leaf_end;     // level 0 only: end of the leaf-kernel fronts (no children, F <= kLeafMaxF)
  int n_levels = 0;
  // The UPPER schedule of the full factorization / back-substitution: the fronts that are neither tree fronts nor leaf-kernel
  // cliques (every blocked front, and the LDS fronts above one) are levelled among THEMSELVES — ulevel = longest chain of
  // upper fronts below — because everything else is finished by the leaf launches and the tree kernels before the first
  // of them starts.  (The height-from-the-leaves levels above stay the order of gsx_relinearize_partial and of the wildfire
  // pass.)  pose3_100k: 17 levels with blocked fronts by height, 11 by ulevel.
  std::vector<int> ulevel;           // front -> upper level, -1: not an upper front
  std::vector<int> usched;           // upper fronts by (ulevel, LDS-class before blocked, n)
  std::vector<int> ulvl_ptr;         // ulevel -> range in usched (size n_ulevels + 1)
  std::vector<int> ulvl_small_end;   // ulevel -> end of the LDS-class fronts inside the range
  int n_ulevels = 0;
  int cap_ulevel0 = -1;              // first upper level of the cap, -1: no cap
  // SIDE work: lean leaves whose (blocked) parent sits above the first blocked level are needed late — their leaf
  // factorization and their product-form gather (gather group `n_levels`, scratch slots from side_slot0) run on a second,
  // low-priority queue beside the blocked chain of the lower levels; the main queue waits for them before level
  // side_level0 + 1.  side_level0 < 0: none.
  int side_level0 = -1;              // the first UPPER level with blocked fronts
  int leaf_side_begin = 0;           // position in sched where the side leaves of level 0 start (== lvl_leaf_end[0]: none)
  int side_slot0 = 0;                // first scratch slot of the side gather group
  std::vector<char> side;            // front -> side leaf
  // Subtree-fused elimination of the LDS-class fronts (front_tree_kernel): a front is a TREE front when it is LDS-class and
  // so is its whole subtree (leaf-kernel children aside).  Tree fronts are cut into tiers by the largest front of their
  // subtree (= the LDS a workgroup needs to climb it); one launch per tier, inside which a workgroup that finishes a front
  // takes the parent when it was the last child to arrive (ClusterTree-inst.h:219-318 post-order, without level barriers).
  std::vector<int> tree_bounds;      // tier -> largest n of its fronts
  std::vector<int> tree_threads;     // tier -> workgroup size (0: the host's default for that n)
  std::vector<int> tree_tier;        // front -> tier, -1: not a tree front
  std::vector<int> tree_up;          // front -> parent when that is a tree front of the same tier, else -1
  std::vector<int> tree_npend;       // front -> children that are tree fronts of the same tier
  std::vector<int> tree_start;       // per tier (tree_start_ptr): the fronts with tree_npend == 0, in schedule order
  std::vector<int> tree_start_ptr;
  // deterministic extend-add into BIG parents: one task per destination block (parent var pair),
  // with the list of source blocks (child Schur-complement blocks) in child order
  std::vector<int64_t> gt_dst;       // task -> arena offset of the destination block (top-left entry)
  std::vector<int> gt_ld, gt_dims;   // destination leading dimension; dB | dA << 8 | diag << 16
  std::vector<int64_t> gt_ptr;       // task -> range in the source arrays (size n_tasks + 1)
  std::vector<int> gs_child, gs_loc; // source: child front id, offset of the block inside the child's front
  std::vector<int> gs_loc2;          // lean child: row of the second factor in its L panel (gs_loc = row of the first); else -1
  std::vector<int> gt_lvl_ptr;       // upper level of the PARENT -> task range (size n_ulevels + 2: the side group last)
  // segments of the source lists (one wave each) and the multi-segment tasks that need a combine pass
  std::vector<int> gseg_task, gseg_slot;          // segment -> task, scratch slot (-1: adds straight to dst)
  std::vector<int64_t> gseg_begin, gseg_end;      // segment -> source range
  std::vector<int> gseg_lvl_ptr;                  // upper level -> segment range (size n_ulevels + 2: the side group last)
  std::vector<int> gm_task, gm_slot, gm_nslots;   // multi-segment task -> first slot, number of slots
  std::vector<int> gm_lvl_ptr;                    // upper level -> multi-task range (size n_ulevels + 2)
  int g_max_slots = 0;                            // scratch slots needed (x 128 doubles), reused per level
  // choleskyPartial's conditioning test per REFERENCE clique: arena offsets of the last / second-to-last (-1: single pivot)
  // diagonal entries of L, and the front that holds them (only the fronts this rank factors)
  std::vector<int64_t> cond_last, cond_prev;
  std::vector<int> cond_front;
  // for partial re-elimination (gsx_relinearize_partial): variable -> factors CSR, gather task -> destination front
  std::vector<int> vf_ptr, vf;
  std::vector<int> gt_front;
  // HARD CONSTRAINTS (HostProblem::con_*; EliminatePreferCholesky -> EliminateQR, HessianFactor.cpp:538-551,
  // Constrained::QR, NoiseModel.cpp:503-620).  A constraint row lives in the front where the first-eliminated variable of
  // its factor is frontal; there it is used as a PIVOT (one frontal scalar expressed by the others — no Cholesky step for
  // it), or, when the front has fewer frontal scalars than rows, handed to the parent.  A front that takes rows in is
  // always BLOCKED (cls 2): its assembled panel is in the arena, where the constraint kernels rewrite it into an
  // unconstrained front with equivalent conditionals and the same Schur complement (constraint.hip).
  std::vector<char> con;               // front -> takes constraint rows in
  std::vector<int> con_fronts;         // those fronts, children before parents
  std::vector<int> con_index;          // front -> index in con_fronts, -1
  std::vector<int> con_in, con_fwd;    // per constrained front: rows in (own + the children's), rows handed to the parent
  std::vector<int> con_own_ptr;        // constrained front -> its own rows (CSR into con_own_*)
  std::vector<int64_t> con_own_jac;    // own row -> offset of its first entry in the Jacobian store ([A b] + row)
  std::vector<int> con_own_m;          // ... rows of its factor (the column stride)
  std::vector<int> con_own_col_ptr;    // own row -> range in con_own_cols (size + 1)
  std::vector<int> con_own_cols;       // per column of the factor's [A b]: the front's row (n - 1: the rhs)
  std::vector<int> con_child_ptr, con_child;  // constrained front -> the constrained fronts below it whose leftover rows arrive here
  std::vector<int> con_fwd_map_ptr, con_fwd_map;  // constrained front -> per separator + rhs row: the row of the front its
                                                  // leftover rows go to (-1: a variable none of them holds)
  // sharding of ONE problem over the GPUs of a node (gsx_set_shard): the fronts whose subtree is cheaper than a share of
  // the whole tree form independent subtrees dealt to the ranks; the rest — the top of the tree, the "cap" — is
  // assembled from every rank's contributions with one all-reduce and factored by all ranks alike.
  int shard_rank = 0, shard_world = 1;
  std::vector<int> owner;            // front -> owning rank, -1 = cap (all ranks); all 0 when not sharded
  std::vector<char> scheduled;       // front -> this rank processes it (owner == rank or cap)
  std::vector<char> f_owned;         // factor -> this rank linearizes it and adds its J'J terms
  int cap_level0 = -1;               // first level of the cap (every cap front is at or above it), -1: no cap
  int64_t cap_begin = 0, cap_end = 0;  // the cap fronts' contiguous share of the arena (doubles)
  int n_cap = 0;
  double cap_cost = 0, own_cost = 0, total_cost = 0;  // flop estimates: cap, this rank's subtrees, whole tree
  // stats
  double flops = 0, front_bytes = 0, lpanel_bytes = 0;
  int64_t max_F = 0, max_rows = 0, n_small = 0, n_big = 0, n_medium = 0;
};

// a variable whose state holds a unit direction: its type's name, and whether the direction in `state` is of unit length
// (unit3_math.h: to 1e-9).  The one place that knows where the direction sits
inline bool is_direction_type(int t) { return t == GSX_VAR_UNIT3 || t == GSX_VAR_ESSENTIAL; }
inline const char* direction_type_name(int t) { return t == GSX_VAR_UNIT3 ? "GSX_VAR_UNIT3" : "GSX_VAR_ESSENTIAL"; }
inline bool direction_state_ok(int t, const double* state) { return unit3_is_unit(state + (t == GSX_VAR_ESSENTIAL ? 9 : 0)); }

// The refusal line of a call that has no handle (the writers, the initializers, triangulation): gsx_last_error(NULL)
// returns the calling thread's last one.
inline std::string& call_error() {
  static thread_local std::string e;
  return e;
}
// those calls read states by their own rules and know no Rot3, Unit3 or EssentialMatrix: a description that holds a variable
// of one of these types is refused by name
inline gsx_status refuse_manifold_only_vars(const gsx_problem_desc* d, const char* who) {
  if (d && d->var_types)
    for (int v = 0; v < d->n_vars; ++v) {
      const int t = d->var_types[v];
      if (t == GSX_VAR_ROT3 || is_direction_type(t)) {
        call_error() = std::string(who) + ": variable " + std::to_string(v) + " (key " +
                       std::to_string(d->var_keys ? (unsigned long long)d->var_keys[v] : 0ull) + ") is a " +
                       (t == GSX_VAR_ROT3 ? "GSX_VAR_ROT3" : direction_type_name(t));
        return GSX_E_INVALID;
      }
    }
  return GSX_OK;
}

// entry of a handle-less call that takes a description: the line of an earlier refusal goes, a Rot3, Unit3 or
// EssentialMatrix variable is refused by name
inline gsx_status enter_call(const gsx_problem_desc* d, const char* who) {
  call_error().clear();
  return refuse_manifold_only_vars(d, who);
}

// host algorithms
gsx_status lower_problem(const gsx_problem_desc* d, HostProblem& P, std::string& err);
// the directions of the packed states `values` are of unit length (to the 1e-9 of unit3_math.h); the first that is not is
// named in err.  Nothing is normalised silently
gsx_status check_direction_states(const HostProblem& P, const double* values, std::string& err);
void compute_ordering(const HostProblem& P, int kind, const ScheduleOptions& opt, std::vector<int>& order);
// multilevel nested dissection of the vertices `verts` of the graph `adj` (nd.cpp); sets of at most `leaf` vertices and
// the separators are ordered by `leaf_order` (appends to `out`)
typedef void (*NdLeafOrder)(const std::vector<std::vector<int>>& adj, const std::vector<int>& w,
                            const std::vector<int>& verts, std::vector<int>& out);
void multilevel_nested_dissection(const std::vector<std::vector<int>>& adj, const std::vector<int>& w,
                                  const std::vector<int>& verts, int leaf, NdLeafOrder leaf_order, std::vector<int>& out);
gsx_status symbolic_analysis(const HostProblem& P, const std::vector<int>& order, double relax, int relax_max_f,
                             int shard_rank, int shard_world, const ScheduleOptions& opt, Symbolic& S, std::string& err);

// ---- Pose3 initialization (init_graph.cpp: host lowering; initialize.hip: device work) ----------------------------------
// The pose graph of initialize::buildPoseGraph<Pose3> (gtsam/slam/InitializePose.h:36-52) over the POSE3 variables of a
// description: node = rank of the variable among the description's POSE3 variables, the anchor (key 99999999) last.
constexpr uint64_t kAnchorKey = 99999999;
struct PoseGraph {
  int n_poses = 0;                   // POSE3 variables of the description; the anchor is node n_poses
  std::vector<int> pose_var;         // node -> variable index in the description
  std::vector<int> node_of_var;      // variable -> node, -1: not a POSE3 variable
  std::vector<char> touched;         // node -> some used factor holds it
  bool all_touched = true;           // every POSE3 variable is held by a used factor
  // edges in factor order (a prior is an edge from the anchor)
  std::vector<int> from, to, factor;
  std::vector<double> rot;           // 9 per edge: measured rotation, row-major
  std::vector<double> weight;        // the rotation "precision": first entry of whiten(e0) (InitializePose3.cpp:48-51)
  std::vector<int> adj_ptr, adj;     // node -> incident edges in factor order (createSymbolicGraph, :221-253)
  bool anchored = true;              // every touched node is joined to the anchor by edges of non-zero weight
};
gsx_status build_pose_graph(const gsx_problem_desc* d, PoseGraph& G, std::string& err);
// an owned gsx_problem_desc
struct OwnedDesc {
  std::vector<uint64_t> keys;
  std::vector<int32_t> types, dims, f_type, f_rows, f_key_ptr, f_vars, f_noise_kind;
  std::vector<int64_t> f_meas_ptr, f_noise_ptr;
  std::vector<double> meas, noise;
  gsx_problem_desc view() const;
};
// The decoupled relaxed system (InitializePose3.cpp:37-71, one of its three identical 3-dimensional parts): variables =
// touched nodes and the anchor as VECTOR(3) in ascending key order; one 3 x 7 GSX_F_LINEAR block per edge of non-zero
// weight (zeros here: chordal_blocks_kernel writes them), then the anchor row [I | e_1].  var_of_node: node -> variable
// of the internal description (-1: untouched); edges: the pose-graph edges that got a block, in order.
void lower_relaxed(const gsx_problem_desc* d, const PoseGraph& G, OwnedDesc& out, std::vector<int>& var_of_node,
                   std::vector<int>& edges);
// The graph of initialize::computePoses<Pose3> (InitializePose.h:57-97): the touched poses and the anchor as POSE3
// variables, the pose-graph edges of non-zero weight as between factors with their own noise, a Unit prior on the anchor.
void lower_anchor_graph(const gsx_problem_desc* d, const PoseGraph& G, OwnedDesc& out, std::vector<int>& var_of_node);

// ---- Pose2 initialization: lago (lago_graph.cpp: host lowering and trees; lago.hip: device work) --------------------------
// The pose graph of initialize::buildPoseGraph<Pose2> (gtsam/slam/InitializePose.h:36-52) over the POSE2 variables of a
// description, the spanning tree of lago::findOdometricPath / findMinimumSpanningTree (gtsam/slam/lago.cpp:202-260) and
// the tree / chord split of lago::getSymbolicGraph (:101-138).  node = rank of the variable among the description's POSE2
// variables, the anchor (kAnchorKey) last.
struct LagoGraph {
  int n_poses = 0;                   // POSE2 variables of the description; the anchor is node n_poses
  std::vector<int> pose_var;         // node -> variable index in the description
  std::vector<int> node_of_var;      // variable -> node, -1: not a POSE2 variable
  std::vector<uint64_t> key;         // node -> key (the anchor's last)
  std::vector<char> touched;         // node -> some used factor holds it
  bool all_touched = true;           // every POSE2 variable is held by a used factor
  // edges in factor order (a prior is an edge from the anchor): the reference's pose2Graph
  std::vector<int> from, to, factor;
  std::vector<double> meas;          // 3 per edge: dx, dy, measured().theta()
  std::vector<double> sigma;         // 3 per edge: the sigmas of its Diagonal model
  // the tree (lago_tree)
  std::vector<int> parent;           // node -> parent node; the anchor: itself; -1: no entry in the PredecessorMap
  std::vector<double> delta;         // node -> signed deltaTheta of the edge parent -> node (deltaThetaMap), 0 without one
  std::vector<int> tree_ids, chord_ids;  // edges, each list in factor order (spanningTreeIds, chordsIds)
  std::vector<char> is_chord;        // edge -> chord
  int max_depth = 0;                 // edges on the longest path from a node to the anchor
  bool anchored = true;              // false: the node the odometric path attaches to the anchor carries no prior
};
// GSX_E_INVALID: malformed description, anchor-key collision, a Gaussian or robust model or a sigma that is not positive on
// a used factor
gsx_status build_lago_graph(const gsx_problem_desc* d, LagoGraph& G, std::string& err);
// GSX_E_INVALID where the reference's tree.at(key) throws
gsx_status lago_tree(LagoGraph& G, bool use_odometric_path, std::string& err);
// The orientation system of buildLinearOrientationGraph (:165-199) with theta_anchor = 0 substituted: the touched poses as
// VECTOR(1) variables in key order; per edge one 1 x 3 GSX_F_LINEAR block, or 1 x 2 for an edge from the anchor (zeros
// here: lago_orientation_blocks_kernel writes them).  var_of_node: node -> variable (-1: untouched or the anchor).
void lower_lago_orientations(const gsx_problem_desc* d, const LagoGraph& G, OwnedDesc& out, std::vector<int>& var_of_node);
// The pose system of computePoses (:308-356): the touched poses and the anchor as VECTOR(3) variables in key order; one
// 3 x 7 block per edge (zeros here: lago_pose_blocks_kernel writes them), then the anchor's prior, whitened by
// Variances(1e-6, 1e-6, 1e-8).
void lower_lago_poses(const gsx_problem_desc* d, const LagoGraph& G, OwnedDesc& out, std::vector<int>& var_of_node);
// depth of every node of a forest given by parent links (root: parent[i] == i); false: an index out of range or a cycle
bool forest_depths(const int32_t* parent, int64_t n, std::vector<int>& depth, int* max_depth);

// seams of initialize.hip and lago.hip into a handle (solver.hip; the handle itself is handle.h); the pointers are device memory on the handle's device
double* handle_jacobian_pool(gsx_context* h);   // the [A b] blocks, factor f at HostProblem::f_jac_off[f]
double* handle_values(gsx_context* h);          // packed Values
double* handle_delta(gsx_context* h);           // the solution of the last solve, tangent order
void* handle_stream(gsx_context* h);            // hipStream_t
const HostProblem& handle_problem(gsx_context* h);
void handle_blocks_written(gsx_context* h);     // the GSX_F_LINEAR blocks were rewritten on the device: what gsx_set_block_jacobians invalidates
void handle_values_written(gsx_context* h);     // the Values were written on the device: as after gsx_set_values

}  // namespace gsx
