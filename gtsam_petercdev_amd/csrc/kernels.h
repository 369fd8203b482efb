// kernels.h — device-side tables and the launch functions of kernels.hip (product; gfx950).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/gsx.h"

namespace gsx {

typedef long long i64;

// Everything a per-factor kernel needs before it touches the state, in ONE 32-byte record (graph order): the chain
// factor id -> key pointer -> variable ids -> state offsets -> state was five dependent loads deep.
struct FactorRec {
  i64 jac_off;
  int s0, s1;                 // state offsets of the first two variables (-1: none)
  int meas_off, noise_off;    // doubles into meas / noise
  int type_kind;              // f_type | noise kind (with the robust bits) << 8 | ABS_* sub-kind of a TL_ABSOLUTE factor
                              // << 16 (0 elsewhere) | type of the first variable << 24
  int rows_dim;               // rows | dimension of the first variable (<= 255) << 8 | columns of [A b] << 16
};
// Immutable problem tables on the device (graph order).
struct DevProblem {
  int n_vars, n_factors;
  const int *var_type, *var_dim, *var_state_off, *var_tan_off;
  const int *f_type, *f_rows, *f_key_ptr, *f_vars, *f_noise_kind, *f_cols;
  const i64 *f_meas_off, *f_noise_off, *f_jac_off;
  const double *meas, *noise;
  const FactorRec* frec;  // per factor
  const int* f_active;  // factors this rank evaluates in the error kernels (nullptr: all n_active = n_factors)
  int n_active;
};

// One H-assembly term: panel[dst + i, j] += sum_r J[r, colB + i] * J[r, colA + j] (32-byte record).
struct TermRec {
  i64 jac;
  int m, colA, colB, dB, dst, pad;
};

// Packed per-variable / per-child records (32 bytes, fetched through the scalar path).
struct VarRec {
  i64 h_off, hmap_off;
  int dA, rows, loc, toff;
};
// Everything the leaf kernels need about one leaf clique, in schedule order (80 bytes through the scalar path: the
// dependent-load chain of a 64-thread workgroup is record -> data instead of id -> front tables -> variable tables ->
// data).  The H-panel fields describe the FIRST frontal variable (the only one of a BAL landmark clique).
struct LeafRec {
  i64 off, h_off, hmap_off, gidx_ptr;
  int n, F, nfv, lean;
  int dA, rows, loc, toff;
  int fvar_ptr, front, pad0, pad1;
};
// The three classes of a leaf launch that puts several cliques in a wave (backsolve_leaf_kernel; front_star_leaf_packed_kernel,
// with n64 = 0):
// cliques and workgroups of each
struct LeafPack {
  int n16, n32, n64, nb16, nb32;
};
// Separator rows a lane of a shared wave keeps in registers: a clique takes 16 lanes up to 64 separator rows, 32 lanes up
// to 128 (the rows the wave form keeps in registers), else the wave.  (2 rows a lane — 32 / 64 rows, the registers of the
// wave form — measured 59.1 us a launch on bal1723 against 53.6 us: profiles/README.md, r06.)
constexpr int kLeafPackRows = 4;
static_assert(16 * kLeafPackRows <= 64 && 32 * kLeafPackRows <= 128, "classes of backsolve_leaf_packed");
// A STAR LEAF (front_star_leaf_kernel): a lean, childless clique whose one frontal variable is of the star group of the
// H assembly (every BAL landmark, upload.hip: upload_symbolic).  Its factor blocks are read straight from [A b] through
// the variable's term records (three per factor: own block, partner block, rhs — the first factor's give the shape), 2-row
// factors at even offsets only; the clique's rows are the panel's (n = panel rows, own rows first, hmap a permutation).
constexpr int kStarMaxD = 3;
// Passes over its partner rows that a clique sharing a wave may take (star_leaf_pack_class): the wave runs to the passes
// of its tallest group, so the bound is the most a short clique waits for a neighbour.  Reasoned, not measured.
constexpr int kStarPackPasses = 4;
// The record also carries what cuts the dependent loads of a clique to record -> data: the factors' [A b] offsets when
// they are evenly spaced (jstride > 0: factor q at jac0 + q jstride — the observations of a landmark stored together; else
// through the term records) and the clique row of every partner row (prow: a row map per clique, in factor order).
struct StarLeafRec {  // 88 bytes
  i64 off, h_off, t0;             // arena L panel, H panel (its rhs row is written), first term record
  i64 jac0, prow_off;             // first factor's [A b] offset, the clique's partner rows in prow
  int n, nf, d, toff;             // clique rows, factors, frontal dimension, tangent offset (damping)
  int colA, colB, colR, dB;       // the factors' shape
  int front, jstride, rrow, pad0; // front, factor spacing in [A b] (0: uneven), clique row of the rhs
};
struct ChildRec {
  i64 src0, cmap_off;   // arena offset of the child's Schur complement (top-left), offset of its row map
  int nc, s1, pad0, pad1;
};
// One LDS-class front: what front_small needs before its first data load, in one 32-byte record (the chain is
// id -> record -> variable records (stored per front: fvar_recs) -> data)
struct FrontRec {
  i64 off;
  int n, F, nfv, fvar_ptr, child_ptr, nchild;
};

// Symbolic tables on the device.
struct DevSymbolic {
  int n_fronts;
  // fronts
  const i64* fr_off;            // arena offset
  const int *fr_N, *fr_F, *fr_nfv, *fr_fvar_ptr, *fvars, *fr_parent, *fr_child_ptr, *children;
  const int* fr_lean;           // 1: lean leaf — only its n x F L panel is stored, no Schur complement
  const i64 *cmap_ptr, *gidx_ptr;
  const int *cmap, *gidx;
  // H panels
  const i64 *h_off, *hmap_ptr;
  const int *h_rows, *hmap, *h_loc;
  // H assembly terms
  const i64* term_ptr;
  const TermRec* terms;
  const VarRec* var_recs;
  const ChildRec* child_recs;
  const FrontRec* front_recs;   // per front
  const VarRec* fvar_recs;      // var_recs in the order of fvars (a front's frontal variables are contiguous)
  // partial ("wildfire") back-substitution (gsx_backsubstitute_wildfire): when wf_dirty is set, a back-substitution
  // kernel first decides whether its clique is dirty — reached through a dirty parent, and re-eliminated (wf_replaced,
  // per front) or with a separator variable that changed (wf_changed, per variable) — records that in wf_dirty and
  // leaves a clean clique alone (ISAM2Clique::isDirty, gtsam/nonlinear/ISAM2Clique.cpp:68-90; children are visited only
  // through a dirty parent, :261-287)
  unsigned char* wf_dirty;
  const unsigned char *wf_replaced, *wf_changed;
};
#ifdef __HIPCC__
// every thread of the clique's workgroup (or wave: `writer` = its first lane) evaluates the same rule on the same bytes
__device__ __forceinline__ bool wildfire_skip(const DevSymbolic& S, int f, bool writer) {
  if (S.wf_dirty == nullptr) return false;
  const int p = S.fr_parent[f];
  bool dirty = (p < 0) || S.wf_dirty[p];
  if (dirty && !S.wf_replaced[f]) {
    dirty = false;
    for (int q = S.fr_fvar_ptr[f] + S.fr_nfv[f]; q < S.fr_fvar_ptr[f + 1]; ++q)
      if (S.wf_changed[S.fvars[q]]) {
        dirty = true;
        break;
      }
  }
  if (writer) S.wf_dirty[f] = dirty ? 1 : 0;
  return !dirty;
}
#endif

// status words written by the factorization / back-substitution kernels
struct DevStatus {
  int n_fail;        // fronts whose partial Cholesky failed (non-positive pivot or exponent-gap test)
  int first_front;   // smallest failing front id (INT_MAX when none)
  int n_nonfinite;   // non-finite entries met in back-substitution
  int n_cheirality;  // SFM factors zeroed in the last linearize
  int n_backsub;     // frontal variables back-substituted by the last wildfire pass (lastBacksubVariableCount)
};

// scalar slots in the device scalar buffer
// sharded problems: the slots summed over the ranks before the host reads them (bit k = slot k; two more bits for the
// status counters of the factorization / of linearize), kXScalars doubles in the exchange vector
constexpr int kXScalars = 16;
constexpr unsigned kXFact = 1u << 12, kXLin = 1u << 13;
void launch_shard_pack(const double* scalars, const DevStatus* status, unsigned dirty, double* x, hipStream_t st);
void launch_shard_unpack(const double* x, unsigned dirty, double* scalars, DevStatus* status, hipStream_t st);
// states of `n` variables (packed one after the other in `src`, variable i at src_off[i]) into the values vector
void launch_scatter_states(const DevProblem& P, const int* vars, const int* src_off, int n, const double* src,
                           double* values, hipStream_t st);
void launch_mask_copy(const double* in, const unsigned char* mask, int64_t n, double* out, hipStream_t st);

enum { SC_LAMBDA = 0, SC_ERR = 1, SC_LIN0 = 2, SC_LIND = 3, SC_TRIAL_ERR = 4, SC_DOT0 = 5, SC_DOT1 = 6, SC_DOT2 = 7,
       SC_DOT3 = 8, SC_LIN0_LOCAL = 9 /* 1/2 sum |b|^2 of this rank's factors: never exchanged */, SC_COUNT = 12 };

struct BigDesc {   // one big front of a level
  i64 off, xoff;             // arena offsets of the n x n front and of its n x F L-panel area
  int N, F, front, parent;   // parent front id (-1 root; kStandaloneFront: the dense entry, not a front of a tree)
};
constexpr int kStandaloneFront = -3;
// choleskyPartial's conditioning test per reference clique, after the factorization (kernels.hip)
void launch_cond_check(int n, const i64* last, const i64* prev, const int* front, const double* arena, DevStatus* status,
                       hipStream_t st);
// a big front owns n x n doubles followed by its n x F L panel (rows below each diagonal tile)
__host__ __device__ inline i64 big_panel_offset(int n) { return ((i64)n * n + 1) & ~(i64)1; }

// ---- launches (all asynchronous on `st`) ---------------------------------------------------------
// The factor lists of the linearize / error kernels: one per factor family whose kernel knows its shapes at compile time
// (a RangeFactor variant is a family), TL_GENERIC for the rare runtime-dimension ones.  GSX_F_LINEAR is in none.
enum { TL_SFM = 0, TL_BETWEEN_POSE2 = 1, TL_BETWEEN_POSE3 = 2, TL_GENERIC = 3, TL_PROJECTION = 4, TL_BEARINGRANGE = 5,
       TL_RANGE_POSE2_POINT = 6, TL_RANGE_POSE2_POSE = 7, TL_RANGE_POSE3_POINT = 8, TL_RANGE_POSE3_POSE = 9,
       TL_BEARING = 10, TL_STEREO = 11,
       // the forms that carry body_P_sensor behind their measurement (the same kernels with a compile-time switch), and
       // GeneralSFMFactor2
       TL_PROJECTION_SENSOR = 12, TL_STEREO_SENSOR = 13, TL_RANGE_POSE2_POINT_SENSOR = 14, TL_RANGE_POSE2_POSE_SENSOR = 15,
       TL_RANGE_POSE3_POINT_SENSOR = 16, TL_RANGE_POSE3_POSE_SENSOR = 17, TL_SFM2 = 18,
       // SmartProjectionPoseFactor<Cal3_S2>: kernels of its own (smart.hip), and state the handle keeps (SmartDev)
       TL_SMART = 19,
       // TranslationFactor and BilinearAngleTranslationFactor (gtsam/sfm/TranslationFactor.h)
       TL_TRANSLATION = 20, TL_BATA = 21,
       // the absolute-measurement factors: every single-key form of GSX_F_GPS, GSX_F_POSE_TRANSLATION_PRIOR,
       // GSX_F_POSE_ROTATION_PRIOR, GSX_F_ATTITUDE and GSX_F_MAG in one list (sorted by ABS_* sub-kind), and the two
       // two-key forms that came with them: BetweenFactor<Rot3> and GPSFactorArmCalib
       TL_ABSOLUTE = 22, TL_BETWEEN_ROT3 = 23, TL_GPS_CALIB = 24,
       // the epipolar factors, a list per form (each kernel knows its form at compile time, as the SENSOR forms do):
       // EssentialMatrixFactor, EssentialMatrixFactor2, EssentialMatrixFactor3 (told from 2 by its 15 measurement doubles),
       // EssentialMatrixFactor4<Cal3_S2>, EssentialMatrixConstraint
       TL_ESSENTIAL = 25, TL_ESSENTIAL_DEPTH = 26, TL_ESSENTIAL_DEPTH_ROTATED = 27, TL_ESSENTIAL_CALIB = 28,
       TL_ESSENTIAL_CONSTRAINT = 29,
       // PriorFactor<Unit3> and PriorFactor<EssentialMatrix>: lists of their own, not TL_GENERIC, so that the generic
       // kernels (local_coords) stay what they were for every graph without the two types
       TL_PRIOR_UNIT3 = 30, TL_PRIOR_ESSENTIAL = 31, kNumTypeLists = 32 };
// sub-kind of a TL_ABSOLUTE factor, in bits 16..23 of FactorRec::type_kind (its noise kind keeps bits 8..15)
enum { ABS_GPS = 0, ABS_GPS_ARM = 1, ABS_TRANS_POSE2 = 2, ABS_TRANS_POSE3 = 3, ABS_ROT_POSE2 = 4, ABS_ROT_POSE3 = 5,
       ABS_ATT_ROT3 = 6, ABS_ATT_POSE3 = 7, ABS_MAG_ROT3 = 8, ABS_MAG_POSE3 = 9, ABS_MAG_POSE2 = 10 };
// of a factor of type `t` on a first variable of type vt0 with nmeas doubles in the handle's measurement table (read only
// for GSX_F_GPS, whose entry is the caller's: upload.hip, factor_type_list); -1: not in that list
inline int absolute_kind_of(int t, int vt0, int vt1, long long nmeas) {
  switch (t) {
    case GSX_F_GPS: return vt1 >= 0 ? -1 : (nmeas > 3 ? ABS_GPS_ARM : ABS_GPS);
    case GSX_F_POSE_TRANSLATION_PRIOR: return vt0 == GSX_VAR_POSE2 ? ABS_TRANS_POSE2 : ABS_TRANS_POSE3;
    case GSX_F_POSE_ROTATION_PRIOR: return vt0 == GSX_VAR_POSE2 ? ABS_ROT_POSE2 : ABS_ROT_POSE3;
    case GSX_F_ATTITUDE: return vt0 == GSX_VAR_ROT3 ? ABS_ATT_ROT3 : ABS_ATT_POSE3;
    case GSX_F_MAG: return vt0 == GSX_VAR_ROT3 ? ABS_MAG_ROT3 : (vt0 == GSX_VAR_POSE3 ? ABS_MAG_POSE3 : ABS_MAG_POSE2);
  }
  return -1;
}
constexpr int kSensorListShift = TL_RANGE_POSE2_POINT_SENSOR - TL_RANGE_POSE2_POINT;  // range list -> its sensor form
// list of a factor of type `t` whose first two variables have types vt0, vt1 and whose measurement has nmeas doubles
// (the sensor forms are told by their length); -1: GSX_F_LINEAR, no list
inline int type_list_of(int t, int vt0, int vt1, long long nmeas) {
  switch (t) {
    case GSX_F_LINEAR: return -1;
    case GSX_F_PRIOR: return vt0 == GSX_VAR_UNIT3 ? TL_PRIOR_UNIT3 : (vt0 == GSX_VAR_ESSENTIAL ? TL_PRIOR_ESSENTIAL : TL_GENERIC);
    case GSX_F_SFM: return TL_SFM;
    case GSX_F_SFM2: return TL_SFM2;
    case GSX_F_PROJECTION: return nmeas > 7 ? TL_PROJECTION_SENSOR : TL_PROJECTION;
    case GSX_F_BEARINGRANGE: return TL_BEARINGRANGE;
    case GSX_F_BETWEEN:
      return vt0 == GSX_VAR_POSE2 ? TL_BETWEEN_POSE2
                                  : (vt0 == GSX_VAR_POSE3 ? TL_BETWEEN_POSE3 : (vt0 == GSX_VAR_ROT3 ? TL_BETWEEN_ROT3 : TL_GENERIC));
    case GSX_F_RANGE:
      return (vt0 == GSX_VAR_POSE2 ? (vt1 == GSX_VAR_POSE2 ? TL_RANGE_POSE2_POSE : TL_RANGE_POSE2_POINT)
                                   : (vt1 == GSX_VAR_POSE3 ? TL_RANGE_POSE3_POSE : TL_RANGE_POSE3_POINT)) +
             (nmeas > 1 ? kSensorListShift : 0);
    case GSX_F_BEARING: return TL_BEARING;
    case GSX_F_STEREO: return nmeas > 9 ? TL_STEREO_SENSOR : TL_STEREO;
    case GSX_F_SMART_PROJECTION: return TL_SMART;
    case GSX_F_TRANSLATION: return TL_TRANSLATION;
    case GSX_F_BILINEAR_TRANSLATION: return TL_BATA;
    case GSX_F_GPS: return vt1 >= 0 ? TL_GPS_CALIB : TL_ABSOLUTE;
    case GSX_F_POSE_TRANSLATION_PRIOR:
    case GSX_F_POSE_ROTATION_PRIOR:
    case GSX_F_ATTITUDE:
    case GSX_F_MAG: return TL_ABSOLUTE;
    case GSX_F_ESSENTIAL: return TL_ESSENTIAL;
    case GSX_F_ESSENTIAL_DEPTH: return nmeas > 6 ? TL_ESSENTIAL_DEPTH_ROTATED : TL_ESSENTIAL_DEPTH;
    case GSX_F_ESSENTIAL_CALIB: return TL_ESSENTIAL_CALIB;
    case GSX_F_ESSENTIAL_CONSTRAINT: return TL_ESSENTIAL_CONSTRAINT;
  }
  return TL_GENERIC;
}
// launch_error holds back one partial-sum slot per list a graph can fill, so that a list of few factors still gets its
// block.  The lists came in groups; the count is the end of the newest group that has a factor, so a graph keeps the
// shares — hence the summation order, hence the bits — that it had before later lists existed.
constexpr int kListGroupEnds[] = {TL_PROJECTION_SENSOR, TL_SMART, TL_TRANSLATION, TL_ABSOLUTE, TL_ESSENTIAL, kNumTypeLists};
constexpr int held_slots(const int counts[kNumTypeLists]) {
  int held = kListGroupEnds[0];
  for (int g = 1; g < (int)(sizeof(kListGroupEnds) / sizeof(kListGroupEnds[0])); ++g)
    for (int k = kListGroupEnds[g - 1]; k < kListGroupEnds[g]; ++k)
      if (counts[k] > 0) held = kListGroupEnds[g];
  return held;
}
constexpr int held_slots_with(int a, int b = TL_SFM) {  // of a graph with factors in the lists a and b
  int counts[kNumTypeLists] = {};
  counts[a] = counts[b] = 1;
  return held_slots(counts);
}
static_assert(held_slots_with(TL_STEREO) == TL_PROJECTION_SENSOR && held_slots_with(TL_SFM2) == TL_SMART &&
                  held_slots_with(TL_SMART) == TL_TRANSLATION && held_slots_with(TL_BATA) == TL_ABSOLUTE &&
                  held_slots_with(TL_GPS_CALIB, TL_TRANSLATION) == TL_ESSENTIAL &&
                  held_slots_with(TL_PRIOR_UNIT3, TL_ABSOLUTE) == kNumTypeLists && held_slots_with(TL_ESSENTIAL, TL_SMART) == kNumTypeLists,
              "the slots the nested conditional of launch_error held back, situation by situation");
// The state of the smart projection factors of a handle (smart.hip), per smart factor in graph order ("slot"): the cameras
// of the call in progress, and the re-triangulation cache of SmartProjectionFactor::decideIfTriangulate — the camera poses
// of the last triangulation, its point and its status (-1: never triangulated).
struct SmartDev {
  const int* slot;     // per FACTOR: its slot, -1 for every other type
  double* cams;        // slot x 8 prepared cameras (triangulate_math.h: Camera, 32 doubles)
  double* cache;       // slot x 8 x 12: R 9, t 3 of every camera at the last triangulation
  double* point;       // slot x 3
  int* status;         // slot: GSX_TRI_* or -1
  int* counters;       // [0] factors without a valid point in the last linearize; [1] factors the last call re-triangulated
  int n;               // smart factors of the problem
};
// `smart` may be null when type_counts[TL_SMART] == 0
void launch_linearize(const DevProblem& P, const int* const type_lists[kNumTypeLists], const int type_counts[kNumTypeLists],
                      const double* values, double* jac, DevStatus* status, hipStream_t st, const SmartDev* smart = nullptr);
// the graph error over the type lists of launch_linearize (a kernel per list, the factor type a compile-time constant)
void launch_error(const DevProblem& P, const int* const type_lists[kNumTypeLists], const int type_counts[kNumTypeLists],
                  const double* values, double* partials, int n_partials_cap, double* scalars, int slot, hipStream_t st,
                  const SmartDev* smart = nullptr);
// smart.hip.  Pass one of both calls: one lane per listed factor decides re-triangulation (consulting and updating the
// cache), triangulates, and leaves cameras, point and status in `S`.
void launch_smart_triangulate(const DevProblem& P, const int* list, int n, const double* values, const SmartDev& S, hipStream_t st);
// pass two of linearize: one wave per listed factor, one lane per column of [F b]; writes the factor's [A b]
void launch_smart_linearize(const DevProblem& P, const int* list, int n, const SmartDev& S, double* jac, hipStream_t st);
// pass two of the error: 0.5 |whitened (h - z)|^2 at the cached points, `blocks` partial sums into partials
void launch_smart_error(const DevProblem& P, const int* list, int n, const SmartDev& S, double* partials, int blocks,
                        hipStream_t st);
// slice > 0: the staged kernel (doubles of LDS per wave = the largest [A b] range of 64 consecutive factors); 0: the direct one
void launch_linear_error(const DevProblem& P, const double* jac, const double* delta, double* partials,
                         int n_partials_cap, double* scalars, int slice, hipStream_t st);
// the linearized errors of an LM trial from the right-hand sides and the solved step (kernels.hip: lin0_kernel)
void launch_lin0(const DevProblem& P, const double* jac, double* partials, int cap, double* scalars, hipStream_t st);
void launch_model_error(const DevProblem& P, const DevSymbolic& S, const int* vars, int nvars, const double* H,
                        const double* delta, const double* damp, double* partials, int cap, double* scalars, hipStream_t st);
void launch_retract(const DevProblem& P, const double* values, const double* delta, double* out, hipStream_t st);
void launch_assemble_h_group(const DevProblem& P, const DevSymbolic& S, const int* vars, int count, int threads,
                             int lds_bytes, bool global, const double* jac, double* H, hipStream_t st);
// star variables in bundles (first position in vars, count) of one shape and <= 64 factors: a wave per bundle
void launch_assemble_h_star_bundles(const DevProblem& P, const DevSymbolic& S, const int* vars, const int2* bundles,
                                    int count, const double* jac, double* H, hipStream_t st);
// the diagonal-panel variables and the star bundles in one launch (they write different panels)
void launch_assemble_h_diag_star(const DevProblem& P, const DevSymbolic& S, const int* dvars, int dcount, const int* svars,
                                 const int2* bundles, int scount, const double* jac, double* H, hipStream_t st);
void launch_hessian_diag(const DevProblem& P, const DevSymbolic& S, const double* H, double* diag, hipStream_t st);
void launch_make_damping(int n, const double* hdiag, int diagonal, double mind, double maxd, double* damp,
                         hipStream_t st);
// small fronts of one size class: ids[0..count), each eliminated by one workgroup of `threads`
// threads with (max_n^2) doubles of LDS
void launch_front_small(const DevProblem& P, const DevSymbolic& S, const int* ids, int count, int max_n,
                        int threads, const double* H, const double* damp, const double* scalars, double* arena,
                        DevStatus* status, hipStream_t st);
// the LDS-class fronts of one tier, whole subtrees in one launch (kernels.hip: front_tree_kernel)
struct TreeArgs {
  const int* start;   // fronts without an unfinished child in the tier
  int nstart;
  int* cursor;        // start entries claimed so far (zeroed by launch_begin_factorization)
  int* pending;       // per front: children of the tier still to arrive (restores itself to npend)
  const int *up, *npend;
};
void launch_front_tree(const DevProblem& P, const DevSymbolic& S, const TreeArgs& T, int max_n, int threads, const double* H,
                       const double* damp, const double* scalars, double* arena, DevStatus* status, hipStream_t st);
// MEDIUM fronts (gsx_internal.h), a workgroup each; LDS = (max_panel + max_n) doubles
void launch_front_medium(const DevProblem& P, const DevSymbolic& S, const int* ids, int count, int max_panel, int max_n,
                         const double* H, const double* damp, const double* scalars, double* arena, DevStatus* status,
                         hipStream_t st);
// the tree tier of the medium fronts (and of the LDS fronts above them)
void launch_front_tree_med(const DevProblem& P, const DevSymbolic& S, const TreeArgs& T, size_t lds_bytes, const double* H,
                           const double* damp, const double* scalars, double* arena, DevStatus* status, hipStream_t st);
void launch_big_init(const DevProblem& P, const DevSymbolic& S, const BigDesc* descs, int count, int max_n,
                     int max_nfv, const double* H, const double* damp, const double* scalars, double* arena,
                     hipStream_t st);
// Partial Cholesky of a group of big fronts (bigfront.hip): rounds of `chunk` frontal columns, three launches each —
// diag (L11 of the chunk, one workgroup per front), rows (L21 = A21 L11^-T, one per 32 rows), schur (A22 -= L21 L21').
struct BigPlan {
  int chunk = 0;
  std::vector<int> fw, rb, pairs;  // per round: widest chunk, most 32-row blocks below it, most lower tile pairs
  int rounds() const { return (int)fw.size(); }
};
void plan_big_group(const BigDesc* host_descs, int count, BigPlan& plan);
void launch_big_diag(const BigDesc* descs, int count, const BigPlan& plan, int round, double* arena, DevStatus* status,
                     hipStream_t st);
#ifdef GSX_STAMP
void big_stamp_dump(const char* what);
#endif
// rows of L21 below a round's chunk; big_rows_lds = the dynamic LDS its kernel asks for at a chunk of fw columns over
// `tiles` 32-row blocks in the whole launch on a device of `cus` compute units, and the rows one workgroup takes (*rows,
// may be null), 0: refused — the launcher then fails the factorization through status
size_t big_rows_lds(int fw, long tiles, int cus, int* rows);
void launch_big_rows(const BigDesc* descs, int count, const BigPlan& plan, int round, double* arena, DevStatus* status,
                     hipStream_t st);
void launch_big_schur(const BigDesc* descs, int count, const BigPlan& plan, int round, double* arena, hipStream_t st);
void launch_front_leaf(const DevProblem& P, const DevSymbolic& S, const LeafRec* recs, int count, int max_panel, int threads,
                       const double* H, const double* damp, const double* scalars, double* arena, DevStatus* status,
                       hipStream_t st);
// the star leaves of one launch group (front_star_leaf_kernel): H assembly and front_leaf of those cliques in one pass, same
// bits; the rhs rows of their H panels are written, the rest of those panels is not.  recs: the n16 cliques that take 16
// lanes of a wave, then the n32 that take 32, then n64 eliminated a wave each.  star_leaf_pack_class: the lanes a clique of
// nf factors with partners of dimension dB gets (16, 32 or 64).
void launch_front_star_leaf(const DevSymbolic& S, const StarLeafRec* recs, int n16, int n32, int n64, const int* prow,
                            const double* jac, const double* damp, const double* scalars, double* H, double* arena,
                            DevStatus* status, hipStream_t st);
int star_leaf_pack_class(int nf, int dB);
// Deterministic extend-add into big parents (big_gather).
// A source is either a block of a child's stored Schur complement (F = 0: entry (i, j) at off + i + j ld) or, for a
// lean leaf child, the product form -W_b W_a' with W_b = rows off.., W_a = rows off + d2.. of the child's n x F L panel.
struct GatherSrc {   // 16 bytes
  i64 off;
  int d2;            // product form: offset of the second row block relative to the first
  int ldF;           // ld | F << 24
};
struct GatherSeg {   // 32 bytes: one wave's work — up to kGatherChunk consecutive sources of one destination block
  i64 dst;           // arena offset of the destination block (top-left entry)
  i64 src;           // first source record
  int n, ld, dims;   // number of sources; destination ld; dB | dA << 8 | diag << 16
  int slot;          // -1: add straight into dst; else scratch slot of a split task
};
struct GatherArgs {
  const GatherSeg* segs;
  const GatherSrc* srcs;
  const i64* gt_dst;                       // per task (combine pass)
  const int *gt_ld, *gt_dims, *gm_task, *gm_slot, *gm_nslots;
  double* scratch;  // slots x 256 doubles (a 16 x 16 accumulator tile in matrix-core register layout)
};
void launch_big_gather(const GatherArgs& G, int seg0, int nseg, int m0, int nm, double* arena, hipStream_t st);
void launch_backsolve(const DevSymbolic& S, const int* ids, int count, int threads, int max_n, const double* arena,
                      double* delta, DevStatus* status, hipStream_t st);
// blocked fronts of a level whose L11 tiles fit in LDS (bigfront.hip); backsolve_big_lds = 0: they do not, use the kernel above
size_t backsolve_big_lds(int max_n, int max_F, int max_sep_rows);
void launch_backsolve_big(const DevSymbolic& S, const int* ids, int count, int max_n, int max_F, const double* arena,
                          double* delta, DevStatus* status, hipStream_t st);
// LDS-class fronts with <= 64 frontal columns (bigfront.hip): all loads of a front in flight together
bool backsolve_small_fits(int max_n, int max_F);
void launch_backsolve_small(const DevSymbolic& S, const int* ids, int count, int max_F, const double* arena, double* delta,
                            DevStatus* status, hipStream_t st);
// the tree fronts of all levels in one launch, top-down (bigfront.hip: backsolve_tree_kernel)
struct BacksolveTreeArgs {
  const int* roots;            // tree fronts whose parent is not a tree front
  int n_roots, n_tickets;      // ... their number; n_tickets = n_roots + the tree fronts that are not a first child
  const int *child_ptr, *children;   // per front: its tree children (CSR over all fronts), the deepest subtree first
  unsigned long long* ready;   // n_tickets - n_roots entries: epoch << 32 | front
  int *head, *tail;            // tickets handed out; entries published (zeroed by the host before the launch)
  unsigned epoch;              // differs from launch to launch (never 0)
};
void launch_backsolve_tree(const DevSymbolic& S, const BacksolveTreeArgs& Q, const double* arena, double* delta,
                           DevStatus* status, hipStream_t st);
// ISAM2's partial ("wildfire") back-substitution, the pass after a level's kernels: a dirty clique's new frontal solution
// is compared with the old one — a change of at least `threshold` in the infinity norm (or a re-eliminated clique) marks
// its frontal variables as changed, a smaller one is undone (valuesChanged / restoreFromOriginals,
// gtsam/nonlinear/ISAM2Clique.cpp:175-201).
struct WildfireArgs {
  const unsigned char *replaced, *dirty;  // per front
  unsigned char* changed;                 // per variable
  const double* old_delta;                // the solution before the pass
  DevStatus* status;                      // n_backsub += frontal variables back-substituted
  double threshold;
};
// flags[ids[k]] = 1 (the cliques a partial re-elimination has just redone)
void launch_mark_fronts(const int* ids, int count, unsigned char* flags, hipStream_t st);
void launch_wildfire_post(const DevSymbolic& S, const int* ids, int count, bool wave_per_clique, const WildfireArgs& W,
                          double* delta, hipStream_t st);
// leaf cliques of a level in one launch: recs holds n16 cliques solved four to a wave (16 lanes each), then n32 solved two
// to a wave, then n64 solved a wave each.  leaf_pack_class: the lanes a clique of n rows and F columns gets in a launch
// whose widest clique has max_F columns — the narrowest group whose kLeafPackRows register rows a lane cover the separator
// and whose lanes hold the F x F triangle
int leaf_pack_class(int n, int F, int max_F);
void launch_backsolve_leaf(const DevSymbolic& S, const LeafRec* recs, int n16, int n32, int n64, int max_F,
                           const double* arena, double* delta, DevStatus* status, hipStream_t st);
// Dogleg (gtsam/nonlinear/DoglegOptimizerImpl.*): gradient g = A'b out of the H panels' rhs rows, |A x|^2 over the
// linearized graph, dot products and out = alpha a + beta b on tangent vectors (deterministic two-stage reductions)
void launch_gradient(const DevProblem& P, const DevSymbolic& S, const double* H, double* g, hipStream_t st);
void launch_ax_sqnorm(const DevProblem& P, const double* jac, const double* x, double* partials, int cap, double* scalars,
                      int slot, hipStream_t st);
void launch_vec_dot(const double* a, const double* b, int64_t n, double* partials, int cap, double* scalars, int slot,
                    hipStream_t st);
void launch_vec_axpby(double* out, double alpha, const double* a, double beta, const double* b, int64_t n, hipStream_t st);
// Marginal covariance block of one variable from the factorization: forward substitution of the
// variable's unit columns up the path of cliques from its own clique to the root, Sigma_vv = sum over the path of y_F' y_F.
// path[0..npath): front ids, child to root; (loc, dA): the variable's rows inside path[0]; lds_doubles = 2 max_n dA.
void launch_marginal_path(const DevSymbolic& S, const int* path, int npath, int loc, int dA, int max_n, const double* arena,
                          double* out, double* Y, int64_t n_tan, hipStream_t st);
void launch_joint_cross(const double* Ya, const double* Yb, int64_t n_tan, int dA, int dB, double* out, hipStream_t st);
// Marginal covariances of all variables in one top-down pass (marginals.hip).  Every front of class 1 or 2 owns a block
// of the covariance arena: its (n - 1) x (n - 1) Sigma over [frontal | separator] rows (column-major, lower triangle
// significant) and a work area of F (n - 1) doubles (X' = L11^-T, then Kt = L21 X).  Per level, from the top: prep
// (X' and the gather of Sigma_SS from the parent's block), kt, sf, ff — one work item per workgroup; then the diagonal
// blocks of the variables (emit) and, last, the leaf-kernel cliques (class 0), which own no block.
struct MargItem {   // 16 bytes
  int front, ti, tj, pad;   // 32 x 32 tile (ti, tj) of the step's result; prep: ti < 0 = the inverse, else 32 separator rows
};
struct MargArgs {
  const i64 *slot, *work;   // per front: doubles into `cov` (-1: a class-0 front)
  double* cov;
  const double* arena;
  const i64* out_off;       // per variable: doubles into `out`, -1: not asked for
  const int* var_dim;
  double* out;
};
void launch_marg_prep(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st);
void launch_marg_kt(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st);
void launch_marg_sf(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st);
void launch_marg_ff(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st);
void launch_marg_emit(const DevSymbolic& S, const MargArgs& M, const int2* vars, int count, hipStream_t st);
void launch_marg_leaf(const DevSymbolic& S, const MargArgs& M, const int* ids, int count, hipStream_t st);
void launch_set_scalar(double* scalars, int slot, double v, hipStream_t st);
// Hard constraints (constraint.hip): one record per constrained front (Symbolic::con_fronts order, children first)
struct ConDesc {
  i64 off;          // arena offset of the front's n x n panel
  i64 work, fwd;    // doubles into the work buffer: 3 K n for the rows / B / Z; n_fwd (n - F) rows handed to the parent
  i64 iwork;        // ints into the int work buffer: n + 2 K + 1
  int N, F, K, n_fwd;
  int own_begin, own_end;      // its own rows (ConTables::own_*)
  int child_begin, child_end;  // ConTables::child_list: the fronts below whose leftover rows arrive here
  int front;
  int fwd_map;                 // ConTables::fwd_map + this: per separator + rhs row, the row of the front its leftovers go to
};
struct ConTables {
  const ConDesc* descs;
  const int *own_col_ptr, *own_cols, *own_m;
  const i64* own_jac;
  const int* child_list;
  const int* fwd_map;
  double* work;
  int* iwork;
};
// the constrained fronts descs[first .. first + count), all of one level, after their gather and before their factorization
void launch_constraint_fronts(const DevSymbolic& S, const ConTables& T, int first, int count, int max_n, const double* jac,
                              double* arena, DevStatus* status, hipStream_t st);
// hdiag[tan[i]] -= sum over k in ptr[i] .. ptr[i + 1] of w[k] jac[jidx[k]]^2 (the constraint rows' share of diag(J'J) at
// the reference's weight)
void launch_constraint_hdiag(int n, const int* tan, const int* ptr, const i64* jidx, const double* w, const double* jac,
                             double* hdiag, hipStream_t st);
constexpr int kTreeCursors = 8;  // cursors of the tree kernels' start lists, zeroed with the status words
void launch_begin_factorization(double* scalars, double lambda, DevStatus* status, int* tree_cursors, hipStream_t st);
// dense unit kernel for gsx_cholesky_partial: in-place lower partial Cholesky of an n x n
// column-major matrix (lower triangle significant)
void launch_dense_partial(double* a, int n, int nf, DevStatus* status, hipStream_t st);
int max_dynamic_lds();

// ---- preconditioned conjugate gradients on the linearized graph (pcg.hip) ------------------------------------------
// The largest tangent dimension of a variable the PCG kernels take, with either preconditioner: pcg_build_blocks keeps a
// d x d block per wave in LDS and gives each row of a Cholesky column step a lane, pcg_jty keeps d products per wave in
// LDS and needs two terms' worth of lanes (G = 64 / d >= 2).  Typed variables have 3, 6 and 9; VECTOR(d) is the caller's.
constexpr int kPcgMaxDim = 32;
// Iterations the host enqueues between two reads of the done flag (7 launches each, 10 with a restart).
#ifndef GSX_PCG_BATCH
#define GSX_PCG_BATCH 8
#endif
constexpr int kPcgBatch = GSX_PCG_BATCH;
static_assert(kPcgBatch >= 1, "GSX_PCG_BATCH must be at least 1");
// the loop's scalars on the device (ConjugateGradientSolver.h:119-151), written by one thread of a one-workgroup kernel
struct PcgScalars {
  double gamma, gamma0, threshold, alpha, beta, pAp;
  int k;         // iterations completed
  int done;      // the reference's loop condition has failed (or fail != 0): every later kernel returns at once
  int fail;      // 1: p'Ap non-positive or non-finite while gamma > threshold; 2: a diagonal block has no Cholesky factor
  int bad_var;   // smallest variable whose block failed (INT_MAX: none)
};
struct HostProblem;
struct PcgWork;   // device tables and vectors of one problem
int pcg_max_dim(const HostProblem& P);
hipError_t pcg_work_create(const HostProblem& P, hipStream_t st, PcgWork** out);
void pcg_work_destroy(PcgWork* w);
// x (device, tangent order) = the PCG estimate of (J'J + lambda diag(damp)) x = J'b; synchronises `st` once per batch
hipError_t pcg_run(PcgWork* w, const double* jac, const double* damp, double lambda, const gsx_pcg_params& prm, double* x,
                   DevStatus* status, hipStream_t st, PcgScalars* out);

}  // namespace gsx
