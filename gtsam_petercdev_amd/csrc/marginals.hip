// marginals.hip — marginal covariances of all variables in one top-down pass (selected inversion / Takahashi recursion
// over the resident factorization; the reference reaches the same blocks through cached separator marginals of the
// Bayes tree: gtsam/inference/BayesTreeCliqueBase-inst.h, gtsam/nonlinear/Marginals.cpp:107-136).  Product code, gfx950.
//
// Per front (F frontal scalars, s = n - F - 1 separator scalars, L = R' stored as L11 (F x F lower) and L21 (s x F)):
//   X = L11^-1,  Kt = L21 X (= K'),  Sigma_SF = -Sigma_SS Kt,  Sigma_FF = X'X - Kt' Sigma_SF
// with Sigma_SS gathered from the parent's finished block through the child's row map.  A front that can have children
// (class 1 and 2) keeps its (n - 1) x (n - 1) block in the covariance arena (lower triangle significant); the
// leaf-kernel cliques (class 0, always childless) only emit the diagonal blocks of their variables.  Parents and children
// are separated by kernel boundaries and no kernel uses atomics: the result is the same bits run to run.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_util.h"

namespace gsx {

namespace {

constexpr int MT = 32;   // tile edge of the products (a workgroup of 256 threads owns an MT x MT output tile, 2 x 2 a thread)

// L(r, j), r >= j, of a front in any of the three footprints (marginal_path_kernel, kernels.hip): inside j's 32-row
// diagonal tile of a blocked front the value sits in the front itself, below it in the L panel
struct FrontL {
  const double* A;
  const double* Lp;
  int n, F;
  bool big;
  __device__ __forceinline__ FrontL(const DevSymbolic& S, const double* arena, int f) {
    n = S.fr_N[f];
    F = S.fr_F[f];
    A = arena + S.fr_off[f];
    big = (S.fr_lean[f] & 2) != 0;
    Lp = big ? A + big_panel_offset(n) : A;
  }
  __device__ __forceinline__ double operator()(int r, int j) const {
    const int tile_end = min((j / 32 + 1) * 32, F);
    return (big && r >= tile_end) ? Lp[r + (i64)j * n] : A[r + (i64)j * n];
  }
};

// acc (2 x 2 a thread: rows tx, tx + 16, columns ty, ty + 16 of the tile) += sum over k in [k0, k1) of a(k, i) b(k, j);
// a / b return 0 outside their operand.  AK / BK: the operand is contiguous in memory along k (else along i / j) — the
// order in which the 256 threads fetch a 32 x 32 piece of it.
template <bool AK, bool BK, class FA, class FB>
__device__ __forceinline__ void tile_mac(double (&acc)[2][2], int k0, int k1, FA a, FB b, double (*As)[MT + 1],
                                         double (*Bs)[MT + 1]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int kb = k0; kb < k1; kb += MT) {
    __syncthreads();
    for (int e = tid; e < MT * MT; e += 256) {
      const int lo = e & (MT - 1), hi = e / MT;
      const int ka = AK ? lo : hi, ia = AK ? hi : lo;
      As[ka][ia] = (kb + ka < k1) ? a(kb + ka, ia) : 0.0;
      const int kq = BK ? lo : hi, jb = BK ? hi : lo;
      Bs[kq][jb] = (kb + kq < k1) ? b(kb + kq, jb) : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < MT; ++kk) {
      const double a0 = As[kk][tx], a1 = As[kk][tx + 16], b0 = Bs[kk][ty], b1 = Bs[kk][ty + 16];
      acc[0][0] = fma(a0, b0, acc[0][0]);
      acc[1][0] = fma(a1, b0, acc[1][0]);
      acc[0][1] = fma(a0, b1, acc[0][1]);
      acc[1][1] = fma(a1, b1, acc[1][1]);
    }
  }
}

// ---- step 1: X' = L11^-T into the work area (item.ti < 0) and Sigma_SS from the parent's block (item.ti >= 0: separator
// rows [32 ti, 32 ti + 32), every column) ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) marg_prep_kernel(DevSymbolic S, MargArgs M, const MargItem* items) {
  const MargItem it = items[blockIdx.x];
  const int f = it.front, tid = threadIdx.x;
  const FrontL L(S, M.arena, f);
  const int F = L.F, m = L.n - 1, s = m - F;
  if (it.ti < 0) {
    // Y = X' (upper triangular, F x F, ld F): thread c owns row c of Y = column c of X, forward substitution
    // L11 x = e_c.  The sum runs from k = 0 (x_k = 0 above the diagonal) so that L(i, k) is one address for the workgroup.
    double* Y = M.cov + M.work[f];
    for (int c = tid; c < F; c += 256) {
      for (int i = 0; i < F; ++i) {
        double acc = (i == c) ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) acc = fma(-L(i, k), Y[c + (i64)k * F], acc);
        Y[c + (i64)i * F] = (i >= c) ? acc / L(i, i) : 0.0;
      }
    }
    return;
  }
  const int p = S.fr_parent[f];
  const double* Pc = M.cov + M.slot[p];
  const int mp = S.fr_N[p] - 1;
  const int* cm = S.cmap + S.cmap_ptr[f];
  double* Sg = M.cov + M.slot[f];
  const int r0 = it.ti * 32, nr = min(32, s - r0);
  for (i64 e = tid; e < (i64)nr * s; e += 256) {
    const int r = r0 + (int)(e % nr), c = (int)(e / nr);
    const int a = cm[r], b = cm[c];
    Sg[(F + r) + (i64)(F + c) * m] = Pc[max(a, b) + (i64)min(a, b) * mp];
  }
}

// ---- step 2: Kt (s x F, ld s) = L21 X, tile (ti, tj); X(k, j) = Y(j, k) is zero for k < j -------------------------------
__global__ void __launch_bounds__(256) marg_kt_kernel(DevSymbolic S, MargArgs M, const MargItem* items) {
  __shared__ double As[MT][MT + 1], Bs[MT][MT + 1];
  const MargItem it = items[blockIdx.x];
  const int f = it.front;
  const FrontL L(S, M.arena, f);
  const int F = L.F, s = L.n - 1 - F;
  const double* Y = M.cov + M.work[f];
  double* Kt = M.cov + M.work[f] + (i64)F * F;
  const int i0 = it.ti * MT, j0 = it.tj * MT;
  double acc[2][2] = {{0, 0}, {0, 0}};
  tile_mac<false, false>(
      acc, j0, F, [&](int k, int i) { return (i0 + i < s) ? L(F + i0 + i, k) : 0.0; },
      [&](int k, int j) { return (j0 + j < F) ? Y[(j0 + j) + (i64)k * F] : 0.0; }, As, Bs);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
      if (i < s && j < F) Kt[i + (i64)j * s] = acc[a][b];
    }
}

// ---- step 3: Sigma_SF (rows F.., columns 0..F of the block) = -Sigma_SS Kt ----------------------------------------------
__global__ void __launch_bounds__(256) marg_sf_kernel(DevSymbolic S, MargArgs M, const MargItem* items) {
  __shared__ double As[MT][MT + 1], Bs[MT][MT + 1];
  const MargItem it = items[blockIdx.x];
  const int f = it.front;
  const int n = S.fr_N[f], F = S.fr_F[f], m = n - 1, s = m - F;
  double* Sg = M.cov + M.slot[f];
  const double* Kt = M.cov + M.work[f] + (i64)F * F;
  const int i0 = it.ti * MT, j0 = it.tj * MT;
  double acc[2][2] = {{0, 0}, {0, 0}};
  tile_mac<false, true>(
      acc, 0, s, [&](int k, int i) { return (i0 + i < s) ? Sg[(F + i0 + i) + (i64)(F + k) * m] : 0.0; },
      [&](int k, int j) { return (j0 + j < F) ? Kt[k + (i64)(j0 + j) * s] : 0.0; }, As, Bs);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
      if (i < s && j < F) Sg[(F + i) + (i64)j * m] = -acc[a][b];
    }
}

// ---- step 4: Sigma_FF (lower triangle) = X'X - Kt' Sigma_SF, lower tiles ti >= tj ---------------------------------------
__global__ void __launch_bounds__(256) marg_ff_kernel(DevSymbolic S, MargArgs M, const MargItem* items) {
  __shared__ double As[MT][MT + 1], Bs[MT][MT + 1];
  const MargItem it = items[blockIdx.x];
  const int f = it.front;
  const int n = S.fr_N[f], F = S.fr_F[f], m = n - 1, s = m - F;
  double* Sg = M.cov + M.slot[f];
  const double* Y = M.cov + M.work[f];
  const double* Kt = Y + (i64)F * F;
  const int i0 = it.ti * MT, j0 = it.tj * MT;
  double acc[2][2] = {{0, 0}, {0, 0}};
  // -Kt' Sigma_SF first, then the sign flips and X'X is added: X(k, i) = Y(i, k), zero for k < i
  tile_mac<true, true>(
      acc, 0, s, [&](int k, int i) { return (i0 + i < F) ? Kt[k + (i64)(i0 + i) * s] : 0.0; },
      [&](int k, int j) { return (j0 + j < F) ? Sg[(F + k) + (i64)(j0 + j) * m] : 0.0; }, As, Bs);
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = -acc[a][b];
  tile_mac<false, false>(
      acc, i0, F, [&](int k, int i) { return (i0 + i < F) ? Y[(i0 + i) + (i64)k * F] : 0.0; },
      [&](int k, int j) { return (j0 + j < F) ? Y[(j0 + j) + (i64)k * F] : 0.0; }, As, Bs);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
      if (i < F && j <= i) Sg[i + (i64)j * m] = acc[a][b];
    }
}

// ---- the variables' diagonal blocks out of the finished blocks (a thread per variable, lower triangle mirrored) ---------
__global__ void __launch_bounds__(256) marg_emit_kernel(DevSymbolic S, MargArgs M, const int2* vars, int count) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  const int v = vars[q].x, f = vars[q].y;
  const int m = S.fr_N[f] - 1, loc = S.h_loc[v], d = M.var_dim[v];
  const double* Sg = M.cov + M.slot[f];
  double* o = M.out + M.out_off[v];
  for (int b = 0; b < d; ++b)
    for (int a = b; a < d; ++a) {
      const double x = Sg[(loc + a) + (i64)(loc + b) * m];
      o[a + b * d] = x;
      o[b + a * d] = x;
    }
}

// ---- leaf-kernel cliques (class 0: childless, F <= 16, lean n x F panel or materialised; both are A[r + j n] for the
// frontal columns): a wave per clique, four to a workgroup.  Sigma_FF = X' (I + L21' Sigma_SS L21) X; the separator is
// walked in strips of 64 rows (a lane per row), whatever its length.
constexpr int kLeafF = 16;
__global__ void __launch_bounds__(256) marg_leaf_kernel(DevSymbolic S, MargArgs M, const int* ids, int count) {
  __shared__ double lds[4][64 * kLeafF + 2 * kLeafF * kLeafF];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + wave;
  if (q >= count) return;
  const int f = ids[q];
  double* ts = lds[wave];                  // 64 x F strip of Sigma_SS L21, later N = Ms X
  double* Xs = ts + 64 * kLeafF;           // X (k, c) at k + 16 c
  double* Ms = Xs + kLeafF * kLeafF;       // I + L21' Sigma_SS L21
  const int n = S.fr_N[f], F = S.fr_F[f], s = n - 1 - F;
  const double* A = M.arena + S.fr_off[f];
  if (lane < F) {
    const int c = lane;
    for (int i = 0; i < F; ++i) {
      double acc = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) acc = fma(-A[i + (i64)k * n], Xs[k + kLeafF * c], acc);
      Xs[i + kLeafF * c] = (i >= c) ? acc / A[i + (i64)i * n] : 0.0;
    }
  }
  for (int e = lane; e < F * F; e += 64) Ms[(e % F) + kLeafF * (e / F)] = (e % F == e / F) ? 1.0 : 0.0;
  wave_sync();
  if (s > 0) {
    const int p = S.fr_parent[f];
    const double* Pc = M.cov + M.slot[p];
    const int mp = S.fr_N[p] - 1;
    const int* cm = S.cmap + S.cmap_ptr[f];
    for (int i0 = 0; i0 < s; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < s;
      const int ci = valid ? cm[i] : 0;
      double tb[kLeafF];
#pragma unroll
      for (int b = 0; b < kLeafF; ++b) tb[b] = 0.0;
      for (int j = 0; j < s; ++j) {
        const int cj = cm[j];
        const double sig = valid ? Pc[max(ci, cj) + (i64)min(ci, cj) * mp] : 0.0;
#pragma unroll
        for (int b = 0; b < kLeafF; ++b)
          if (b < F) tb[b] = fma(sig, A[(F + j) + (i64)b * n], tb[b]);
      }
#pragma unroll
      for (int b = 0; b < kLeafF; ++b)
        if (b < F) ts[lane + 64 * b] = tb[b];
      wave_sync();
      const int ni = min(64, s - i0);
      for (int e = lane; e < F * F; e += 64) {
        const int a = e % F, b = e / F;
        double acc = 0.0;
        for (int ii = 0; ii < ni; ++ii) acc = fma(A[(F + i0 + ii) + (i64)a * n], ts[ii + 64 * b], acc);
        Ms[a + kLeafF * b] += acc;
      }
      wave_sync();
    }
  }
  // N = Ms X into ts (k + 16 b)
  for (int e = lane; e < F * F; e += 64) {
    const int a = e % F, b = e / F;
    double acc = 0.0;
    for (int k = b; k < F; ++k) acc = fma(Ms[a + kLeafF * k], Xs[k + kLeafF * b], acc);
    ts[a + kLeafF * b] = acc;
  }
  wave_sync();
  const int v0 = S.fr_fvar_ptr[f], nfv = S.fr_nfv[f];
  for (int vq = 0; vq < nfv; ++vq) {
    const int v = S.fvars[v0 + vq];
    const i64 oo = M.out_off[v];
    if (oo < 0) continue;
    const int d = M.var_dim[v], loc = S.h_loc[v];
    for (int e = lane; e < d * d; e += 64) {
      const int a = e % d, b = e / d;
      const int hi = loc + max(a, b), lo = loc + min(a, b);
      double acc = 0.0;
      for (int k = hi; k < F; ++k) acc = fma(Xs[k + kLeafF * hi], ts[k + kLeafF * lo], acc);
      M.out[oo + e] = acc;
    }
  }
}

}  // namespace

void launch_marg_prep(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st) {
  if (count) marg_prep_kernel<<<count, 256, 0, st>>>(S, M, items);
}
void launch_marg_kt(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st) {
  if (count) marg_kt_kernel<<<count, 256, 0, st>>>(S, M, items);
}
void launch_marg_sf(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st) {
  if (count) marg_sf_kernel<<<count, 256, 0, st>>>(S, M, items);
}
void launch_marg_ff(const DevSymbolic& S, const MargArgs& M, const MargItem* items, int count, hipStream_t st) {
  if (count) marg_ff_kernel<<<count, 256, 0, st>>>(S, M, items);
}
void launch_marg_emit(const DevSymbolic& S, const MargArgs& M, const int2* vars, int count, hipStream_t st) {
  if (count) marg_emit_kernel<<<(count + 255) / 256, 256, 0, st>>>(S, M, vars, count);
}
void launch_marg_leaf(const DevSymbolic& S, const MargArgs& M, const int* ids, int count, hipStream_t st) {
  if (count) marg_leaf_kernel<<<(count + 3) / 4, 256, 0, st>>>(S, M, ids, count);
}

}  // namespace gsx
