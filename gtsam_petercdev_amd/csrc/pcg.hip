// pcg.hip — preconditioned conjugate gradients on the linearized graph (product; gfx950, FP64 throughout).
//
// preconditionedConjugateGradient (gtsam/linear/ConjugateGradientSolver.h:109-171) restated on the device for the system
// PCGSolver hands it (gtsam/linear/PCGSolver.cpp: GaussianFactorGraphSystem): A = J'J + lambda D, b = J'b, x0 = 0, with
// BlockJacobiPreconditioner (gtsam/linear/Preconditioner.cpp:87-176: L_v = chol(lower) of variable v's diagonal block,
// leftPrecondition solves with L, rightPrecondition with L') or DummyPreconditioner (the identity).
//
// A is never formed.  One product q = A p is two passes over the [A b] blocks of the factors (JacobianFactor layout,
// column-major m x (sum d + 1)): y = J p, a thread per residual row, then q_v = sum over the variable's term list of
// A_fv' y_f + lambda D_v p_v, a wave per variable.  Every sum has a fixed shape — a lane takes every G-th term of the list in
// list order, the G partial sums of a component are added in lane order, the per-variable partials of a dot product are
// summed by one workgroup in a fixed strided + tree order — so a solve gives the same bits on every run; there are no
// floating-point atomics.
//
// The loop's scalars (gamma, alpha, beta, threshold, k, the done flag) live in one PcgScalars record on the device; two
// one-workgroup kernels per iteration finish the dot products and update them.  The host enqueues kPcgBatch iterations
// and reads the record once per batch; after `done` is set every kernel returns at its first instruction, so x stays what
// it was when the reference's loop condition failed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "gsx_internal.h"
#include "kernels.h"

namespace gsx {

namespace {

struct PcgVarRec {   // 24 bytes
  i64 lofs;          // doubles into the L blocks (d x d column-major, lower triangle; the upper one is zero)
  int toff, d;       // tangent offset, tangent dimension
  int t0, t1;        // the variable's terms
};
struct PcgTermRec {  // 24 bytes: one (factor, variable) incidence, in graph order of the factors
  i64 jac;           // the factor's [A b]
  int m, col;        // rows; first column of the variable's block
  int yoff, bcol;    // the factor's rows in y; the rhs column
};
struct PcgRowRec {   // 24 bytes: one residual row
  i64 a0;            // its first entry in [A b] (the column stride is m)
  int m, k0, k1, pad;
};
struct PcgKeyRec {   // one (factor, key): first column, tangent offset, dimension
  int col, toff, d;
};

constexpr int kRedThreads = 256;

// sum of part[0 .. n) by one workgroup of kRedThreads threads, the same order on every run; valid in thread 0
__device__ double block_sum(const double* part, int n) {
  __shared__ double red[kRedThreads];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += kRedThreads) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kRedThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// the loop's scalars, and the status words the block build counts in (the damping weight the factorization kernels read
// from the scalar buffer is left alone: a resident factorization and its lambda stay what they were)
__global__ void pcg_begin_kernel(PcgScalars* sc, DevStatus* status) {
  status->n_fail = 0;
  status->first_front = INT_MAX;
  status->n_nonfinite = 0;
  sc->gamma = sc->gamma0 = sc->threshold = sc->alpha = sc->beta = sc->pAp = 0.0;
  sc->k = 0;
  sc->done = 0;
  sc->fail = 0;
  sc->bad_var = INT_MAX;
}

// L_v = chol(sum over the term list of A_fv' A_fv + lambda D_v), a wave per variable, the block in LDS
__global__ void __launch_bounds__(64) pcg_build_blocks_kernel(PcgScalars* sc, const PcgVarRec* vars, const PcgTermRec* terms,
                                                              const double* jac, const double* damp, double lambda,
                                                              double* L, DevStatus* status) {
  __shared__ double A[kPcgMaxDim * kPcgMaxDim];
  const PcgVarRec V = vars[blockIdx.x];
  const int d = V.d, lane = threadIdx.x;
  const int E = d * (d + 1) / 2;
  for (int e = lane; e < E; e += 64) {
    int j = 0, rem = e;
    while (rem >= d - j) {
      rem -= d - j;
      ++j;
    }
    const int i = j + rem;
    double s = 0;
    for (int t = V.t0; t < V.t1; ++t) {
      const PcgTermRec T = terms[t];
      const double* ai = jac + T.jac + (i64)(T.col + i) * T.m;
      const double* aj = jac + T.jac + (i64)(T.col + j) * T.m;
      for (int r = 0; r < T.m; ++r) s += ai[r] * aj[r];
    }
    if (i == j) s += lambda * damp[V.toff + i];
    A[i + j * d] = s;
  }
  __syncthreads();
  for (int j = 0; j < d; ++j) {
    if (lane == 0) {
      double s = A[j + j * d];
      for (int k = 0; k < j; ++k) s -= A[j + k * d] * A[j + k * d];
      if (!(s > 0.0) || !isfinite(s)) {   // Eigen's llt reports NumericalIssue here; the reference goes on with NaNs
        atomicAdd(&status->n_fail, 1);
        atomicMin(&sc->bad_var, (int)blockIdx.x);
        s = 1.0;
      }
      A[j + j * d] = sqrt(s);
    }
    __syncthreads();
    if (lane > j && lane < d) {
      double s = A[lane + j * d];
      for (int k = 0; k < j; ++k) s -= A[lane + k * d] * A[j + k * d];
      A[lane + j * d] = s / A[j + j * d];
    }
    __syncthreads();
  }
  for (int e = lane; e < d * d; e += 64) L[V.lofs + e] = (e % d >= e / d) ? A[e] : 0.0;
}

// y = J v, a thread per residual row
__global__ void __launch_bounds__(256) pcg_jv_kernel(const PcgScalars* sc, int nrows, const PcgRowRec* rows,
                                                     const PcgKeyRec* keys, const double* jac, const double* v, double* y) {
  if (sc->done) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  const PcgRowRec R = rows[i];
  double s = 0;
  for (int k = R.k0; k < R.k1; ++k) {
    const PcgKeyRec K = keys[k];
    const double* a = jac + R.a0 + (i64)K.col * R.m;
    for (int c = 0; c < K.d; ++c) s += a[(i64)c * R.m] * v[K.toff + c];
  }
  y[i] = s;
}

// q_v = sum over the term list of A_fv' y_f (y == nullptr: of A_fv' b_f, the right-hand side J'b) + lambda D_v p_v, and the
// variable's share of p . q.  A wave per variable: lane = (g, c), component c of the terms g, g + G, g + 2G, ...
__global__ void __launch_bounds__(64) pcg_jty_kernel(const PcgScalars* sc, const PcgVarRec* vars, const PcgTermRec* terms,
                                                     const double* jac, const double* y, const double* p, const double* damp,
                                                     double lambda, double* q, double* var_partial) {
  if (sc->done) return;
  __shared__ double part[64];
  __shared__ double pq[kPcgMaxDim];
  const PcgVarRec V = vars[blockIdx.x];
  const int d = V.d, lane = threadIdx.x;
  const int G = 64 / d, c = lane % d, g = lane / d;
  double s = 0;
  if (g < G) {
    for (int t = V.t0 + g; t < V.t1; t += G) {
      const PcgTermRec T = terms[t];
      const double* a = jac + T.jac + (i64)(T.col + c) * T.m;
      if (y) {
        const double* yf = y + T.yoff;
        for (int r = 0; r < T.m; ++r) s += a[r] * yf[r];
      } else {
        const double* b = jac + T.jac + (i64)T.bcol * T.m;
        for (int r = 0; r < T.m; ++r) s += a[r] * b[r];
      }
    }
  }
  part[lane] = s;
  __syncthreads();
  if (lane < d) {
    double tot = 0;
    for (int k = 0; k < G; ++k) tot += part[k * d + lane];
    double pv = 0;
    if (p) {
      pv = p[V.toff + lane];
      tot += lambda * damp[V.toff + lane] * pv;
    }
    q[V.toff + lane] = tot;
    pq[lane] = pv * tot;
  }
  __syncthreads();
  if (lane == 0) {
    double tot = 0;
    for (int k = 0; k < d; ++k) tot += pq[k];
    var_partial[blockIdx.x] = tot;
  }
}

// alpha = gamma / (p . A p)
__global__ void __launch_bounds__(kRedThreads) pcg_alpha_kernel(PcgScalars* sc, const double* var_partial, int n_vars) {
  if (sc->done) return;
  const double s = block_sum(var_partial, n_vars);
  if (threadIdx.x != 0) return;
  sc->pAp = s;
  if ((!(s > 0.0) || !isfinite(s)) && sc->gamma > sc->threshold) {   // the system is not positive definite along p
    sc->fail = 1;
    sc->done = 1;
    return;
  }
  sc->alpha = sc->gamma / s;
}

// x += alpha p; q2 = L^-1 q; r -= alpha q2; the variable's share of r . r.  A thread per variable.
__global__ void __launch_bounds__(256) pcg_update1_kernel(const PcgScalars* sc, int n_vars, const PcgVarRec* vars,
                                                          const double* L, const double* p, const double* q, double* q2,
                                                          double* x, double* r, double* var_partial) {
  if (sc->done) return;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vars) return;
  const PcgVarRec V = vars[v];
  const int d = V.d;
  const double alpha = sc->alpha;
  p += V.toff, q += V.toff, q2 += V.toff, x += V.toff, r += V.toff;
  for (int i = 0; i < d; ++i) x[i] += alpha * p[i];
  if (L) {
    const double* Lv = L + V.lofs;
    for (int i = 0; i < d; ++i) {
      double s = q[i];
      for (int j = 0; j < i; ++j) s -= Lv[i + j * d] * q2[j];
      q2[i] = s / Lv[i + i * d];
    }
  } else {
    for (int i = 0; i < d; ++i) q2[i] = q[i];
  }
  double rr = 0;
  for (int i = 0; i < d; ++i) {
    const double ri = r[i] + (-alpha) * q2[i];
    r[i] = ri;
    rr += ri * ri;
  }
  var_partial[v] = rr;
}

// the reference's loop condition for iteration k (ConjugateGradientSolver.h:136)
__device__ bool pcg_goes_on(const PcgScalars* sc, int k, int max_it, int min_it) {
  return k <= max_it && (sc->gamma > sc->threshold || k <= min_it);
}

// gamma = r . r, beta = gamma / the previous gamma, k advances and the loop condition is evaluated for the next iteration
__global__ void __launch_bounds__(kRedThreads) pcg_beta_kernel(PcgScalars* sc, const double* var_partial, int n_vars,
                                                               int max_it, int min_it) {
  if (sc->done) return;
  const double s = block_sum(var_partial, n_vars);
  if (threadIdx.x != 0) return;
  const double prev = sc->gamma;
  sc->gamma = s;
  sc->beta = s / prev;
  sc->k += 1;   // iterations completed; the next one is k + 1
  if (!pcg_goes_on(sc, sc->k + 1, max_it, min_it)) sc->done = 1;
}

// q1 = L^-T r; p = q1 + beta p.  A thread per variable.
__global__ void __launch_bounds__(256) pcg_update2_kernel(const PcgScalars* sc, int n_vars, const PcgVarRec* vars,
                                                          const double* L, const double* r, double* q1, double* p) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vars) return;
  // (the iteration that set `done` still finishes its direction update in the reference; p is not an output, so nothing
  // is lost by leaving it)
  if (sc->done) return;
  const PcgVarRec V = vars[v];
  const int d = V.d;
  const double beta = sc->beta;
  r += V.toff, q1 += V.toff, p += V.toff;
  if (L) {
    const double* Lv = L + V.lofs;
    for (int i = d - 1; i >= 0; --i) {
      double s = r[i];
      for (int j = i + 1; j < d; ++j) s -= Lv[j + i * d] * q1[j];
      q1[i] = s / Lv[i + i * d];
    }
  } else {
    for (int i = 0; i < d; ++i) q1[i] = r[i];
  }
  for (int i = 0; i < d; ++i) p[i] = beta * p[i] + q1[i];
}

// the start and the restart (k % reset == 0): q1 = b - A x (Ax == nullptr: x = 0, q1 = b); r = L^-1 q1; p = L^-T r; the
// variable's share of r . r
__global__ void __launch_bounds__(256) pcg_residual_kernel(const PcgScalars* sc, int n_vars, const PcgVarRec* vars,
                                                           const double* L, const double* b, const double* Ax, double* q1,
                                                           double* r, double* p, double* var_partial) {
  if (sc->done) return;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vars) return;
  const PcgVarRec V = vars[v];
  const int d = V.d;
  b += V.toff, q1 += V.toff, r += V.toff, p += V.toff;
  if (Ax) Ax += V.toff;
  for (int i = 0; i < d; ++i) q1[i] = Ax ? b[i] - Ax[i] : b[i];
  double rr = 0;
  if (L) {
    const double* Lv = L + V.lofs;
    for (int i = 0; i < d; ++i) {
      double s = q1[i];
      for (int j = 0; j < i; ++j) s -= Lv[i + j * d] * r[j];
      r[i] = s / Lv[i + i * d];
    }
    for (int i = d - 1; i >= 0; --i) {
      double s = r[i];
      for (int j = i + 1; j < d; ++j) s -= Lv[j + i * d] * p[j];
      p[i] = s / Lv[i + i * d];
    }
  } else {
    for (int i = 0; i < d; ++i) p[i] = r[i] = q1[i];
  }
  for (int i = 0; i < d; ++i) rr += r[i] * r[i];
  var_partial[v] = rr;
}

// gamma = r . r after pcg_residual_kernel; first != 0: also gamma0, the threshold and the loop condition for k = 1
__global__ void __launch_bounds__(kRedThreads) pcg_gamma_kernel(PcgScalars* sc, const double* var_partial, int n_vars,
                                                                int first, double eps_rel, double eps_abs, int max_it,
                                                                int min_it) {
  if (sc->done) return;
  const double s = block_sum(var_partial, n_vars);
  if (threadIdx.x != 0) return;
  sc->gamma = s;
  if (!first) return;
  sc->gamma0 = s;
  sc->threshold = fmax(eps_abs, eps_rel * eps_rel * s);
  if (sc->bad_var != INT_MAX) {   // a diagonal block could not be factored
    sc->fail = 2;
    sc->done = 1;
    return;
  }
  if (!pcg_goes_on(sc, 1, max_it, min_it)) sc->done = 1;
}

}  // namespace

struct PcgWork {
  int n_vars = 0, n_rows = 0;
  i64 tan_size = 0, l_size = 0;
  PcgVarRec* vars = nullptr;
  PcgTermRec* terms = nullptr;
  PcgRowRec* rows = nullptr;
  PcgKeyRec* keys = nullptr;
  double *L = nullptr, *r = nullptr, *p = nullptr, *q = nullptr, *q2 = nullptr, *b = nullptr, *y = nullptr,
         *var_partial = nullptr;
  PcgScalars* sc = nullptr;
  PcgScalars* h_sc = nullptr;   // pinned
};

void pcg_work_destroy(PcgWork* w) {
  if (!w) return;
  void* dev[] = {w->vars, w->terms, w->rows, w->keys, w->L, w->r, w->p, w->q, w->q2, w->b, w->y, w->var_partial, w->sc};
  for (void* ptr : dev)
    if (ptr) (void)hipFree(ptr);
  if (w->h_sc) (void)hipHostFree(w->h_sc);
  delete w;
}

int pcg_max_dim(const HostProblem& P) {
  int m = 0;
  for (int v = 0; v < P.n_vars; ++v) m = std::max(m, P.dims[v]);
  return m;
}

template <class Tp>
static hipError_t pcg_upload(const std::vector<Tp>& v, Tp** out, hipStream_t st) {
  hipError_t e = hipMalloc((void**)out, std::max<size_t>(v.size(), 1) * sizeof(Tp));
  if (e != hipSuccess || v.empty()) return e;
  // (the vectors live until the synchronisation at the end of pcg_work_create)
  return hipMemcpyAsync(*out, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice, st);
}

hipError_t pcg_work_create(const HostProblem& P, hipStream_t st, PcgWork** out) {
  *out = nullptr;
  PcgWork* w = new PcgWork();
  w->n_vars = P.n_vars;
  w->tan_size = P.tan_size;
  std::vector<PcgVarRec> vars(P.n_vars);
  std::vector<PcgRowRec> rows;
  std::vector<PcgKeyRec> keys;
  std::vector<int> f_yoff(P.n_factors), count(P.n_vars + 1, 0);
  int nrows = 0;
  for (int f = 0; f < P.n_factors; ++f) {
    f_yoff[f] = nrows;
    const int k0 = (int)keys.size();
    int col = 0;
    for (int k = P.f_key_ptr[f]; k < P.f_key_ptr[f + 1]; ++k) {
      const int v = P.f_vars[k];
      keys.push_back(PcgKeyRec{col, P.tan_off[v], P.dims[v]});
      col += P.dims[v];
      count[v + 1]++;
    }
    for (int r = 0; r < P.f_rows[f]; ++r) rows.push_back(PcgRowRec{P.f_jac_off[f] + r, P.f_rows[f], k0, (int)keys.size(), 0});
    nrows += P.f_rows[f];
  }
  w->n_rows = nrows;
  for (int v = 0; v < P.n_vars; ++v) count[v + 1] += count[v];
  std::vector<PcgTermRec> terms(count[P.n_vars]);
  std::vector<int> fill(count.begin(), count.end() - 1);
  for (int f = 0; f < P.n_factors; ++f) {   // graph order: a variable's terms come in the order of its factors
    int col = 0;
    for (int k = P.f_key_ptr[f]; k < P.f_key_ptr[f + 1]; ++k) {
      const int v = P.f_vars[k];
      terms[fill[v]++] = PcgTermRec{P.f_jac_off[f], P.f_rows[f], col, f_yoff[f], P.f_cols[f] - 1};
      col += P.dims[v];
    }
  }
  i64 lofs = 0;
  for (int v = 0; v < P.n_vars; ++v) {
    vars[v] = PcgVarRec{lofs, P.tan_off[v], P.dims[v], count[v], count[v + 1]};
    lofs += (i64)P.dims[v] * P.dims[v];
  }
  w->l_size = lofs;
  hipError_t e = pcg_upload(vars, &w->vars, st);
  if (e == hipSuccess) e = pcg_upload(terms, &w->terms, st);
  if (e == hipSuccess) e = pcg_upload(rows, &w->rows, st);
  if (e == hipSuccess) e = pcg_upload(keys, &w->keys, st);
  const size_t nt = (size_t)std::max<i64>(P.tan_size, 1) * sizeof(double);
  double** vecs[] = {&w->r, &w->p, &w->q, &w->q2, &w->b};
  for (double** vp : vecs)
    if (e == hipSuccess) e = hipMalloc((void**)vp, nt);
  if (e == hipSuccess) e = hipMalloc((void**)&w->L, (size_t)std::max<i64>(lofs, 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->y, (size_t)std::max(nrows, 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->var_partial, (size_t)std::max(P.n_vars, 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&w->sc, sizeof(PcgScalars));
  if (e == hipSuccess) e = hipHostMalloc((void**)&w->h_sc, sizeof(PcgScalars));
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    pcg_work_destroy(w);
    return e;
  }
  *out = w;
  return hipSuccess;
}

hipError_t pcg_run(PcgWork* w, const double* jac, const double* damp, double lambda, const gsx_pcg_params& prm, double* x,
                   DevStatus* status, hipStream_t st, PcgScalars* out) {
  const int nv = w->n_vars, nr = w->n_rows;
  const int vb = (nv + 255) / 256, rb = (nr + 255) / 256;
  const int max_it = prm.max_iterations, min_it = prm.min_iterations;
  const double* L = prm.preconditioner == GSX_PRECOND_BLOCK_JACOBI ? w->L : nullptr;
  hipError_t e = hipMemsetAsync(x, 0, (size_t)w->tan_size * sizeof(double), st);
  if (e != hipSuccess) return e;
  pcg_begin_kernel<<<1, 1, 0, st>>>(w->sc, status);
  if (nv > 0) {
    if (L) pcg_build_blocks_kernel<<<nv, 64, 0, st>>>(w->sc, w->vars, w->terms, jac, damp, lambda, w->L, status);
    pcg_jty_kernel<<<nv, 64, 0, st>>>(w->sc, w->vars, w->terms, jac, nullptr, nullptr, damp, lambda, w->b, w->var_partial);
    pcg_residual_kernel<<<vb, 256, 0, st>>>(w->sc, nv, w->vars, L, w->b, nullptr, w->q, w->r, w->p, w->var_partial);
  }
  pcg_gamma_kernel<<<1, kRedThreads, 0, st>>>(w->sc, w->var_partial, nv, 1, prm.epsilon_rel, prm.epsilon_abs, max_it, min_it);
  // A p for p = v, into q (the shares of v . q go to var_partial)
  auto multiply = [&](const double* v) {
    if (nr > 0) pcg_jv_kernel<<<rb, 256, 0, st>>>(w->sc, nr, w->rows, w->keys, jac, v, w->y);
    pcg_jty_kernel<<<nv, 64, 0, st>>>(w->sc, w->vars, w->terms, jac, w->y, v, damp, lambda, w->q, w->var_partial);
  };
  int k = 1;
  for (;;) {
    for (int n = 0; n < kPcgBatch && k <= max_it && nv > 0; ++n, ++k) {
      if (k % prm.reset == 0) {   // restart from the true residual (the kernels look at `done` themselves)
        multiply(x);
        pcg_residual_kernel<<<vb, 256, 0, st>>>(w->sc, nv, w->vars, L, w->b, w->q, w->q2, w->r, w->p, w->var_partial);
        pcg_gamma_kernel<<<1, kRedThreads, 0, st>>>(w->sc, w->var_partial, nv, 0, 0.0, 0.0, max_it, min_it);
      }
      multiply(w->p);
      pcg_alpha_kernel<<<1, kRedThreads, 0, st>>>(w->sc, w->var_partial, nv);
      pcg_update1_kernel<<<vb, 256, 0, st>>>(w->sc, nv, w->vars, L, w->p, w->q, w->q2, x, w->r, w->var_partial);
      pcg_beta_kernel<<<1, kRedThreads, 0, st>>>(w->sc, w->var_partial, nv, max_it, min_it);
      pcg_update2_kernel<<<vb, 256, 0, st>>>(w->sc, nv, w->vars, L, w->r, w->q, w->p);
    }
    e = hipMemcpyAsync(w->h_sc, w->sc, sizeof(PcgScalars), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (w->h_sc->done || k > max_it || nv == 0) break;
  }
  *out = *w->h_sc;
  return hipSuccess;
}

}  // namespace gsx
