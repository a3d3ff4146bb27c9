// Element-wise kernels of the method of moving asymptotes (reference src/ParOptMMA.cpp:523-1010).
#include <math.h>

#include <type_traits>
#include <vector>

#include "core.hpp"
#include "mma.hpp"
#include "wcon.hpp"

namespace po {

#define PO_M_LOOP(i, n)                                                                   \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n);               \
       i += (int64_t)gridDim.x * blockDim.x)
#define PO_MLAUNCH(kernel, grid, ...)                                                     \
  do {                                                                                    \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, __VA_ARGS__);      \
    c->n_launches++;                                                                      \
    PO_HIP(hipGetLastError());                                                            \
  } while (0)

// asymptote update :615-651
__global__ void __launch_bounds__(kBlock)
    mma_asymptotes_kernel(const double *__restrict__ x, const double *__restrict__ x1,
                          const double *__restrict__ x2, const double *__restrict__ lb,
                          const double *__restrict__ ub, MmaParams p, int first, int64_t n,
                          double *__restrict__ L, double *__restrict__ U) {
  PO_M_LOOP(j, n) {
    const double xj = x[j];
    const double lower = fmax(lb[j], xj - p.movlim), upper = fmin(ub[j], xj + p.movlim);
    if (first) {
      L[j] = xj - p.init_off * (upper - lower);
      U[j] = xj + p.init_off * (upper - lower);
    } else {
      const double indc = (xj - x1[j]) * (x1[j] - x2[j]);
      const double Lprev = L[j], Uprev = U[j];
      double intrvl = fmax(upper - lower, 0.01);
      intrvl = fmin(intrvl, 100.0);
      double l, u;
      if (indc < 0.0) {
        l = xj - p.contract * (x1[j] - Lprev);
        u = xj + p.contract * (Uprev - x1[j]);
      } else {
        l = xj - p.relax * (x1[j] - Lprev);
        u = xj + p.relax * (Uprev - x1[j]);
      }
      l = fmin(l, xj - p.min_off * intrvl);
      u = fmax(u, xj + p.min_off * intrvl);
      l = fmax(l, xj - p.max_off * intrvl);
      u = fmin(u, xj + p.max_off * intrvl);
      L[j] = l;
      U[j] = u;
    }
  }
}
int k_mma_asymptotes(Ctx *c, const double *x, const double *x1, const double *x2, const double *lb,
                     const double *ub, const MmaParams &p, int first, int64_t n, double *L, double *U) {
  if (n <= 0) return PO_OK;
  PO_MLAUNCH(mma_asymptotes_kernel, grid_for(c, n), x, x1, x2, lb, ub, p, first, n, L, U);
  return PO_OK;
}

// move limits and objective coefficients :669-690
__global__ void __launch_bounds__(kBlock)
    mma_coef_kernel(const double *__restrict__ x, const double *__restrict__ lb, const double *__restrict__ ub,
                    const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ g,
                    MmaParams p, int64_t n, double *__restrict__ alpha, double *__restrict__ beta,
                    double *__restrict__ p0, double *__restrict__ q0) {
  PO_M_LOOP(j, n) {
    const double xj = x[j], Lj = L[j], Uj = U[j];
    const double lower = fmax(lb[j], xj - p.movlim), upper = fmin(ub[j], xj + p.movlim);
    alpha[j] = fmax(fmax(lower, 0.9 * Lj + 0.1 * xj), xj - 0.5 * (upper - lower));
    beta[j] = fmin(fmin(upper, 0.9 * Uj + 0.1 * xj), xj + 0.5 * (upper - lower));
    const double gpos = fmax(0.0, g[j]), gneg = fmax(0.0, -g[j]);
    p0[j] = (Uj - xj) * (Uj - xj) * ((1.0 + p.delta) * gpos + p.delta * gneg + p.eps / (Uj - Lj));
    q0[j] = (xj - Lj) * (xj - Lj) * ((1.0 + p.delta) * gneg + p.delta * gpos + p.eps / (Uj - Lj));
  }
}
int k_mma_coef(Ctx *c, const double *x, const double *lb, const double *ub, const double *L, const double *U,
               const double *g, const MmaParams &p, int64_t n, double *alpha, double *beta, double *p0,
               double *q0) {
  if (n <= 0) return PO_OK;
  PO_MLAUNCH(mma_coef_kernel, grid_for(c, n), x, lb, ub, L, U, g, p, n, alpha, beta, p0, q0);
  return PO_OK;
}

// constraint coefficients :692-712
__global__ void __launch_bounds__(kBlock)
    mma_pq_kernel(const double *__restrict__ x, const double *__restrict__ L, const double *__restrict__ U,
                  const double *__restrict__ A, int64_t n, double *__restrict__ pi, double *__restrict__ qi,
                  double *__restrict__ partials) {
  __shared__ double sm[4];
  double s = 0.0;
  PO_M_LOOP(j, n) {
    const double xj = x[j], du = U[j] - xj, dl = xj - L[j];
    const double gpos = fmax(0.0, -A[j]), gneg = fmax(0.0, A[j]);
    const double pv = du * du * gpos, qv = dl * dl * gneg;
    pi[j] = pv;
    qi[j] = qv;
    s += pv / du + qv / dl;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
int k_mma_pq(Ctx *c, const double *x, const double *L, const double *U, const double *A, int64_t n, double *pi,
             double *qi, double *bsum) {
  const int grid = grid_for(c, n);
  PO_TRY(ensure_partials(c, (size_t)grid));
  PO_MLAUNCH(mma_pq_kernel, grid, x, L, U, A, n, pi, qi, c->d_partials);
  return reduce_finish(c, grid, 1, 0, 0, bsum);
}

__global__ void __launch_bounds__(kBlock)
    mma_inv_kernel(const double *__restrict__ x, const double *__restrict__ L, const double *__restrict__ U,
                   int64_t n, double *__restrict__ uinv, double *__restrict__ linv) {
  PO_M_LOOP(j, n) {
    uinv[j] = 1.0 / (U[j] - x[j]);
    linv[j] = 1.0 / (x[j] - L[j]);
  }
}
int k_mma_inv(Ctx *c, const double *x, const double *L, const double *U, int64_t n, double *uinv, double *linv) {
  if (n <= 0) return PO_OK;
  PO_MLAUNCH(mma_inv_kernel, grid_for(c, n), x, L, U, n, uinv, linv);
  return PO_OK;
}

// gradients of the rational approximations :871-924, all constraints in one pass
__global__ void __launch_bounds__(kBlock)
    mma_grad_kernel(const double *__restrict__ x, const double *__restrict__ L, const double *__restrict__ U,
                    PtrTable P, PtrTable Q, int nv, int64_t n, PtrTableW out) {
  PO_M_LOOP(j, n) {
    const double ui = 1.0 / (U[j] - x[j]), li = 1.0 / (x[j] - L[j]);
    const double u2 = ui * ui, l2 = li * li;
    out.p[0][j] = u2 * P.p[0][j] - l2 * Q.p[0][j];
    for (int i = 1; i < nv; i++) out.p[i][j] = l2 * Q.p[i][j] - u2 * P.p[i][j];
  }
}
int k_mma_grad(Ctx *c, const double *x, const double *L, const double *U, const double *const *P,
               const double *const *Q, int nv, int64_t n, double *const *out) {
  if (n <= 0 || nv <= 0) return PO_OK;
  if (nv > kMaxPanel) {
    set_error("MMA: %d constraints exceed the panel width %d", nv - 1, kMaxPanel - 1);
    return PO_ERR_ARG;
  }
  PtrTable pt, qt;
  PtrTableW ot;
  for (int i = 0; i < kMaxPanel; i++) {
    pt.p[i] = i < nv ? P[i] : nullptr;
    qt.p[i] = i < nv ? Q[i] : nullptr;
    ot.p[i] = i < nv ? out[i] : nullptr;
  }
  PO_MLAUNCH(mma_grad_kernel, grid_for(c, n), x, L, U, pt, qt, nv, n, ot);
  return PO_OK;
}

// diagonal Hessian of the subproblem Lagrangian :967-1010
__global__ void __launch_bounds__(kBlock)
    mma_hdiag_kernel(const double *__restrict__ x, const double *__restrict__ L, const double *__restrict__ U,
                     PtrTable P, PtrTable Q, CoefTable w, int nv, int64_t n, double *__restrict__ h) {
  PO_M_LOOP(j, n) {
    const double ui = 1.0 / (U[j] - x[j]), li = 1.0 / (x[j] - L[j]);
    const double u3 = ui * ui * ui, l3 = li * li * li;
    double s = 0.0;
    for (int i = 0; i < nv; i++) s += 2.0 * w.a[i] * (u3 * P.p[i][j] + l3 * Q.p[i][j]);
    h[j] = s;
  }
}
int k_mma_hdiag(Ctx *c, const double *x, const double *L, const double *U, const double *const *P,
                const double *const *Q, const double *w, int nv, int64_t n, double *h) {
  if (n <= 0) return PO_OK;
  PtrTable pt, qt;
  CoefTable ct;
  for (int i = 0; i < kMaxPanel; i++) {
    pt.p[i] = i < nv ? P[i] : nullptr;
    qt.p[i] = i < nv ? Q[i] : nullptr;
    ct.a[i] = i < nv ? w[i] : 0.0;
  }
  PO_MLAUNCH(mma_hdiag_kernel, grid_for(c, n), x, L, U, pt, qt, ct, nv, n, h);
  return PO_OK;
}

// ---- the dual of the separable subproblem (Svanberg 1987, section 5; the subproblem of :523-1010) -----------------
// For 0 <= lambda <= gamma put P = p0 + sum_i lambda_i p_i, Q = q0 + sum_i lambda_i q_i (> 0).  The minimiser of the
// Lagrangian is x = clamp((sqrt(P) L + sqrt(Q) U) / (sqrt(P) + sqrt(Q)), alpha, beta), element by element, and with
// u = 1 / (U - x), l = 1 / (x - L):
//   W = sum P u + Q l (+ lambda.b on the host),  dW/dlambda_i = sum p_i u + q_i l (+ b_i),
//   -hess W = sum over the free elements (unclamped x strictly inside (alpha, beta)) of g_i g_k / h,
//   g_i = p_i u^2 - q_i l^2,  h = 2 (P u^3 + Q l^3).
// One pass, the primal point in registers.  Per element two square roots and four reciprocals (1 / (sqrt P + sqrt Q),
// u, l, 1 / h), each formed once.  The element past an odd length (all operands 0.0 there) takes u = l = 1 / h = 0, so
// that it adds an exact zero to every sum and its stores are zeros.
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f64x2 ld_nt(const double *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(p));
}
__device__ __forceinline__ void st_nt(double *p, f64x2 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<f64x2 *>(p));
}
__device__ __forceinline__ f64x2 fma2(double a, f64x2 v, f64x2 acc) {
  return (f64x2){fma(a, v.x, acc.x), fma(a, v.y, acc.y)};
}
// sum of the four products a.x b.x + c.x d.x + a.y b.y + c.y d.y on top of acc, in this fixed order
__device__ __forceinline__ double dot4(f64x2 a, f64x2 b, f64x2 c, f64x2 d, double acc) {
  return fma(a.x, b.x, fma(c.x, d.x, fma(a.y, b.y, fma(c.y, d.y, acc))));
}

struct DualPoint {
  f64x2 x, u, l, fr;  // fr: 1.0 where the element is free, else 0.0
};
__device__ __forceinline__ void dual_point1(double P, double Q, double L, double U, double a, double b, bool live,
                                            double &x, double &u, double &l, double &fr) {
  const double sp = sqrt(P), sq = sqrt(Q);
  const double r = 1.0 / (sp + sq);
  const double xs = fma(sp, L, sq * U) * r;
  fr = (live && xs > a && xs < b) ? 1.0 : 0.0;
  x = fmin(fmax(xs, a), b);
  u = live ? 1.0 / (U - x) : 0.0;
  l = live ? 1.0 / (x - L) : 0.0;
}
__device__ __forceinline__ DualPoint dual_point(f64x2 P, f64x2 Q, f64x2 L, f64x2 U, f64x2 a, f64x2 b, bool has2) {
  double x0, u0, l0, f0, x1, u1, l1, f1;
  dual_point1(P.x, Q.x, L.x, U.x, a.x, b.x, true, x0, u0, l0, f0);
  dual_point1(P.y, Q.y, L.y, U.y, a.y, b.y, has2, x1, u1, l1, f1);
  DualPoint t;
  t.x = (f64x2){x0, x1};
  t.u = (f64x2){u0, u1};
  t.l = (f64x2){l0, l1};
  t.fr = (f64x2){f0, f1};
  return t;
}
// P, Q += sum_{j <= i < j + B} lambda_i (p_i, q_i): 2 B loads in flight, issued back to back before their arithmetic
template <int B>
__device__ __forceinline__ void dual_pq_batch(const PtrTable &Pt, const PtrTable &Qt, const CoefTable &lam, int j,
                                              int64_t q, f64x2 &P, f64x2 &Q) {
  f64x2 pv[B], qv[B];
#pragma unroll
  for (int u = 0; u < B; u++) {
    pv[u] = ld_nt(Pt.p[j + u] + 2 * q);
    qv[u] = ld_nt(Qt.p[j + u] + 2 * q);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < B; u++) {
    P = fma2(lam.a[j + u], pv[u], P);
    Q = fma2(lam.a[j + u], qv[u], Q);
  }
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void dual_pq_all(const PtrTable &Pt, const PtrTable &Qt, const CoefTable &lam, int m,
                                            int64_t q, f64x2 &P, f64x2 &Q) {
  int j = 0;
  for (; j + 8 <= m; j += 8) dual_pq_batch<8>(Pt, Qt, lam, j, q, P, Q);
  if (j + 4 <= m) {
    dual_pq_batch<4>(Pt, Qt, lam, j, q, P, Q);
    j += 4;
  }
  if (j + 2 <= m) {
    dual_pq_batch<2>(Pt, Qt, lam, j, q, P, Q);
    j += 2;
  }
  if (j < m) dual_pq_batch<1>(Pt, Qt, lam, j, q, P, Q);
}

#ifndef PO_MMA_DUAL_HOLD
// widest column capacity whose pairs stay in registers (-DPO_MMA_DUAL_HOLD=8 for an A/B: at m = 16 / 32 the pass
// takes 0.92 / 7.5 ms with 32 and 1.37 / 11.6 ms with 8, n = 10 M / 50 M, profiles/r09_bench_mma_hold_ab.jsonl)
#define PO_MMA_DUAL_HOLD 32
#endif
template <int N>
__device__ __forceinline__ void dual_block_reduce(double (&a)[N], double *__restrict__ partials, double *sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double v = a[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sm[wave * N + j] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int j = threadIdx.x;
    partials[(size_t)j * gridDim.x + blockIdx.x] = (sm[j] + sm[N + j]) + (sm[2 * N + j] + sm[3 * N + j]);
  }
}

// MC: compile-time column capacity (m <= MC; the sums of the columns past m stay 0).  MC <= PO_MMA_DUAL_HOLD (32): the
// m column pairs of an element pair stay in registers between the formation of P, Q and the sums -- every stream is
// read once (MC = 32: 392-406 VGPRs, 408-428 in the rho form, one workgroup per CU, 64 loads of 16 B in flight per
// lane).  Wider: the columns come in batches of NVB = 8 pairs and are read a second time for the sums, right behind
// the first (the per-column accumulators are what fills the registers there).
// MODE 0: slots {W, g[MC]}; 1: ... and the MC (MC + 1) / 2 sums of -hess W (k-major lower triangle, i <= k);
// 2: slots as 0, and the columns G_i and the weights d = [free] / h are stored for the weighted Gram.
//
// RHO (mma_globalization = conservative): every approximation carries Svanberg's term rho_i d(x),
//   d(x) = sum (x - xk)^2 u l = sum w_U u + w_L l - 1,  w_U = (U - xk)^2 / (U - L),  w_L = (xk - L)^2 / (U - L),
// so the Lagrangian keeps its form with P = P0 + sigma w_U, Q = Q0 + sigma w_L (sigma = rho_0 + lambda . rho, added
// last; P0, Q0 the sums above).  One more stream (xk) and one more slot, D = d(x), the last one; slot 0 is taken on
// P0, Q0 (the host adds sigma D and rho_i D), the Hessian columns gain rho_i (w_U u^2 - w_L l^2) and h is taken on the
// full P, Q.  With every rho_i = 0 each added term is an exact zero: same bits as the plain form.
// MODE 3 (RHO only), the point pass of an inner iteration: x, zl, zu are stored and the slots are
// {Delta_0, Delta_i[MC], D}, Delta_i = sum p_i (u - u_k) + q_i (l - l_k) = f~_i(x) - f~_i(xk), with
// u - u_k = (x - xk) u u_k and l - l_k = -(x - xk) l l_k (no cancellation against n).
template <int MC, int MODE, bool RHO>
struct DualSlots {
  static constexpr int NH = MODE == 1 ? MC * (MC + 1) / 2 : 0;
  static constexpr int NS = 1 + MC + NH + (RHO ? 1 : 0);
};
template <int MC, int MODE, bool RHO>
__device__ __forceinline__ void dual_body(const double *__restrict__ L, const double *__restrict__ U,
                                          const double *__restrict__ alpha, const double *__restrict__ beta,
                                          const double *__restrict__ p0, const double *__restrict__ q0,
                                          const PtrTable &Pt, const PtrTable &Qt, const CoefTable &lam, int m,
                                          int64_t n,
                                          const PtrTableW &Gt, double *__restrict__ dout,
                                          double *__restrict__ partials, double *sm, int64_t qfirst, int64_t qstride,
                                          const double *__restrict__ xk,
                                          const CoefTable &rho, double sigma, double *__restrict__ xo,
                                          double *__restrict__ zlo, double *__restrict__ zuo) {
  constexpr bool HOLD = MC <= PO_MMA_DUAL_HOLD;
  constexpr bool POINT = MODE == 3;
  constexpr bool HESS = MODE == 1 || MODE == 2;
  constexpr int NVB = 8;
  constexpr int NS = DualSlots<MC, MODE, RHO>::NS;
  static_assert(MODE != 1 || MC <= kMmaDualFused, "the fused Hessian needs the columns in registers");
  static_assert(!POINT || RHO, "the point pass with sums belongs to the rho form");
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) acc[s] = 0.0;
  const int64_t npairs = (n + 1) >> 1;
  for (int64_t q = qfirst; q < npairs; q += qstride) {
    const bool has2 = 2 * q + 1 < n;
    const f64x2 Lv = ld_nt(L + 2 * q), Uv = ld_nt(U + 2 * q), av = ld_nt(alpha + 2 * q), bv = ld_nt(beta + 2 * q);
    f64x2 P = ld_nt(p0 + 2 * q), Q = ld_nt(q0 + 2 * q);
    f64x2 xkv = (f64x2){0.0, 0.0}, p0v = P, q0v = Q;
    if (RHO) xkv = ld_nt(xk + 2 * q);
    f64x2 pv[HOLD ? MC : 1], qv[HOLD ? MC : 1];
    if (HOLD) {
#pragma unroll
      for (int i = 0; i < MC; i++) {
        pv[i] = (f64x2){0.0, 0.0};
        qv[i] = (f64x2){0.0, 0.0};
        if (i < m) {
          pv[i] = ld_nt(Pt.p[i] + 2 * q);
          qv[i] = ld_nt(Qt.p[i] + 2 * q);
        }
      }
#pragma unroll
      for (int i = 0; i < MC; i++) {
        if (i < m) {
          P = fma2(lam.a[i], pv[i], P);
          Q = fma2(lam.a[i], qv[i], Q);
        }
      }
    } else {
      dual_pq_all(Pt, Qt, lam, m, q, P, Q);
    }
    const f64x2 P0s = P, Q0s = Q;
    f64x2 wU = (f64x2){0.0, 0.0}, wL = (f64x2){0.0, 0.0}, rs = (f64x2){0.0, 0.0}, dx = (f64x2){0.0, 0.0};
    if (RHO) {
      const f64x2 dU = Uv - xkv, dL = xkv - Lv;
      rs.x = 1.0 / (Uv.x - Lv.x);
      rs.y = has2 ? 1.0 / (Uv.y - Lv.y) : 0.0;
      wU = dU * dU * rs;
      wL = dL * dL * rs;
      P = fma2(sigma, wU, P);
      Q = fma2(sigma, wL, Q);
    }
    const DualPoint t = dual_point(P, Q, Lv, Uv, av, bv, has2);
    const f64x2 u2 = t.u * t.u, l2 = t.l * t.l;
    f64x2 su = t.u, sl = t.l;  // what the column sums are taken on
    if (RHO) {
      dx = t.x - xkv;
      if (!has2) dx.y = 0.0;
      const f64x2 ul = t.u * t.l;
      acc[NS - 1] = fma(dx.x * dx.x, ul.x, fma(dx.y * dx.y, ul.y, acc[NS - 1]));
      if (POINT) {
        f64x2 uk, lk;
        uk.x = 1.0 / (Uv.x - xkv.x);
        lk.x = 1.0 / (xkv.x - Lv.x);
        uk.y = has2 ? 1.0 / (Uv.y - xkv.y) : 0.0;
        lk.y = has2 ? 1.0 / (xkv.y - Lv.y) : 0.0;
        su = dx * t.u * uk;
        sl = -(dx * t.l * lk);
        const f64x2 ql = Q * l2;
        const f64x2 r = (f64x2){fma(P.x, u2.x, -ql.x), fma(P.y, u2.y, -ql.y)};
        f64x2 xs = t.x, lo, up;
        lo.x = t.x.x == av.x ? fmax(r.x, 0.0) : 0.0;
        up.x = t.x.x == bv.x ? fmax(-r.x, 0.0) : 0.0;
        lo.y = (has2 && t.x.y == av.y) ? fmax(r.y, 0.0) : 0.0;
        up.y = (has2 && t.x.y == bv.y) ? fmax(-r.y, 0.0) : 0.0;
        if (!has2) xs.y = 0.0;
        st_nt(xo + 2 * q, xs);
        st_nt(zlo + 2 * q, lo);
        st_nt(zuo + 2 * q, up);
      }
    }
    if (POINT) acc[0] = dot4(p0v, su, q0v, sl, acc[0]);
    else acc[0] = dot4(P0s, t.u, Q0s, t.l, acc[0]);
    f64x2 dw = (f64x2){0.0, 0.0}, gd = (f64x2){0.0, 0.0};
    if (HESS) {
      const f64x2 h = 2.0 * (P * (u2 * t.u) + Q * (l2 * t.l));
      dw.x = t.fr.x != 0.0 ? 1.0 / h.x : 0.0;
      dw.y = t.fr.y != 0.0 ? 1.0 / h.y : 0.0;
      if (MODE == 2) st_nt(dout + 2 * q, dw);
      // w_U u^2 - w_L l^2 = (a - b)(a + b) / (U - L) with a = (U - xk) u = 1 + dx u, b = (xk - L) l = 1 - dx l: the
      // derivative of d, which vanishes at xk -- taken in the form that does not cancel there
      if (RHO) gd = dx * (t.u + t.l) * (2.0 + dx * (t.u - t.l)) * rs;
    }
    if (HOLD) {
      f64x2 gv[HESS ? MC : 1];
#pragma unroll
      for (int i = 0; i < MC; i++) {
        acc[1 + i] = dot4(pv[i], su, qv[i], sl, acc[1 + i]);
        if (HESS) {
          const f64x2 ql = qv[i] * l2;
          gv[i] = (f64x2){fma(pv[i].x, u2.x, -ql.x), fma(pv[i].y, u2.y, -ql.y)};
          if (RHO) gv[i] = fma2(rho.a[i], gd, gv[i]);
          if (MODE == 2 && i < m) st_nt(Gt.p[i] + 2 * q, gv[i]);
        }
      }
      if (MODE == 1) {
#pragma unroll
        for (int k = 0; k < MC; k++) {
          const f64x2 gk = gv[k] * dw;
#pragma unroll
          for (int i = 0; i <= k; i++) {
            const int s = 1 + MC + k * (k + 1) / 2 + i;
            acc[s] = fma(gv[i].x, gk.x, fma(gv[i].y, gk.y, acc[s]));
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < MC; j += NVB) {
        if (j < m) {
          f64x2 cp[NVB], cq[NVB];
#pragma unroll
          for (int v = 0; v < NVB; v++) {
            cp[v] = (f64x2){0.0, 0.0};
            cq[v] = (f64x2){0.0, 0.0};
            if (j + v < m) {
              cp[v] = ld_nt(Pt.p[j + v] + 2 * q);
              cq[v] = ld_nt(Qt.p[j + v] + 2 * q);
            }
          }
#pragma unroll
          for (int v = 0; v < NVB; v++) {
            acc[1 + j + v] = dot4(cp[v], su, cq[v], sl, acc[1 + j + v]);
            if (MODE == 2 && j + v < m) {
              const f64x2 ql = cq[v] * l2;
              f64x2 gc = (f64x2){fma(cp[v].x, u2.x, -ql.x), fma(cp[v].y, u2.y, -ql.y)};
              if (RHO) gc = fma2(rho.a[j + v], gd, gc);
              st_nt(Gt.p[j + v] + 2 * q, gc);
            }
          }
        }
      }
    }
  }
  dual_block_reduce<NS>(acc, partials, sm);
}

template <int MC, int MODE>
__global__ void __launch_bounds__(kBlock)
    mma_dual_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                    const double *__restrict__ beta, const double *__restrict__ p0, const double *__restrict__ q0,
                    PtrTable Pt, PtrTable Qt, CoefTable lam, int m, int64_t n, PtrTableW Gt, double *__restrict__ dout,
                    double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, MODE, false>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  dual_body<MC, MODE, false>(L, U, alpha, beta, p0, q0, Pt, Qt, lam, m, n, Gt, dout, partials, sm, qfirst, qstride,
                             nullptr, lam, 0.0, nullptr, nullptr, nullptr);
}
// the rho form of the pass (modes 0, 1, 2)
template <int MC, int MODE>
__global__ void __launch_bounds__(kBlock)
    mma_dual_rho_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                        const double *__restrict__ beta, const double *__restrict__ p0, const double *__restrict__ q0,
                        const double *__restrict__ xk, PtrTable Pt, PtrTable Qt, CoefTable lam, CoefTable rho,
                        double sigma, int m, int64_t n, PtrTableW Gt, double *__restrict__ dout,
                        double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, MODE, true>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  dual_body<MC, MODE, true>(L, U, alpha, beta, p0, q0, Pt, Qt, lam, m, n, Gt, dout, partials, sm, qfirst, qstride,
                            xk, rho, sigma, nullptr, nullptr, nullptr);
}
// the point pass of an inner iteration: x, zl, zu and the m + 2 sums {Delta_0, Delta_i, D}; every stream read once
// (MC <= 32; wider, the columns a second time as in the pass above)
template <int MC>
__global__ void __launch_bounds__(kBlock)
    mma_gcmma_point_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                           const double *__restrict__ beta, const double *__restrict__ p0,
                           const double *__restrict__ q0, const double *__restrict__ xk, PtrTable Pt, PtrTable Qt,
                           CoefTable lam, double sigma, int m, int64_t n, double *__restrict__ x,
                           double *__restrict__ zl, double *__restrict__ zu, double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, 3, true>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  PtrTableW none = {};
  dual_body<MC, 3, true>(L, U, alpha, beta, p0, q0, Pt, Qt, lam, m, n, none, nullptr, partials, sm, qfirst, qstride,
                         xk, lam, sigma, x, zl, zu);
}

// the start values of rho: slots {sum |g| (U - L), sum |A_i| (U - L)}, one read-only pass
template <int MC>
__global__ void __launch_bounds__(kBlock)
    mma_gcmma_rho_start_kernel(const double *__restrict__ L, const double *__restrict__ U,
                               const double *__restrict__ g, PtrTable At, int m, int64_t n,
                               double *__restrict__ partials) {
  constexpr int NVB = 8;
  constexpr int NS = 1 + MC;
  __shared__ double sm[4 * NS];
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) acc[s] = 0.0;
  const int64_t npairs = (n + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
    const f64x2 w = ld_nt(U + 2 * q) - ld_nt(L + 2 * q), gv = ld_nt(g + 2 * q);
    acc[0] = fma(fabs(gv.x), w.x, fma(fabs(gv.y), w.y, acc[0]));
#pragma unroll
    for (int j = 0; j < MC; j += NVB) {
      if (j < m) {
        f64x2 cv[NVB < MC ? NVB : MC];
#pragma unroll
        for (int v = 0; v < NVB && v < MC; v++) {
          cv[v] = (f64x2){0.0, 0.0};
          if (j + v < m) cv[v] = ld_nt(At.p[j + v] + 2 * q);
        }
#pragma unroll
        for (int v = 0; v < NVB && v < MC; v++)
          acc[1 + j + v] = fma(fabs(cv[v].x), w.x, fma(fabs(cv[v].y), w.y, acc[1 + j + v]));
      }
    }
  }
  dual_block_reduce<NS>(acc, partials, sm);
}

// one pass at the final lambda: x, and the bound multipliers zl = max(r, 0) where x = alpha, zu = max(-r, 0) where
// x = beta, r = P u^2 - Q l^2 (0 elsewhere)
__global__ void __launch_bounds__(kBlock)
    mma_dual_point_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                          const double *__restrict__ beta, const double *__restrict__ p0,
                          const double *__restrict__ q0, PtrTable Pt, PtrTable Qt, CoefTable lam, int m, int64_t n,
                          double *__restrict__ x, double *__restrict__ zl, double *__restrict__ zu) {
  const int64_t npairs = (n + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
    const bool has2 = 2 * q + 1 < n;
    const f64x2 Lv = ld_nt(L + 2 * q), Uv = ld_nt(U + 2 * q), av = ld_nt(alpha + 2 * q), bv = ld_nt(beta + 2 * q);
    f64x2 P = ld_nt(p0 + 2 * q), Q = ld_nt(q0 + 2 * q);
    dual_pq_all(Pt, Qt, lam, m, q, P, Q);
    const DualPoint t = dual_point(P, Q, Lv, Uv, av, bv, has2);
    const f64x2 ql = Q * (t.l * t.l), u2 = t.u * t.u;
    const f64x2 r = (f64x2){fma(P.x, u2.x, -ql.x), fma(P.y, u2.y, -ql.y)};
    f64x2 xo = t.x, lo, up;
    lo.x = t.x.x == av.x ? fmax(r.x, 0.0) : 0.0;
    up.x = t.x.x == bv.x ? fmax(-r.x, 0.0) : 0.0;
    lo.y = (has2 && t.x.y == av.y) ? fmax(r.y, 0.0) : 0.0;
    up.y = (has2 && t.x.y == bv.y) ? fmax(-r.y, 0.0) : 0.0;
    if (!has2) xo.y = 0.0;
    st_nt(x + 2 * q, xo);
    st_nt(zl + 2 * q, lo);
    st_nt(zu + 2 * q, up);
  }
}

static int dual_tables(const MmaDualData &s, const double *lambda, PtrTable *pt, PtrTable *qt, CoefTable *ct) {
  if (s.m < 0 || s.m > kMmaDualMax) {
    set_error("MMA dual: %d constraints outside 0..%d", s.m, kMmaDualMax);
    return PO_ERR_ARG;
  }
  for (int i = 0; i < kMaxPanel; i++) {
    pt->p[i] = i < s.m ? s.p[i] : nullptr;
    qt->p[i] = i < s.m ? s.q[i] : nullptr;
    ct->a[i] = i < s.m ? lambda[i] : 0.0;
  }
  return PO_OK;
}

// m -> the compile-time column capacity MC that covers it; f(std::integral_constant<int, MC>) launches
template <int V>
using Const = std::integral_constant<int, V>;
template <class F>
static int with_capacity(int m, F &&f) {
  if (m <= 2) return f(Const<2>{});
  if (m <= 4) return f(Const<4>{});
  if (m <= 8) return f(Const<8>{});
  if (m <= 16) return f(Const<16>{});
  if (m <= 32) return f(Const<32>{});
  if (m <= 64) return f(Const<64>{});
  return f(Const<96>{});
}
// sigma = rho_0 + lambda . rho and the table of rho_1..m
static double rho_tables(const MmaDualRho &r, int m, const double *lambda, CoefTable *rt) {
  double sigma = r.rho[0];
  for (int i = 0; i < kMaxPanel; i++) rt->a[i] = i < m ? r.rho[1 + i] : 0.0;
  for (int i = 0; i < m; i++) sigma += lambda[i] * r.rho[1 + i];
  return sigma;
}

int k_mma_dual(Ctx *c, const MmaDualData &s, const double *lambda, int form, double *W, double *grad, double *H,
               double *const *G, double *dvec, const MmaDualRho *r, double *D) {
  const int m = s.m;
  PtrTable pt, qt;
  CoefTable ct, rt;
  PO_TRY(dual_tables(s, lambda, &pt, &qt, &ct));
  if (form < 0 || form > 2 || (form == 1 && m > kMmaDualFused)) {
    set_error("MMA dual: the fused form covers at most %d constraints (%d given)", kMmaDualFused, m);
    return PO_ERR_ARG;
  }
  if (form != 0 && !H) form = 0;
  if (form == 2 && (!G || !dvec)) {
    set_error("MMA dual: the panel form needs its %d column vectors and the weight vector", m);
    return PO_ERR_ARG;
  }
  PtrTableW gt;
  for (int i = 0; i < kMaxPanel; i++) gt.p[i] = (form == 2 && i < m) ? G[i] : nullptr;
  const double sigma = r ? rho_tables(*r, m, lambda, &rt) : 0.0;
  count_bytes(c, 2 * m + 6 + (r ? 1 : 0) + (form == 2 ? m + 1 : 0), s.n);
  // (one grid for every form: the value and the gradient have the same bits whichever form computed them)
  const int grid = grid_for(c, s.n, kBpcPanel);
  int mc = 0, ns = 0;
  auto launch = [&](auto MC, auto MODE) -> int {
    constexpr int kMC = decltype(MC)::value, kMode = decltype(MODE)::value;
    if constexpr (kMode != 1 || kMC <= kMmaDualFused) {  // (form 1 past kMmaDualFused was refused above)
      mc = kMC;
      ns = r ? DualSlots<kMC, kMode, true>::NS : DualSlots<kMC, kMode, false>::NS;
      PO_TRY(ensure_partials(c, (size_t)grid * ns));
      if (r) {
        PO_MLAUNCH((mma_dual_rho_kernel<kMC, kMode>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, r->xk, pt, qt, ct,
                   rt, sigma, m, s.n, gt, dvec, c->d_partials);
      } else {
        PO_MLAUNCH((mma_dual_kernel<kMC, kMode>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, pt, qt, ct, m, s.n, gt,
                   dvec, c->d_partials);
      }
    }
    return PO_OK;
  };
  PO_TRY(with_capacity(m, [&](auto MC) {
    return form == 1 ? launch(MC, Const<1>{}) : form == 2 ? launch(MC, Const<2>{}) : launch(MC, Const<0>{});
  }));
  double sums[1 + 96 + 36 + 1];
  PO_TRY(reduce_finish(c, grid, ns, 0, 0, sums, true));
  double w = sums[0];
  if (r) {  // (exact zeros where rho = 0)
    const double d = sums[ns - 1];
    w += sigma * d;
    for (int i = 0; i < m; i++) sums[1 + i] += r->rho[1 + i] * d;
    if (D) *D = d;
  }
  for (int i = 0; i < m; i++) {
    w += lambda[i] * s.b[i];
    grad[i] = sums[1 + i] + s.b[i];
  }
  *W = w;
  if (form == 1) {
    for (int k = 0; k < m; k++)
      for (int i = 0; i <= k; i++) H[i + (size_t)m * k] = H[k + (size_t)m * i] = sums[1 + mc + k * (k + 1) / 2 + i];
  } else if (form == 2 && m > 0) {
    PO_TRY(k_wgram(c, dvec, G, m, s.n, H));
  }
  return PO_OK;
}

int k_mma_gcmma_point(Ctx *c, const MmaDualData &s, const MmaDualRho &r, const double *lambda, double *x, double *zl,
                      double *zu, double *sums) {
  const int m = s.m;
  PtrTable pt, qt;
  CoefTable ct, rt;
  PO_TRY(dual_tables(s, lambda, &pt, &qt, &ct));
  const double sigma = rho_tables(r, m, lambda, &rt);  // (the point pass takes no table of rho)
  count_bytes(c, 2 * m + 7 + 3, s.n);
  const int grid = grid_for(c, s.n, kBpcPanel);
  int ns = 0;
  PO_TRY(with_capacity(m, [&](auto MC) -> int {
    constexpr int kMC = decltype(MC)::value;
    ns = DualSlots<kMC, 3, true>::NS;
    PO_TRY(ensure_partials(c, (size_t)grid * ns));
    PO_MLAUNCH((mma_gcmma_point_kernel<kMC>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, r.xk, pt, qt, ct, sigma, m,
               s.n, x, zl, zu, c->d_partials);
    return PO_OK;
  }));
  double all[96 + 2];
  PO_TRY(reduce_finish(c, grid, ns, 0, 0, all, true));
  for (int i = 0; i <= m; i++) sums[i] = all[i];
  sums[m + 1] = all[ns - 1];
  return PO_OK;
}

int k_mma_gcmma_rho_sums(Ctx *c, const double *L, const double *U, const double *g, const double *const *A, int m,
                         int64_t n, double *sums) {
  if (m < 0 || m > kMmaDualMax) {
    set_error("MMA: %d constraints outside 0..%d", m, kMmaDualMax);
    return PO_ERR_ARG;
  }
  PtrTable at;
  for (int i = 0; i < kMaxPanel; i++) at.p[i] = i < m ? A[i] : nullptr;
  count_bytes(c, m + 3, n);
  const int grid = grid_for(c, n, kBpcPanel);
  int ns = 0;
  PO_TRY(with_capacity(m, [&](auto MC) -> int {
    constexpr int kMC = decltype(MC)::value;
    ns = 1 + kMC;  // (the kernel's own NS)
    PO_TRY(ensure_partials(c, (size_t)grid * ns));
    PO_MLAUNCH((mma_gcmma_rho_start_kernel<kMC>), grid, L, U, g, at, m, n, c->d_partials);
    return PO_OK;
  }));
  double all[96 + 1];
  PO_TRY(reduce_finish(c, grid, ns, 0, 0, all, true));
  for (int i = 0; i <= m; i++) sums[i] = all[i];
  return PO_OK;
}

int k_mma_dual_point(Ctx *c, const MmaDualData &s, const double *lambda, double *x, double *zl, double *zu) {
  PtrTable pt, qt;
  CoefTable ct;
  PO_TRY(dual_tables(s, lambda, &pt, &qt, &ct));
  if (s.n <= 0) return PO_OK;
  count_bytes(c, 2 * s.m + 6 + 3, s.n);
  PO_MLAUNCH(mma_dual_point_kernel, grid_for(c, s.n, kBpcPanel), s.L, s.U, s.alpha, s.beta, s.p0, s.q0, pt, qt, ct,
             s.m, s.n, x, zl, zu);
  return PO_OK;
}

}  // namespace po
