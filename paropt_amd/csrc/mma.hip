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
// the same quantities at a stored point x (the grouped dual: x comes from the group solve): free where x lies
// strictly inside (alpha, beta)
__device__ __forceinline__ DualPoint dual_point_at(f64x2 x, f64x2 L, f64x2 U, f64x2 a, f64x2 b, bool has2) {
  DualPoint t;
  t.x = x;
  t.u.x = 1.0 / (U.x - x.x);
  t.l.x = 1.0 / (x.x - L.x);
  t.u.y = has2 ? 1.0 / (U.y - x.y) : 0.0;
  t.l.y = has2 ? 1.0 / (x.y - L.y) : 0.0;
  t.fr.x = (x.x > a.x && x.x < b.x) ? 1.0 : 0.0;
  t.fr.y = (has2 && x.y > a.y && x.y < b.y) ? 1.0 : 0.0;
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
// MODE 4, the sums of the grouped dual: as 2, at the stored point xin instead of the closed form.
// MODE 5 (RHO only), the sums of the point pass at the stored point xin: slots as 3, read-only -- nothing is stored and
// P, Q are not formed.
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
                                          double *__restrict__ zlo, double *__restrict__ zuo,
                                          const double *__restrict__ xin = nullptr) {
  constexpr bool HOLD = MC <= PO_MMA_DUAL_HOLD;
  constexpr bool POINT = MODE == 3;
  constexpr bool PSUMS = POINT || MODE == 5;  // the slots {Delta_0, Delta_i, D}
  constexpr bool STORED = MODE == 4 || MODE == 5;
  constexpr bool PANEL = MODE == 2 || MODE == 4;
  constexpr bool HESS = MODE == 1 || PANEL;
  constexpr int NVB = 8;
  constexpr int NS = DualSlots<MC, MODE, RHO>::NS;
  static_assert(MODE != 1 || MC <= kMmaDualFused, "the fused Hessian needs the columns in registers");
  static_assert(!PSUMS || RHO, "the point pass with sums belongs to the rho form");
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
      if (MODE != 5) {
#pragma unroll
        for (int i = 0; i < MC; i++) {
          if (i < m) {
            P = fma2(lam.a[i], pv[i], P);
            Q = fma2(lam.a[i], qv[i], Q);
          }
        }
      }
    } else if (MODE != 5) {
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
    const DualPoint t = STORED ? dual_point_at(ld_nt(xin + 2 * q), Lv, Uv, av, bv, has2)
                               : dual_point(P, Q, Lv, Uv, av, bv, has2);
    const f64x2 u2 = t.u * t.u, l2 = t.l * t.l;
    f64x2 su = t.u, sl = t.l;  // what the column sums are taken on
    if (RHO) {
      dx = t.x - xkv;
      if (!has2) dx.y = 0.0;
      const f64x2 ul = t.u * t.l;
      acc[NS - 1] = fma(dx.x * dx.x, ul.x, fma(dx.y * dx.y, ul.y, acc[NS - 1]));
      if (PSUMS) {
        f64x2 uk, lk;
        uk.x = 1.0 / (Uv.x - xkv.x);
        lk.x = 1.0 / (xkv.x - Lv.x);
        uk.y = has2 ? 1.0 / (Uv.y - xkv.y) : 0.0;
        lk.y = has2 ? 1.0 / (xkv.y - Lv.y) : 0.0;
        su = dx * t.u * uk;
        sl = -(dx * t.l * lk);
      }
      if (POINT) {
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
    if (PSUMS) acc[0] = dot4(p0v, su, q0v, sl, acc[0]);
    else acc[0] = dot4(P0s, t.u, Q0s, t.l, acc[0]);
    f64x2 dw = (f64x2){0.0, 0.0}, gd = (f64x2){0.0, 0.0};
    if (HESS) {
      const f64x2 h = 2.0 * (P * (u2 * t.u) + Q * (l2 * t.l));
      dw.x = t.fr.x != 0.0 ? 1.0 / h.x : 0.0;
      dw.y = t.fr.y != 0.0 ? 1.0 / h.y : 0.0;
      if (PANEL) st_nt(dout + 2 * q, dw);
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
          if (PANEL && i < m) st_nt(Gt.p[i] + 2 * q, gv[i]);
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
            if (PANEL && j + v < m) {
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

// ---- host scaffolding of the dual passes --------------------------------------------------------------------------
static int check_m(int m, const char *who = "MMA dual") {
  if (m < 0 || m > kMmaDualMax) {
    set_error("%s: %d constraints outside 0..%d", who, m, kMmaDualMax);
    return PO_ERR_ARG;
  }
  return PO_OK;
}
// the first m entries from cols / values, null or 0.0 past them (Table: PtrTable or PtrTableW)
template <class Table, class P>
static Table ptr_table(P *const *cols, int m) {
  Table t;
  for (int i = 0; i < kMaxPanel; i++) t.p[i] = i < m ? cols[i] : nullptr;
  return t;
}
static CoefTable coef_table(const double *values, int m) {
  CoefTable t;
  for (int i = 0; i < kMaxPanel; i++) t.a[i] = i < m ? values[i] : 0.0;
  return t;
}
struct DualTables {  // of a rational subproblem at lambda
  PtrTable pt, qt;
  CoefTable ct;
};
static int dual_tables(const MmaDualData &s, const double *lambda, DualTables *t) {
  PO_TRY(check_m(s.m));
  *t = DualTables{ptr_table<PtrTable>(s.p, s.m), ptr_table<PtrTable>(s.q, s.m), coef_table(lambda, s.m)};
  return PO_OK;
}
// sigma = rho_0 + lambda . rho (the table of rho_1..m is coef_table(r.rho + 1, m))
static double rho_sigma(const MmaDualRho &r, int m, const double *lambda) {
  double sigma = r.rho[0];
  for (int i = 0; i < m; i++) sigma += lambda[i] * r.rho[1 + i];
  return sigma;
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
  return f(Const<kMaxPanel>{});
}
// the widest result of a reducing pass: the value, kMaxPanel columns or kMmaDualFused with their Hessian sums, and two
// slots behind them (D or the cap hits, the most steps)
constexpr int kFusedSums = kMmaDualFused * (kMmaDualFused + 1) / 2;
constexpr int kPassSlots = 1 + kMaxPanel + kFusedSums + 2;
struct PassShape {
  int mc = 0, ns = 0;  // the capacity that ran and its sum slots
};
// One reducing pass over n at the panel grid: slots(MC) sum slots and nmax maxima per workgroup, launch(MC, grid)
// writes them to c->d_partials, out[slots + nmax] receives them reduced; collective.
template <class Slots, class Launch>
static int reducing_pass(Ctx *c, int m, int64_t n, int nmax, Slots &&slots, Launch &&launch, double *out,
                         PassShape *shape) {
  const int grid = grid_for(c, n, kBpcPanel);
  PO_TRY(with_capacity(m, [&](auto MC) -> int {
    shape->mc = decltype(MC)::value;
    shape->ns = slots(MC);
    PO_TRY(ensure_partials(c, (size_t)grid * (shape->ns + nmax)));
    return launch(MC, grid);
  }));
  return reduce_finish(c, grid, shape->ns, 0, nmax, out, true);
}

// The forms of an evaluation (mma.hpp): 0 value and gradient, 1 the Hessian sums in the pass, 2 the panel form.
static int check_form(int *form, int m, const double *H) {
  if (*form < 0 || *form > 2 || (*form == 1 && m > kMmaDualFused)) {
    set_error("MMA dual: the fused form covers at most %d constraints (%d given)", kMmaDualFused, m);
    return PO_ERR_ARG;
  }
  if (*form != 0 && !H) *form = 0;
  return PO_OK;
}
// f(MC, MODE) with MODE = form at compile time, for the pairs that exist (check_form refused form 1 past kMmaDualFused)
template <class MC, class F>
static int with_form(int form, MC mc, F &&f) {
  auto guarded = [&](auto MODE) -> int {
    if constexpr (decltype(MODE)::value != 1 || MC::value <= kMmaDualFused) return f(mc, MODE);
    return PO_OK;
  };
  return form == 1 ? guarded(Const<1>{}) : form == 2 ? guarded(Const<2>{}) : guarded(Const<0>{});
}
// H from the pass: the fused sums behind the mc columns, or the weighted Gram of the panel form's columns
static int form_hessian(Ctx *c, int form, const double *sums, int mc, const double *dvec, const double *const *cols,
                        int m, int64_t n, double *H) {
  if (form == 1) {
    for (int k = 0; k < m; k++)
      for (int i = 0; i <= k; i++) H[i + (size_t)m * k] = H[k + (size_t)m * i] = sums[1 + mc + k * (k + 1) / 2 + i];
  } else if (form == 2 && m > 0) {
    PO_TRY(k_wgram(c, dvec, cols, m, n, H));
  }
  return PO_OK;
}

// the rho form's last slot d: the value gains sigma d, column i gains rho_i d (exact zeros where rho = 0)
static void apply_rho(double *sums, int ns, double sigma, const double *rho, int m, double *D) {
  const double d = sums[ns - 1];
  sums[0] += sigma * d;
  for (int i = 0; i < m; i++) sums[1 + i] += rho[1 + i] * d;
  if (D) *D = d;
}
// W = w + lambda . b and grad = sums_1..m + b of the rational dual
static void dual_value_grad(double w, const double *sums, const double *lambda, const double *b, int m, double *W,
                            double *grad) {
  for (int i = 0; i < m; i++) {
    w += lambda[i] * b[i];
    grad[i] = sums[1 + i] + b[i];
  }
  *W = w;
}
// {Delta_0..m, D}: the first m + 1 slots and the last one
static void copy_point_sums(const double *all, int ns, int m, double *sums) {
  for (int i = 0; i <= m; i++) sums[i] = all[i];
  sums[m + 1] = all[ns - 1];
}

int k_mma_dual(Ctx *c, const MmaDualData &s, const double *lambda, int form, double *W, double *grad, double *H,
               double *const *G, double *dvec, const MmaDualRho *r, double *D) {
  const int m = s.m;
  DualTables t;
  PO_TRY(dual_tables(s, lambda, &t));
  PO_TRY(check_form(&form, m, H));
  if (form == 2 && (!G || !dvec)) {
    set_error("MMA dual: the panel form needs its %d column vectors and the weight vector", m);
    return PO_ERR_ARG;
  }
  const PtrTableW gt = ptr_table<PtrTableW>(G, form == 2 ? m : 0);
  const CoefTable rt = r ? coef_table(r->rho + 1, m) : CoefTable();
  const double sigma = r ? rho_sigma(*r, m, lambda) : 0.0;
  count_bytes(c, 2 * m + 6 + (r ? 1 : 0) + (form == 2 ? m + 1 : 0), s.n);
  // (one grid for every form: the value and the gradient have the same bits whichever form computed them)
  const auto slots = [&](auto MC) {
    return with_form(form, MC, [&](auto MC_, auto MODE) -> int {
      constexpr int kMC = decltype(MC_)::value, kMode = decltype(MODE)::value;
      return r ? DualSlots<kMC, kMode, true>::NS : DualSlots<kMC, kMode, false>::NS;
    });
  };
  const auto launch = [&](auto MC, int grid) {
    return with_form(form, MC, [&](auto MC_, auto MODE) -> int {
      constexpr int kMC = decltype(MC_)::value, kMode = decltype(MODE)::value;
      if (r) {
        PO_MLAUNCH((mma_dual_rho_kernel<kMC, kMode>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, r->xk, t.pt, t.qt,
                   t.ct, rt, sigma, m, s.n, gt, dvec, c->d_partials);
      } else {
        PO_MLAUNCH((mma_dual_kernel<kMC, kMode>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, t.pt, t.qt, t.ct, m, s.n,
                   gt, dvec, c->d_partials);
      }
      return PO_OK;
    });
  };
  double sums[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(c, m, s.n, 0, slots, launch, sums, &sh));
  if (r) apply_rho(sums, sh.ns, sigma, r->rho, m, D);
  dual_value_grad(sums[0], sums, lambda, s.b, m, W, grad);
  return form_hessian(c, form, sums, sh.mc, dvec, G, m, s.n, H);
}

int k_mma_gcmma_point(Ctx *c, const MmaDualData &s, const MmaDualRho &r, const double *lambda, double *x, double *zl,
                      double *zu, double *sums) {
  const int m = s.m;
  DualTables t;
  PO_TRY(dual_tables(s, lambda, &t));
  const double sigma = rho_sigma(r, m, lambda);  // (the point pass takes no table of rho)
  count_bytes(c, 2 * m + 7 + 3, s.n);
  double all[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(
      c, m, s.n, 0, [](auto MC) { return DualSlots<decltype(MC)::value, 3, true>::NS; },
      [&](auto MC, int grid) -> int {
        PO_MLAUNCH((mma_gcmma_point_kernel<decltype(MC)::value>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, r.xk,
                   t.pt, t.qt, t.ct, sigma, m, s.n, x, zl, zu, c->d_partials);
        return PO_OK;
      },
      all, &sh));
  copy_point_sums(all, sh.ns, m, sums);
  return PO_OK;
}

int k_mma_gcmma_rho_sums(Ctx *c, const double *L, const double *U, const double *g, const double *const *A, int m,
                         int64_t n, double *sums) {
  PO_TRY(check_m(m, "MMA"));
  const PtrTable at = ptr_table<PtrTable>(A, m);
  count_bytes(c, m + 3, n);
  double all[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(
      c, m, n, 0, [](auto MC) { return 1 + decltype(MC)::value; },  // (the kernel's own NS)
      [&](auto MC, int grid) -> int {
        PO_MLAUNCH((mma_gcmma_rho_start_kernel<decltype(MC)::value>), grid, L, U, g, at, m, n, c->d_partials);
        return PO_OK;
      },
      all, &sh));
  for (int i = 0; i <= m; i++) sums[i] = all[i];
  return PO_OK;
}

int k_mma_dual_point(Ctx *c, const MmaDualData &s, const double *lambda, double *x, double *zl, double *zu) {
  DualTables t;
  PO_TRY(dual_tables(s, lambda, &t));
  if (s.n <= 0) return PO_OK;
  count_bytes(c, 2 * s.m + 6 + 3, s.n);
  PO_MLAUNCH(mma_dual_point_kernel, grid_for(c, s.n, kBpcPanel), s.L, s.U, s.alpha, s.beta, s.p0, s.q0, t.pt, t.qt,
             t.ct, s.m, s.n, x, zl, zu);
  return PO_OK;
}

// ---- grouped sparse constraints in the dual (mma.hpp) ----------------------------------------------------------------
// the sums at the stored point: the panel form of the pass above with x loaded
template <int MC>
__global__ void __launch_bounds__(kBlock)
    mma_dual_stored_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                           const double *__restrict__ beta, const double *__restrict__ p0,
                           const double *__restrict__ q0, const double *__restrict__ x, PtrTable Pt, PtrTable Qt,
                           CoefTable lam, int m, int64_t n, PtrTableW Gt, double *__restrict__ dout,
                           double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, 4, false>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  dual_body<MC, 4, false>(L, U, alpha, beta, p0, q0, Pt, Qt, lam, m, n, Gt, dout, partials, sm, qfirst, qstride,
                          nullptr, lam, 0.0, nullptr, nullptr, nullptr, x);
}
// ... in the rho form: slot 0 on P0, Q0, the columns with rho_i times the derivative of d, h on the full P, Q, and D
template <int MC>
__global__ void __launch_bounds__(kBlock)
    mma_dual_stored_rho_kernel(const double *__restrict__ L, const double *__restrict__ U,
                               const double *__restrict__ alpha, const double *__restrict__ beta,
                               const double *__restrict__ p0, const double *__restrict__ q0,
                               const double *__restrict__ xk, const double *__restrict__ x, PtrTable Pt, PtrTable Qt,
                               CoefTable lam, CoefTable rho, double sigma, int m, int64_t n, PtrTableW Gt,
                               double *__restrict__ dout, double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, 4, true>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  dual_body<MC, 4, true>(L, U, alpha, beta, p0, q0, Pt, Qt, lam, m, n, Gt, dout, partials, sm, qfirst, qstride, xk,
                         rho, sigma, nullptr, nullptr, nullptr, x);
}
// the sums {Delta_0, Delta_i, D} of a conservative trial at the stored point: read-only, once per trial
template <int MC>
__global__ void __launch_bounds__(kBlock)
    mma_gcmma_group_sums_kernel(const double *__restrict__ L, const double *__restrict__ U,
                                const double *__restrict__ p0, const double *__restrict__ q0,
                                const double *__restrict__ xk, const double *__restrict__ x, PtrTable Pt, PtrTable Qt,
                                int m, int64_t n, double *__restrict__ partials) {
  __shared__ double sm[4 * DualSlots<MC, 5, true>::NS];
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  PtrTableW none = {};
  CoefTable zero = {};
  // (the move limits only decide [free], which no slot of this mode takes: L, U stand in for them)
  dual_body<MC, 5, true>(L, U, L, U, p0, q0, Pt, Qt, zero, m, n, none, nullptr, partials, sm, qfirst, qstride, xk,
                         zero, 0.0, nullptr, nullptr, nullptr, x);
}

// sum of nw consecutive LDS values in index order (row_sum of wcon.hip)
__device__ __forceinline__ double row_sum_lds(const double *row, int nw) {
  double sacc = 0.0;
  int k = 0;
  for (; k + 4 <= nw; k += 4) {
    const double a = row[k], b = row[k + 1], c = row[k + 2], e = row[k + 3];
    sacc += a;
    sacc += b;
    sacc += c;
    sacc += e;
  }
  for (; k < nw; k++) sacc += row[k];
  return sacc;
}
// One element of a group: phi'(x) = P u^2 - Q l^2 is increasing on (L, U); ga, gb are its values at alpha and beta.
struct GroupEl {
  double P, Q, L, U, a, b, ga, gb;
};
__device__ __forceinline__ double group_phi1(double P, double Q, double L, double U, double x) {
  const double u = 1.0 / (U - x), l = 1.0 / (x - L);
  const double ql = Q * (l * l);
  return fma(P, u * u, -ql);
}
// clamp(root of phi'(x) = t, alpha, beta) by a bracketed Newton iteration from x0: a step that leaves the bracket is
// replaced by its midpoint; it ends when the iterate or the bracket stops moving.  *capped is raised at the step cap.
// RHO: it also ends when the step changes neither U - x nor x - L.  Where |x| is far below |L|, |U| a step of one ulp
// of x is below the resolution of both differences: phi' keeps its value (a rounding residue of P u^2 - Q l^2, which
// sigma makes large), the step keeps its size, and x creeps one ulp at a time into the cap.  The plain form keeps its
// stop test, and with it its bits.
// `steps` receives the evaluations of phi' the search took (0 on a move limit).
// EARLY: a Newton step below the resolution of x ends the search at once.  Without it such a step is first tested
// against the bracket, whose end x itself has just become: it counts as having left the bracket, and where the
// iterates came from one side only the far end is still a move limit, so the search goes on by bisection from there
// (some 50 more steps, seen on a fifth of the free elements).  The grouped kernels keep that order, and their bits.
template <bool RHO, bool EARLY = false>
__device__ __forceinline__ double group_el_root_steps(const GroupEl &e, double t, double x0, int &capped, int &steps) {
  steps = 0;
  if (!(t > e.ga)) return e.a;
  if (!(t < e.gb)) return e.b;
  double lo = e.a, hi = e.b, x = x0;
  if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
  int it = 0;
  for (; it < kGroupNewtonCap; it++) {
    const double u = 1.0 / (e.U - x), l = 1.0 / (x - e.L);
    const double u2 = u * u, l2 = l * l;
    const double f = fma(e.P, u2, -(e.Q * l2)) - t;
    const double h = 2.0 * (e.P * (u2 * u) + e.Q * (l2 * l));
    if (f < 0.0) lo = x;
    else if (f > 0.0) hi = x;
    else break;
    double xn = x - f / h;
    if (EARLY && xn == x) break;
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    if (!(xn > lo && xn < hi) || xn == x) break;
    if (RHO && e.U - xn == e.U - x && xn - e.L == x - e.L) break;
    x = xn;
  }
  if (it == kGroupNewtonCap) capped++;
  steps = it == kGroupNewtonCap ? it : it + 1;
  return x;
}
template <bool RHO>
__device__ __forceinline__ double group_el_root(const GroupEl &e, double t, double x0, int &capped) {
  int steps;
  return group_el_root_steps<RHO>(e, t, x0, capped, steps);
}
// the closed form of the plain dual (dual_point1: same expressions, same bits)
__device__ __forceinline__ double group_closed_form(double P, double Q, double L, double U, double a, double b) {
  const double sp = sqrt(P), sq = sqrt(Q);
  const double r = 1.0 / (sp + sq);
  const double xs = fma(sp, L, sq * U) * r;
  return fmin(fmax(xs, a), b);
}
// P, Q of the element at index i, in the fma order of dual_pq_all (four column pairs requested together)
__device__ __forceinline__ void group_pq(const double *__restrict__ p0, const double *__restrict__ q0,
                                         const PtrTable &Pt, const PtrTable &Qt, const CoefTable &lam, int m,
                                         int64_t i, double &P, double &Q) {
  P = __builtin_nontemporal_load(p0 + i);
  Q = __builtin_nontemporal_load(q0 + i);
  int j = 0;
  for (; j + 4 <= m; j += 4) {
    const double a0 = __builtin_nontemporal_load(Pt.p[j] + i), a1 = __builtin_nontemporal_load(Pt.p[j + 1] + i),
                 a2 = __builtin_nontemporal_load(Pt.p[j + 2] + i), a3 = __builtin_nontemporal_load(Pt.p[j + 3] + i);
    const double b0 = __builtin_nontemporal_load(Qt.p[j] + i), b1 = __builtin_nontemporal_load(Qt.p[j + 1] + i),
                 b2 = __builtin_nontemporal_load(Qt.p[j + 2] + i), b3 = __builtin_nontemporal_load(Qt.p[j + 3] + i);
    P = fma(lam.a[j], a0, P);
    Q = fma(lam.a[j], b0, Q);
    P = fma(lam.a[j + 1], a1, P);
    Q = fma(lam.a[j + 1], b1, Q);
    P = fma(lam.a[j + 2], a2, P);
    Q = fma(lam.a[j + 2], b2, Q);
    P = fma(lam.a[j + 3], a3, P);
    Q = fma(lam.a[j + 3], b3, Q);
  }
  for (; j < m; j++) {
    const double a0 = __builtin_nontemporal_load(Pt.p[j] + i), b0 = __builtin_nontemporal_load(Qt.p[j] + i);
    P = fma(lam.a[j], a0, P);
    Q = fma(lam.a[j], b0, Q);
  }
}
// the rho form (dual_body, RHO): P, Q of the element at index i gain sigma (w_U, w_L) -- the same expressions
__device__ __forceinline__ void group_pq_rho(const double *__restrict__ xk, double sigma, double L, double U,
                                             int64_t i, double &P, double &Q) {
  const double xkv = __builtin_nontemporal_load(xk + i);
  const double dU = U - xkv, dL = xkv - L;
  const double rs = 1.0 / (U - L);
  const double wU = dU * dU * rs, wL = dL * dL * rs;
  P = fma(sigma, wU, P);
  Q = fma(sigma, wL, Q);
}
// x, and with zl != nullptr the bound multipliers, of an element whose multiplier term is t (0 outside the groups)
__device__ __forceinline__ void group_store(const GroupEl &e, double x, double t, int64_t i, double *__restrict__ xo,
                                            double *__restrict__ zl, double *__restrict__ zu) {
  xo[i] = x;
  if (zl) {
    const double r = group_phi1(e.P, e.Q, e.L, e.U, x) - t;
    zl[i] = x == e.a ? fmax(r, 0.0) : 0.0;
    zu[i] = x == e.b ? fmax(-r, 0.0) : 0.0;
  }
}
// {sum zw psi, strict, at zlo, at gamma, cap hits, steps}, {most steps of a group, |psi| strict}
constexpr int kGroupSums = 6, kGroupMaxs = 2;
// The group solve.  A workgroup owns a tile of G whole periods (G period <= kGroupTile): lane <-> variable, two
// variables per lane, P and Q in registers for the whole tile.  Every round the lanes of the unfinished groups solve
// their elements at the group's current zw and put x and [free] / h into LDS (rows of the padded stride of wcon.hip);
// one thread per group takes the two row sums, psi = a sum x + c and psi' = a^2 sum [free] / h, and moves zw: Newton
// inside the bracket [lo, hi], whose upper end gamma is evaluated only when a step reaches it; the midpoint when the
// step leaves the bracket.  The rounds end when every group of the tile has ended.  Variables before `start`, in the
// gaps between the groups and behind the last period take the closed form.
// RHO: the conservative approximations around xk -- P, Q gain sigma (w_U, w_L) once, right after they are formed (one
// more stream); everything downstream takes the full P, Q.  The groups themselves are affine and carry no rho.
template <bool RHO>
__global__ void __launch_bounds__(kBlock)
    mma_group_solve_kernel(GroupMap gm, double ga, const double *__restrict__ cvec, int64_t nwineq, double gamma,
                           const double *__restrict__ L, const double *__restrict__ U,
                           const double *__restrict__ alpha, const double *__restrict__ beta,
                           const double *__restrict__ p0, const double *__restrict__ q0, PtrTable Pt, PtrTable Qt,
                           CoefTable lam, int m, int64_t n, int G, int64_t ntiles, double *__restrict__ xo,
                           double *__restrict__ zwo, double *__restrict__ zl, double *__restrict__ zu,
                           double *__restrict__ partials, const double *__restrict__ xk, double sigma) {
  __shared__ double smx[kGroupTile + kBlock], smd[kGroupTile + kBlock];
  __shared__ double sz[kBlock];
  __shared__ int sdone[kBlock];
  __shared__ double red[4 * (kGroupSums + kGroupMaxs)];
  const int period = gm.nw + gm.skip;
  const int pad = (period & 1) ? 0 : 1, rstride = period + pad;
  const int tid = threadIdx.x;
  const int gi0 = tid / period, k0 = tid - gi0 * period;
  const int gi1 = (tid + kBlock) / period, k1 = tid + kBlock - gi1 * period;
  const int s0 = tid + pad * gi0, s1 = tid + kBlock + pad * gi1;
  const int64_t span = gm.start + gm.nwcon * (int64_t)period;
  const int64_t cover_end = span < n ? span : n;
  double acc_zp = 0.0, acc_strict = 0.0, acc_lo = 0.0, acc_gam = 0.0, acc_psi = 0.0, acc_steps = 0.0;
  int capped = 0, most = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t g0 = tile * G;
    const int ng = (int)((gm.nwcon - g0) < G ? (gm.nwcon - g0) : G);
    const int64_t v0 = gm.start + g0 * (int64_t)period;
    int64_t vend = v0 + (int64_t)ng * period;
    if (vend > n) vend = n;
    const int nvv = (int)(vend - v0);
    const bool in0 = tid < nvv, in1 = tid + kBlock < nvv;
    const bool grp0 = in0 && k0 < gm.nw, grp1 = in1 && k1 < gm.nw;
    const int64_t i0 = v0 + (in0 ? tid : 0), i1 = v0 + (in1 ? tid + kBlock : 0);
    GroupEl e0, e1;
    e0.L = __builtin_nontemporal_load(L + i0);
    e1.L = __builtin_nontemporal_load(L + i1);
    e0.U = __builtin_nontemporal_load(U + i0);
    e1.U = __builtin_nontemporal_load(U + i1);
    e0.a = __builtin_nontemporal_load(alpha + i0);
    e1.a = __builtin_nontemporal_load(alpha + i1);
    e0.b = __builtin_nontemporal_load(beta + i0);
    e1.b = __builtin_nontemporal_load(beta + i1);
    group_pq(p0, q0, Pt, Qt, lam, m, i0, e0.P, e0.Q);
    group_pq(p0, q0, Pt, Qt, lam, m, i1, e1.P, e1.Q);
    if (RHO) {
      group_pq_rho(xk, sigma, e0.L, e0.U, i0, e0.P, e0.Q);
      group_pq_rho(xk, sigma, e1.L, e1.U, i1, e1.P, e1.Q);
    }
    // the closed form: the point of every element at zw = 0, and the start of the root searches
    const double xc0 = group_closed_form(e0.P, e0.Q, e0.L, e0.U, e0.a, e0.b);
    const double xc1 = group_closed_form(e1.P, e1.Q, e1.L, e1.U, e1.a, e1.b);
    double x0 = xc0, x1 = xc1, t0 = 0.0, t1 = 0.0;
    e0.ga = e0.gb = e1.ga = e1.gb = 0.0;
    if (grp0) {
      e0.ga = group_phi1(e0.P, e0.Q, e0.L, e0.U, e0.a);
      e0.gb = group_phi1(e0.P, e0.Q, e0.L, e0.U, e0.b);
    }
    if (grp1) {
      e1.ga = group_phi1(e1.P, e1.Q, e1.L, e1.U, e1.a);
      e1.gb = group_phi1(e1.P, e1.Q, e1.L, e1.U, e1.b);
    }
    // the state of group g0 + tid
    const bool mine = tid < ng;
    const double zlo = (mine && g0 + tid >= nwineq) ? -gamma : 0.0;
    const double cg = mine ? cvec[g0 + tid] : 0.0;
    double zw = zlo, lo = zlo, hi = gamma, psi = 0.0;
    bool hik = false, active = mine;
    int steps = 0;
    if (mine) {
      sz[tid] = zw;
      sdone[tid] = 0;
    }
    __syncthreads();
    for (;;) {
      if (grp0 && !sdone[gi0]) {
        t0 = ga * sz[gi0];
        x0 = t0 == 0.0 ? xc0 : group_el_root<RHO>(e0, t0, x0, capped);
        const double u = 1.0 / (e0.U - x0), l = 1.0 / (x0 - e0.L);
        smx[s0] = x0;
        smd[s0] = (x0 > e0.a && x0 < e0.b) ? 1.0 / (2.0 * (e0.P * (u * u * u) + e0.Q * (l * l * l))) : 0.0;
      }
      if (grp1 && !sdone[gi1]) {
        t1 = ga * sz[gi1];
        x1 = t1 == 0.0 ? xc1 : group_el_root<RHO>(e1, t1, x1, capped);
        const double u = 1.0 / (e1.U - x1), l = 1.0 / (x1 - e1.L);
        smx[s1] = x1;
        smd[s1] = (x1 > e1.a && x1 < e1.b) ? 1.0 / (2.0 * (e1.P * (u * u * u) + e1.Q * (l * l * l))) : 0.0;
      }
      __syncthreads();
      if (active) {
        const double sx = row_sum_lds(smx + tid * rstride, gm.nw), sd = row_sum_lds(smd + tid * rstride, gm.nw);
        psi = fma(ga, sx, cg);
        steps++;
        if ((zw == zlo && psi >= 0.0) || (zw == gamma && psi <= 0.0) || psi == 0.0) {
          active = false;
        } else {
          if (psi < 0.0) {
            lo = zw;
          } else {
            hi = zw;
            hik = true;
          }
          double zn = sd > 0.0 ? zw - psi / (ga * ga * sd) : hi;
          if (!(zn > lo && zn < hi)) zn = hik ? 0.5 * (lo + hi) : gamma;
          if ((hik && !(zn > lo && zn < hi)) || zn == zw) {
            active = false;
          } else if (steps >= kGroupNewtonCap) {
            active = false;
            capped++;
          } else {
            zw = zn;
            sz[tid] = zw;
          }
        }
        if (!active) sdone[tid] = 1;
      }
      if (!__syncthreads_or(active ? 1 : 0)) break;
    }
    if (mine) {
      zwo[g0 + tid] = zw;
      acc_zp = fma(zw, psi, acc_zp);
      const bool strict = zw > zlo && zw < gamma;
      if (strict) {
        acc_strict += 1.0;
        acc_psi = fmax(acc_psi, fabs(psi));
      } else if (zw < gamma) {
        acc_lo += 1.0;
      } else {
        acc_gam += 1.0;
      }
      most = steps > most ? steps : most;
      acc_steps += (double)steps;
    }
    if (in0) group_store(e0, x0, grp0 ? t0 : 0.0, i0, xo, zl, zu);
    if (in1) group_store(e1, x1, grp1 ? t1 : 0.0, i1, xo, zl, zu);
  }
  // variables outside every period: the closed form
  const int64_t nout = gm.start + (n - cover_end);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + tid; i < nout; i += (int64_t)gridDim.x * kBlock) {
    const int64_t g = i < gm.start ? i : cover_end + (i - gm.start);
    GroupEl e;
    e.L = L[g];
    e.U = U[g];
    e.a = alpha[g];
    e.b = beta[g];
    e.ga = e.gb = 0.0;
    group_pq(p0, q0, Pt, Qt, lam, m, g, e.P, e.Q);
    if (RHO) group_pq_rho(xk, sigma, e.L, e.U, g, e.P, e.Q);
    group_store(e, group_closed_form(e.P, e.Q, e.L, e.U, e.a, e.b), 0.0, g, xo, zl, zu);
  }
  if ((n & 1) && blockIdx.x == 0 && tid == 0) {  // the pad element of an odd length stays zero
    xo[n] = 0.0;
    if (zl) zl[n] = zu[n] = 0.0;
  }
  // the sums and maxima of the workgroup, in a fixed order
  double v[kGroupSums + kGroupMaxs] = {acc_zp,        acc_strict, acc_lo, acc_gam, (double)capped, acc_steps,
                                       (double)most, acc_psi};
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < kGroupSums + kGroupMaxs; j++) {
    double r = v[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double other = __shfl_xor(r, o, 64);
      r = j < kGroupSums ? r + other : fmax(r, other);
    }
    if (lane == 0) red[wave * (kGroupSums + kGroupMaxs) + j] = r;
  }
  __syncthreads();
  if (tid < kGroupSums + kGroupMaxs) {
    constexpr int N = kGroupSums + kGroupMaxs;
    const double a = red[tid], b = red[N + tid], cc = red[2 * N + tid], d = red[3 * N + tid];
    partials[(size_t)tid * gridDim.x + blockIdx.x] = tid < kGroupSums ? (a + b) + (cc + d) : fmax(fmax(a, b), fmax(cc, d));
  }
}

bool mma_dual_groups_tile(const GroupMap &m, int64_t n) {
  const int64_t period = (int64_t)m.nw + m.skip;
  if (m.nwcon <= 0) return true;
  return m.nw > 0 && period <= kGroupTile && m.start >= 0 && m.start + (m.nwcon - 1) * period + m.nw <= n;
}

int k_mma_group_solve(Ctx *c, const MmaDualData &s, const MmaDualGroups &g, const double *lambda, double *x,
                      double *zw, double *zl, double *zu, MmaGroupStats *st, const MmaDualRho *r) {
  DualTables t;
  PO_TRY(dual_tables(s, lambda, &t));
  const double sigma = r ? rho_sigma(*r, s.m, lambda) : 0.0;  // (the groups take no table of rho)
  GroupMap gm = g.map;
  if (gm.nwcon <= 0) {  // no group: every variable takes the closed form
    gm = GroupMap();
    gm.nw = 1;
  }
  if (!mma_dual_groups_tile(gm, s.n) || (zl == nullptr) != (zu == nullptr)) {
    set_error("MMA dual: the group map (nwcon %lld, nw %d, skip %d, start %lld) does not tile %lld variables",
              (long long)gm.nwcon, gm.nw, gm.skip, (long long)gm.start, (long long)s.n);
    return PO_ERR_ARG;
  }
  const int period = gm.nw + gm.skip;
  int G = kGroupTile / period;
  if (G > kBlock) G = kBlock;
  const int64_t ntiles = (gm.nwcon + G - 1) / G;
  count_bytes(c, 2 * s.m + 6 + 1 + (r ? 1 : 0) + (zl ? 2 : 0), s.n);
  count_bytes(c, 2.0, gm.nwcon);
  int64_t want = ntiles > (s.n + kBlock - 1) / kBlock / 8 ? ntiles : (s.n + kBlock - 1) / kBlock / 8;
  if (want > (int64_t)c->num_cu * 4) want = (int64_t)c->num_cu * 4;
  const int grid = want < 1 ? 1 : (int)want;
  PO_TRY(ensure_partials(c, (size_t)grid * (kGroupSums + kGroupMaxs)));
  if (r) {
    PO_MLAUNCH(mma_group_solve_kernel<true>, grid, gm, g.a, g.c, g.nwinequality, g.gamma, s.L, s.U, s.alpha, s.beta,
               s.p0, s.q0, t.pt, t.qt, t.ct, s.m, s.n, G, ntiles, x, zw, zl, zu, c->d_partials, r->xk, sigma);
  } else {
    PO_MLAUNCH(mma_group_solve_kernel<false>, grid, gm, g.a, g.c, g.nwinequality, g.gamma, s.L, s.U, s.alpha, s.beta,
               s.p0, s.q0, t.pt, t.qt, t.ct, s.m, s.n, G, ntiles, x, zw, zl, zu, c->d_partials, nullptr, 0.0);
  }
  double out[kGroupSums + kGroupMaxs];
  PO_TRY(reduce_finish(c, grid, kGroupSums, 0, kGroupMaxs, out, true));
  if (st) {
    st->zw_psi = out[0];
    st->strict = (long)out[1];
    st->at_lower = (long)out[2];
    st->at_gamma = (long)out[3];
    st->cap_hits = (long)out[4];
    st->steps = (long)out[5];
    st->max_inner = (int)out[6];
    st->max_psi = out[7];
  }
  return PO_OK;
}

int k_mma_gcmma_group_sums(Ctx *c, const MmaDualData &s, const double *xk, const double *x, double *sums) {
  const int m = s.m;
  PO_TRY(check_m(m));
  const PtrTable pt = ptr_table<PtrTable>(s.p, m), qt = ptr_table<PtrTable>(s.q, m);  // (the pass takes no multipliers)
  count_bytes(c, 2 * m + 6, s.n);
  double all[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(
      c, m, s.n, 0, [](auto MC) { return DualSlots<decltype(MC)::value, 5, true>::NS; },
      [&](auto MC, int grid) -> int {
        PO_MLAUNCH((mma_gcmma_group_sums_kernel<decltype(MC)::value>), grid, s.L, s.U, s.p0, s.q0, xk, x, pt, qt, m, s.n,
                   c->d_partials);
        return PO_OK;
      },
      all, &sh));
  copy_point_sums(all, sh.ns, m, sums);
  return PO_OK;
}

// sw_i <- [zlo_i < zw_i < gamma and sw_i > 0] / sw_i: the weights of the Gram over the group panel
__global__ void __launch_bounds__(kBlock)
    mma_group_weights_kernel(const double *__restrict__ zw, int64_t nwcon, int64_t nwineq, double gamma,
                             double *__restrict__ sw) {
  PO_M_LOOP(i, nwcon) {
    const double z = zw[i], sv = sw[i];
    const double zlo = i >= nwineq ? -gamma : 0.0;
    sw[i] = (z > zlo && z < gamma && sv > 0.0) ? 1.0 / sv : 0.0;
  }
  // (the pad element of an odd length: its panel entries are zeros)
  if ((nwcon & 1) && blockIdx.x == 0 && threadIdx.x == 0) sw[nwcon] = 0.0;
}

int k_mma_dual_groups(Ctx *c, const MmaDualData &s, const MmaDualGroups &g, const double *lambda, double *W,
                      double *grad, double *H, double *const *G, double *dvec, double *x, double *zw,
                      double *const *Uw, double *sw, double *zl, double *zu, MmaGroupStats *st, const MmaDualRho *r,
                      double *D) {
  const int m = s.m;
  MmaGroupStats local;
  if (!st) st = &local;
  PO_TRY(k_mma_group_solve(c, s, g, lambda, x, zw, zl, zu, st, r));
  DualTables t;
  PO_TRY(dual_tables(s, lambda, &t));
  if (!dvec || (m > 0 && !G)) {
    set_error("MMA dual: the grouped evaluation needs its %d column vectors and the weight vector", m);
    return PO_ERR_ARG;
  }
  const PtrTableW gt = ptr_table<PtrTableW>(G, m);
  const CoefTable rt = r ? coef_table(r->rho + 1, m) : CoefTable();
  const double sigma = r ? rho_sigma(*r, m, lambda) : 0.0;
  count_bytes(c, 2 * m + 7 + (r ? 1 : 0) + m + 1, s.n);
  double sums[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(
      c, m, s.n, 0,
      [&](auto MC) {
        constexpr int kMC = decltype(MC)::value;
        return r ? DualSlots<kMC, 4, true>::NS : DualSlots<kMC, 4, false>::NS;
      },
      [&](auto MC, int grid) -> int {
        constexpr int kMC = decltype(MC)::value;
        if (r) {
          PO_MLAUNCH((mma_dual_stored_rho_kernel<kMC>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, r->xk, x, t.pt,
                     t.qt, t.ct, rt, sigma, m, s.n, gt, dvec, c->d_partials);
        } else {
          PO_MLAUNCH((mma_dual_stored_kernel<kMC>), grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, x, t.pt, t.qt, t.ct, m,
                     s.n, gt, dvec, c->d_partials);
        }
        return PO_OK;
      },
      sums, &sh));
  if (r) apply_rho(sums, sh.ns, sigma, r->rho, m, D);
  dual_value_grad(sums[0] - st->zw_psi, sums, lambda, s.b, m, W, grad);
  if (!H || m <= 0) return PO_OK;
  PO_TRY(k_wgram(c, dvec, G, m, s.n, H));
  if (g.map.nwcon <= 0 && c->size == 1) return PO_OK;
  if (!Uw || !sw) {
    set_error("MMA dual: the grouped Hessian needs its %d group columns and the group weights", m);
    return PO_ERR_ARG;
  }
  std::vector<double> H2((size_t)m * m, 0.0);
  PO_TRY(k_group_panel(c, g.map, G, m, dvec, 1.0, Uw));
  PO_TRY(k_group_sum(c, g.map, sw, 0, 0.0, 1.0, dvec));
  if (g.map.nwcon > 0) {
    count_bytes(c, 3.0, g.map.nwcon);
    PO_MLAUNCH(mma_group_weights_kernel, grid_for(c, g.map.nwcon), zw, g.map.nwcon, g.nwinequality, g.gamma, sw);
  }
  PO_TRY(k_wgram(c, sw, Uw, m, g.map.nwcon, H2.data()));
  for (size_t i = 0; i < H2.size(); i++) H[i] -= H2[i];
  return PO_OK;
}

// ---- the dual of the subproblem with linearised constraints (mma.hpp; the subproblem of :804-924 with
// mma_use_constraint_linearization) ------------------------------------------------------------------------------------
// With t = sum_i lambda_i A_i the minimiser of the Lagrangian is, element by element, the root of the increasing
// function p0 u^2 - q0 l^2 = t clamped into [alpha, beta]: the bracketed Newton iteration of the grouped constraints
// (group_el_root_steps with both of its extra stops), started from the stored x.  P = p0 and Q = q0 never depend on lambda, so a multiplier of
// either sign is harmless.
struct LinearPoint {
  f64x2 x, u, l, fr;  // fr: 1.0 where the root lies strictly inside (alpha, beta), else 0.0
};
__device__ __forceinline__ void linear_point1(double p0, double q0, double L, double U, double a, double b, double t,
                                              double xs, bool live, double &x, double &u, double &l, double &fr,
                                              int &capped, int &most) {
  x = u = l = fr = 0.0;
  if (!live) return;
  GroupEl e;
  e.P = p0;
  e.Q = q0;
  e.L = L;
  e.U = U;
  e.a = a;
  e.b = b;
  e.ga = group_phi1(p0, q0, L, U, a);
  e.gb = group_phi1(p0, q0, L, U, b);
  int steps;
  // (both extra stops: where |x| is far below |L|, |U| the search would otherwise creep into the cap, see above)
  x = group_el_root_steps<true, true>(e, t, xs, capped, steps);
  most = steps > most ? steps : most;
  u = 1.0 / (U - x);
  l = 1.0 / (x - L);
  fr = (x > a && x < b) ? 1.0 : 0.0;
}
__device__ __forceinline__ LinearPoint linear_point(f64x2 p0, f64x2 q0, f64x2 L, f64x2 U, f64x2 a, f64x2 b, f64x2 t,
                                                    f64x2 xs, bool has2, int &capped, int &most) {
  double x0, u0, l0, f0, x1, u1, l1, f1;
  linear_point1(p0.x, q0.x, L.x, U.x, a.x, b.x, t.x, xs.x, true, x0, u0, l0, f0, capped, most);
  linear_point1(p0.y, q0.y, L.y, U.y, a.y, b.y, t.y, xs.y, has2, x1, u1, l1, f1, capped, most);
  LinearPoint r;
  r.x = (f64x2){x0, x1};
  r.u = (f64x2){u0, u1};
  r.l = (f64x2){l0, l1};
  r.fr = (f64x2){f0, f1};
  return r;
}
// t += sum_{j <= i < j + B} lambda_i A_i: B loads in flight, issued back to back before their arithmetic (the one-table
// form of dual_pq_batch: same fma order)
template <int B>
__device__ __forceinline__ void linear_t_batch(const PtrTable &At, const CoefTable &lam, int j, int64_t q, f64x2 &t) {
  f64x2 av[B];
#pragma unroll
  for (int u = 0; u < B; u++) av[u] = ld_nt(At.p[j + u] + 2 * q);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < B; u++) t = fma2(lam.a[j + u], av[u], t);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void linear_t_all(const PtrTable &At, const CoefTable &lam, int m, int64_t q, f64x2 &t) {
  int j = 0;
  for (; j + 8 <= m; j += 8) linear_t_batch<8>(At, lam, j, q, t);
  if (j + 4 <= m) {
    linear_t_batch<4>(At, lam, j, q, t);
    j += 4;
  }
  if (j + 2 <= m) {
    linear_t_batch<2>(At, lam, j, q, t);
    j += 2;
  }
  if (j < m) linear_t_batch<1>(At, lam, j, q, t);
}
// Sums: {sum p0 u + q0 l, s_i[MC] = sum A_i (x - xk), in MODE 1 the MC (MC + 1) / 2 sums of [free] A_i A_k / h (k-major
// lower triangle), cap hits of the root searches}; one maximum behind them: the most evaluations one root search took.
template <int MC, int MODE>
struct LinearSlots {
  static constexpr int NH = MODE == 1 ? MC * (MC + 1) / 2 : 0;
  static constexpr int NS = 1 + MC + NH + 1;
};
// MC, MODE 0 / 1 / 2 as in mma_dual_kernel; the columns are the A_i themselves (MODE 2 stores only the weights
// [free] / h).  xs: the start of the root searches, xo: the point of this evaluation (may be the same vector: a lane
// reads its pair before it writes it).  Streams: 8 + m in, 1 out (2 in MODE 2).
template <int MC, int MODE>
__global__ void __launch_bounds__(kBlock)
    mma_dual_linear_kernel(const double *__restrict__ L, const double *__restrict__ U, const double *__restrict__ alpha,
                           const double *__restrict__ beta, const double *__restrict__ p0,
                           const double *__restrict__ q0, const double *__restrict__ xk, const double *xs, PtrTable At,
                           CoefTable lam, int m, int64_t n, double *xo, double *__restrict__ dout,
                           double *__restrict__ partials) {
  constexpr bool HOLD = MC <= PO_MMA_DUAL_HOLD;
  constexpr int NVB = 8;
  constexpr int NS = LinearSlots<MC, MODE>::NS;
  static_assert(MODE != 1 || MC <= kMmaDualFused, "the fused Hessian needs the columns in registers");
  __shared__ double sm[4 * NS];
  __shared__ double smax[4];
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) acc[s] = 0.0;
  int capped = 0, most = 0;
  const int64_t npairs = (n + 1) >> 1;
  // first pair and stride of a lane: taken here, where the workgroup size is a launch constant
  const int64_t qfirst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, qstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = qfirst; q < npairs; q += qstride) {
    const bool has2 = 2 * q + 1 < n;
    const f64x2 Lv = ld_nt(L + 2 * q), Uv = ld_nt(U + 2 * q), av = ld_nt(alpha + 2 * q), bv = ld_nt(beta + 2 * q);
    const f64x2 P = ld_nt(p0 + 2 * q), Q = ld_nt(q0 + 2 * q), xkv = ld_nt(xk + 2 * q), xsv = ld_nt(xs + 2 * q);
    f64x2 t = (f64x2){0.0, 0.0};
    f64x2 cv[HOLD ? MC : 1];
    if (HOLD) {
#pragma unroll
      for (int i = 0; i < MC; i++) {
        cv[i] = (f64x2){0.0, 0.0};
        if (i < m) cv[i] = ld_nt(At.p[i] + 2 * q);
      }
#pragma unroll
      for (int i = 0; i < MC; i++)
        if (i < m) t = fma2(lam.a[i], cv[i], t);
    } else {
      linear_t_all(At, lam, m, q, t);
    }
    const LinearPoint pt = linear_point(P, Q, Lv, Uv, av, bv, t, xsv, has2, capped, most);
    st_nt(xo + 2 * q, pt.x);
    acc[0] = dot4(P, pt.u, Q, pt.l, acc[0]);
    f64x2 dx = pt.x - xkv;
    if (!has2) dx.y = 0.0;
    f64x2 dw = (f64x2){0.0, 0.0};
    if (MODE != 0) {
      const f64x2 h = 2.0 * (P * (pt.u * pt.u * pt.u) + Q * (pt.l * pt.l * pt.l));
      dw.x = pt.fr.x != 0.0 ? 1.0 / h.x : 0.0;
      dw.y = pt.fr.y != 0.0 ? 1.0 / h.y : 0.0;
      if (MODE == 2) st_nt(dout + 2 * q, dw);
    }
    if (HOLD) {
#pragma unroll
      for (int i = 0; i < MC; i++) acc[1 + i] = fma(cv[i].x, dx.x, fma(cv[i].y, dx.y, acc[1 + i]));
      if (MODE == 1) {
#pragma unroll
        for (int k = 0; k < MC; k++) {
          const f64x2 gk = cv[k] * dw;
#pragma unroll
          for (int i = 0; i <= k; i++) {
            const int s = 1 + MC + k * (k + 1) / 2 + i;
            acc[s] = fma(cv[i].x, gk.x, fma(cv[i].y, gk.y, acc[s]));
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < MC; j += NVB) {
        if (j < m) {
          f64x2 cb[NVB];
#pragma unroll
          for (int v = 0; v < NVB; v++) {
            cb[v] = (f64x2){0.0, 0.0};
            if (j + v < m) cb[v] = ld_nt(At.p[j + v] + 2 * q);
          }
#pragma unroll
          for (int v = 0; v < NVB; v++) acc[1 + j + v] = fma(cb[v].x, dx.x, fma(cb[v].y, dx.y, acc[1 + j + v]));
        }
      }
    }
  }
  acc[NS - 1] = (double)capped;
  dual_block_reduce<NS>(acc, partials, sm);
  double mx = (double)most;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(size_t)NS * gridDim.x + blockIdx.x] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
}

// one pass at the final lambda: x (root searches started from xs), zl = max(r, 0) where x = alpha, zu = max(-r, 0)
// where x = beta, r = p0 u^2 - q0 l^2 - t (0 elsewhere); slots {cap hits} and the maximum {most evaluations}
__global__ void __launch_bounds__(kBlock)
    mma_dual_linear_point_kernel(const double *__restrict__ L, const double *__restrict__ U,
                                 const double *__restrict__ alpha, const double *__restrict__ beta,
                                 const double *__restrict__ p0, const double *__restrict__ q0, const double *xs,
                                 PtrTable At, CoefTable lam, int m, int64_t n, double *x, double *__restrict__ zl,
                                 double *__restrict__ zu, double *__restrict__ partials) {
  __shared__ double sm[4];
  __shared__ double smax[4];
  int capped = 0, most = 0;
  const int64_t npairs = (n + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
    const bool has2 = 2 * q + 1 < n;
    const f64x2 Lv = ld_nt(L + 2 * q), Uv = ld_nt(U + 2 * q), av = ld_nt(alpha + 2 * q), bv = ld_nt(beta + 2 * q);
    const f64x2 P = ld_nt(p0 + 2 * q), Q = ld_nt(q0 + 2 * q), xsv = ld_nt(xs + 2 * q);
    f64x2 t = (f64x2){0.0, 0.0};
    linear_t_all(At, lam, m, q, t);
    const LinearPoint pt = linear_point(P, Q, Lv, Uv, av, bv, t, xsv, has2, capped, most);
    const f64x2 ql = Q * (pt.l * pt.l), u2 = pt.u * pt.u;
    const f64x2 r = (f64x2){fma(P.x, u2.x, -ql.x) - t.x, fma(P.y, u2.y, -ql.y) - t.y};
    f64x2 lo, up;
    lo.x = pt.x.x == av.x ? fmax(r.x, 0.0) : 0.0;
    up.x = pt.x.x == bv.x ? fmax(-r.x, 0.0) : 0.0;
    lo.y = (has2 && pt.x.y == av.y) ? fmax(r.y, 0.0) : 0.0;
    up.y = (has2 && pt.x.y == bv.y) ? fmax(-r.y, 0.0) : 0.0;
    st_nt(x + 2 * q, pt.x);
    st_nt(zl + 2 * q, lo);
    st_nt(zu + 2 * q, up);
  }
  double acc[1] = {(double)capped};
  dual_block_reduce<1>(acc, partials, sm);
  double mx = (double)most;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(size_t)gridDim.x + blockIdx.x] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
}

static void linear_stats(const double *capmax, MmaLinearStats *st) {
  if (!st) return;
  st->cap_hits += (long)capmax[0];
  st->max_steps = st->max_steps > (int)capmax[1] ? st->max_steps : (int)capmax[1];
}

int k_mma_dual_linear(Ctx *c, const MmaDualLinear &s, const double *lambda, int form, const double *xstart, double *x,
                      double *W, double *grad, double *H, double *dvec, MmaLinearStats *st) {
  const int m = s.m;
  PO_TRY(check_m(s.m));
  const PtrTable at = ptr_table<PtrTable>(s.A, s.m);
  const CoefTable ct = coef_table(lambda, s.m);
  PO_TRY(check_form(&form, m, H));
  if (form == 2 && !dvec) {
    set_error("MMA dual: the panel form needs the weight vector");
    return PO_ERR_ARG;
  }
  count_bytes(c, m + 9 + (form == 2 ? 1 : 0), s.n);
  // (one grid for every form: the value and the gradient have the same bits whichever form computed them)
  const auto slots = [&](auto MC) {
    return with_form(form, MC, [](auto MC_, auto MODE) -> int {
      return LinearSlots<decltype(MC_)::value, decltype(MODE)::value>::NS;
    });
  };
  const auto launch = [&](auto MC, int grid) {
    return with_form(form, MC, [&](auto MC_, auto MODE) -> int {
      PO_MLAUNCH((mma_dual_linear_kernel<decltype(MC_)::value, decltype(MODE)::value>), grid, s.L, s.U, s.alpha, s.beta,
                 s.p0, s.q0, s.xk, xstart, at, ct, m, s.n, x, dvec, c->d_partials);
      return PO_OK;
    });
  };
  double sums[kPassSlots];
  PassShape sh;
  PO_TRY(reducing_pass(c, m, s.n, 1, slots, launch, sums, &sh));  // (the most steps ride as a maximum)
  linear_stats(sums + sh.ns - 1, st);
  double w = sums[0];
  for (int i = 0; i < m; i++) {
    const double ci = s.cons[i] + sums[1 + i];
    w -= lambda[i] * ci;
    grad[i] = -ci;
  }
  *W = w;
  return form_hessian(c, form, sums, sh.mc, dvec, s.A, m, s.n, H);
}

int k_mma_dual_linear_point(Ctx *c, const MmaDualLinear &s, const double *lambda, const double *xstart, double *x,
                            double *zl, double *zu, MmaLinearStats *st) {
  PO_TRY(check_m(s.m));
  const PtrTable at = ptr_table<PtrTable>(s.A, s.m);
  const CoefTable ct = coef_table(lambda, s.m);
  count_bytes(c, s.m + 7 + 3, s.n);
  const int grid = grid_for(c, s.n, kBpcPanel);
  PO_TRY(ensure_partials(c, (size_t)grid * 2));
  PO_MLAUNCH(mma_dual_linear_point_kernel, grid, s.L, s.U, s.alpha, s.beta, s.p0, s.q0, xstart, at, ct, s.m, s.n, x, zl,
             zu, c->d_partials);
  double capmax[2];
  PO_TRY(reduce_finish(c, grid, 1, 0, 1, capmax, true));
  linear_stats(capmax, st);
  return PO_OK;
}

}  // namespace po
