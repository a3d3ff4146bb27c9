// Globally convergent MMA (Svanberg 2002 / 2007; mma_globalization = conservative): host side, replicated on every
// rank, no device code and no HIP include -- every input comes out of reductions, so every rank takes the same
// decisions (tests/test_mma_gcmma_host.py runs it without a device).
//
// Every approximation carries the same separable term, f~_i^rho(x) = f~_i(x) + rho_i d(x), i = 0..m (0: the objective,
// i >= 1: g_i = -c_i), d >= 0 with d(xk) = 0 and grad d(xk) = 0.  A subproblem solution x^ is accepted when every
// approximation is conservative there,
//     f_i(x^) <= f_i(xk) + Delta_i + rho_i D + tol max(1, |f_i(x^)|),   Delta_i = f~_i(x^) - f~_i(xk),  D = d(x^),
// and otherwise the rho_i of the violated functions are raised and the subproblem is solved again: an inner iteration
// costs no gradient evaluation and rewrites no coefficient vector.
#pragma once
#include <stdint.h>

#include <functional>

namespace po {

struct GcmmaParams {
  double rho_init = 0.1, rho_min = 1e-6, tol = 1e-7;
  int max_inner = 15;
};

// rho_i = max(rho_init / nglobal * sums[i], rho_min), sums[i] = sum_j |df_i / dx_j| (U_j - L_j), i = 0..m
void gcmma_rho_start(int m, const double *sums, int64_t nglobal, const GcmmaParams &p, double *rho);

// viol[i] = f_i(x^) - (f_i(xk) + Delta_i + rho_i D), i = 0..m; fnew, fk: {f_0, g_1..g_m}; sums: {Delta_0..m, D}.
// True when no viol[i] exceeds tol max(1, |f_i(x^)|), or D == 0 (x^ = xk).  A NaN is a violation.
bool gcmma_accept(int m, const double *fnew, const double *fk, const double *sums, const double *rho, double tol,
                  double *viol);

// rho_i <- min(1.1 (rho_i + viol_i / D), 10 rho_i) where viol_i > 0
void gcmma_raise(int m, const double *viol, double D, double *rho);

// One trial of the inner iteration at the current rho: solve the subproblem (warm-started), and return the sums
// {Delta_0..m, D} of its solution and the true values fnew = {f_0, g_1..g_m} there.  Non-zero: error code.
typedef std::function<int(const double *rho, double *sums, double *fnew)> GcmmaTrialFn;

// The inner iteration: trials until one is accepted or max_inner raises are spent (the last point is then taken:
// *capped).  rho: the start values on entry, those of the accepted trial on return.  Returns the first non-zero code
// of trial, else 0.
int gcmma_inner(int m, const double *fk, const GcmmaParams &p, const GcmmaTrialFn &trial, double *rho, int *raises,
                bool *capped);

}  // namespace po
