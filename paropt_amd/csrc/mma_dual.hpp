// The m-dimensional dual of the separable MMA subproblem (Svanberg 1987, section 5): host side, replicated on every
// rank, no device code and no HIP include -- the solver sees the n-sized data only through an evaluation callback,
// so it compiles and runs without a device (tests/test_mma_dual_host.py).
//
//   maximise W(lambda) over 0 <= lambda <= gamma,   W concave and C1 but only piecewise C2
//
// with g = grad W and H = -hess W (positive semi-definite, exactly zero while every variable sits on a move limit).
#pragma once
#include <functional>

namespace po {

// eval(lambda, want_hessian, &W, g[m], H[m * m]) -> 0 on success; H is the NEGATED Hessian, symmetric, column-major,
// written only when want_hessian is set
typedef std::function<int(const double *lambda, bool want_hessian, double *W, double *g, double *H)> MmaDualEvalFn;

struct MmaDualResult {
  int status = 0;       // 0: max|pg| <= tol; 1: gave up (evaluation cap, or the regularisation passed 1e30)
  int iterations = 0;   // accepted steps
  int evaluations = 0;  // calls of eval
  double pg = 0.0;      // max|projected gradient| at the returned point
};

// Levenberg-regularised projected Newton ascent: d_F = (H_FF + tau I)^-1 g_F on the free set, candidate clipped into
// the box, accepted on sufficient increase of W (or, within the rounding error of W, on a decrease of max|pg|),
// tau / 8 on acceptance, 8 tau on rejection.  lambda: start point on entry (clipped into [0, gamma] first), the
// solution on return.  Returns the first non-zero code of eval, else 0.
int mma_dual_solve(int m, const double *gamma, double tol, int max_evaluations, const MmaDualEvalFn &eval,
                   double *lambda, MmaDualResult *res);
// The same iteration over the box lower <= lambda <= upper (per component; the clip, the projected gradient and the
// free set take both ends): the dual with linearised constraints, whose equality multipliers lie in [-gamma, gamma].
// The form above is this one with lower = 0.
int mma_dual_solve(int m, const double *lower, const double *upper, double tol, int max_evaluations,
                   const MmaDualEvalFn &eval, double *lambda, MmaDualResult *res);

}  // namespace po
