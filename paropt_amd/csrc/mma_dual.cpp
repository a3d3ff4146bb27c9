// Solver of the MMA subproblem's dual (see mma_dual.hpp).  Host only: no HIP include.
#include "mma_dual.hpp"

#include <math.h>

#include <algorithm>
#include <vector>

namespace po {

namespace {

constexpr double kNoise = 1e-13;  // relative evaluation error allowed for W (the reductions' own bound per term)

// pg_i = 0 where the bound blocks the ascent direction, g_i elsewhere; returns max|pg|
double projected_gradient(int m, const double *lam, const double *lower, const double *upper, const double *g,
                          double *pg) {
  double mx = 0.0;
  for (int i = 0; i < m; i++) {
    const bool blocked = (lam[i] <= lower[i] && g[i] < 0.0) || (lam[i] >= upper[i] && g[i] > 0.0);
    pg[i] = blocked ? 0.0 : g[i];
    mx = std::max(mx, fabs(pg[i]));
  }
  return mx;
}

// in-place Cholesky solve of the k x k column-major system A y = b (A symmetric positive definite); false when a
// pivot is not positive
bool chol_solve(int k, double *A, double *b) {
  for (int j = 0; j < k; j++) {
    double d = A[j + (size_t)k * j];
    for (int p = 0; p < j; p++) d -= A[j + (size_t)k * p] * A[j + (size_t)k * p];
    if (!(d > 0.0)) return false;
    d = sqrt(d);
    A[j + (size_t)k * j] = d;
    for (int i = j + 1; i < k; i++) {
      double s = A[i + (size_t)k * j];
      for (int p = 0; p < j; p++) s -= A[i + (size_t)k * p] * A[j + (size_t)k * p];
      A[i + (size_t)k * j] = s / d;
    }
  }
  for (int i = 0; i < k; i++) {
    double s = b[i];
    for (int p = 0; p < i; p++) s -= A[i + (size_t)k * p] * b[p];
    b[i] = s / A[i + (size_t)k * i];
  }
  for (int i = k - 1; i >= 0; i--) {
    double s = b[i];
    for (int p = i + 1; p < k; p++) s -= A[p + (size_t)k * i] * b[p];
    b[i] = s / A[i + (size_t)k * i];
  }
  return true;
}

}  // namespace

int mma_dual_solve(int m, const double *gamma, double tol, int max_evaluations, const MmaDualEvalFn &eval,
                   double *lambda, MmaDualResult *res) {
  const std::vector<double> lower(m, 0.0);
  return mma_dual_solve(m, lower.data(), gamma, tol, max_evaluations, eval, lambda, res);
}

int mma_dual_solve(int m, const double *lower, const double *upper, double tol, int max_evaluations,
                   const MmaDualEvalFn &eval, double *lambda, MmaDualResult *res) {
  MmaDualResult r;
  const size_t mm = (size_t)m * m;
  std::vector<double> g(m), H(mm), gc(m), Hc(mm), cand(m), pg(m), A(mm), d(m);
  std::vector<int> freeset;
  for (int i = 0; i < m; i++) lambda[i] = std::min(std::max(lambda[i], lower[i]), upper[i]);
  double W = 0.0, Wc = 0.0;
  int rc = eval(lambda, true, &W, g.data(), H.data());
  r.evaluations = 1;
  if (rc != 0) {
    *res = r;
    return rc;
  }
  double trace = 0.0;
  for (int i = 0; i < m; i++) trace += H[i + (size_t)m * i];
  double tau = 1e-8 * std::max(1.0, trace);
  r.status = 1;
  for (;;) {
    r.pg = projected_gradient(m, lambda, lower, upper, g.data(), pg.data());
    if (r.pg <= tol) {
      r.status = 0;
      break;
    }
    if (r.evaluations >= max_evaluations || !(tau <= 1e30)) break;
    freeset.clear();
    for (int i = 0; i < m; i++)
      if (pg[i] != 0.0) freeset.push_back(i);
    const int k = (int)freeset.size();
    for (int b = 0; b < k; b++) {
      for (int a = 0; a < k; a++) A[a + (size_t)k * b] = H[freeset[a] + (size_t)m * freeset[b]];
      A[b + (size_t)k * b] += tau;
      d[b] = g[freeset[b]];
    }
    if (!chol_solve(k, A.data(), d.data())) {  // rounding left H_FF + tau I indefinite: regularise more
      tau *= 8.0;
      continue;
    }
    for (int i = 0; i < m; i++) cand[i] = lambda[i];
    for (int b = 0; b < k; b++) {
      const int i = freeset[b];
      cand[i] = std::min(std::max(lambda[i] + d[b], lower[i]), upper[i]);
    }
    rc = eval(cand.data(), true, &Wc, gc.data(), Hc.data());
    r.evaluations++;
    if (rc != 0) break;
    double slope = 0.0;
    for (int i = 0; i < m; i++) slope += g[i] * (cand[i] - lambda[i]);
    // Sufficient increase.  Close to the solution the predicted increase (~ max|pg|^2 / H) falls below the rounding
    // error of W itself, a sum of n terms: the plain test then rejects good steps at random, the regularisation grows
    // and the iteration stalls short of the tolerance (seen with tol 1e-8 and 1e-9 on two of three test problems when
    // only the summation order changes).  So a step whose W lies within kNoise |W| of the test is taken as well when
    // it lowers max|pg| -- that quantity then decreases strictly, so the slack cannot cycle.  (A NaN fails both.)
    bool accept = Wc >= W + 1e-4 * slope;
    if (!accept && Wc >= W + 1e-4 * slope - kNoise * std::max(1.0, fabs(W)))
      accept = projected_gradient(m, cand.data(), lower, upper, gc.data(), pg.data()) < r.pg;
    if (accept) {
      for (int i = 0; i < m; i++) lambda[i] = cand[i];
      W = Wc;
      g.swap(gc);
      H.swap(Hc);
      tau = std::max(tau / 8.0, 1e-14);
      r.iterations++;
    } else {
      tau *= 8.0;
    }
  }
  *res = r;
  return rc;
}

}  // namespace po
