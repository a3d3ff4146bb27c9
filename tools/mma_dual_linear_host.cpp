// Stand-alone host driver of the MMA dual solver's box form (paropt_amd/csrc/mma_dual.cpp) on the dual of the
// subproblem with linearised constraints: no device, no HIP.  Reads one subproblem from a binary file, evaluates W,
// grad W and -hess W in plain loops (the element roots by the bracketed Newton iteration of mma.hip, started from the
// point of the evaluation before), runs mma_dual_solve and prints the result.  Built with -fsanitize=address,undefined
// by tests/test_mma_dual_linear_host.py.
//
// file: int64 n, m, max_evaluations; double tol; lower[m], upper[m], lambda0[m], cons[m];
//       L, U, alpha, beta, p0, q0, xk [n each]; A[m][n]
// out:  "status evaluations iterations pg cap_hits" and one line per multiplier (%.17g)
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../paropt_amd/csrc/mma_dual.hpp"

static bool read_doubles(FILE *f, std::vector<double> &v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(double), count, f) == count;
}

static const int kNewtonCap = 100;

// clamp(root of p0 u^2 - q0 l^2 = t, a, b) from x0; *capped is raised at the step cap
static double element_root(double p0, double q0, double L, double U, double a, double b, double t, double x0,
                           long *capped) {
  auto phi1 = [&](double x) {
    const double u = 1.0 / (U - x), l = 1.0 / (x - L);
    return p0 * u * u - q0 * l * l;
  };
  if (!(t > phi1(a))) return a;
  if (!(t < phi1(b))) return b;
  double lo = a, hi = b, x = x0;
  if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
  int it = 0;
  for (; it < kNewtonCap; it++) {
    const double u = 1.0 / (U - x), l = 1.0 / (x - L);
    const double f = p0 * u * u - q0 * l * l - t;
    const double h = 2.0 * (p0 * u * u * u + q0 * l * l * l);
    if (f < 0.0) lo = x;
    else if (f > 0.0) hi = x;
    else break;
    double xn = x - f / h;
    if (xn == x) break;
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    if (!(xn > lo && xn < hi) || xn == x) break;
    if (U - xn == U - x && xn - L == x - L) break;  // the step changes neither difference
    x = xn;
  }
  if (it == kNewtonCap) (*capped)++;
  return x;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s subproblem.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t head[3];
  double tol = 0.0;
  if (fread(head, sizeof(int64_t), 3, f) != 3 || fread(&tol, sizeof(double), 1, f) != 1) return 2;
  const size_t n = (size_t)head[0];
  const int m = (int)head[1], max_evals = (int)head[2];
  std::vector<double> lower, upper, lam, cons, L, U, al, be, p0, q0, xk, A;
  bool ok = read_doubles(f, lower, m) && read_doubles(f, upper, m) && read_doubles(f, lam, m) &&
            read_doubles(f, cons, m) && read_doubles(f, L, n) && read_doubles(f, U, n) && read_doubles(f, al, n) &&
            read_doubles(f, be, n) && read_doubles(f, p0, n) && read_doubles(f, q0, n) && read_doubles(f, xk, n) &&
            read_doubles(f, A, (size_t)m * n);
  fclose(f);
  if (!ok) return 2;
  std::vector<double> x(xk), c(m);
  long capped = 0;
  auto eval = [&](const double *lm, bool want_h, double *W, double *g, double *H) {
    double w = 0.0;
    for (int i = 0; i < m; i++) c[i] = 0.0;
    if (want_h)
      for (size_t k = 0; k < (size_t)m * m; k++) H[k] = 0.0;
    for (size_t j = 0; j < n; j++) {
      double t = 0.0;
      for (int i = 0; i < m; i++) t += lm[i] * A[i * n + j];
      const double xj = element_root(p0[j], q0[j], L[j], U[j], al[j], be[j], t, x[j], &capped);
      x[j] = xj;
      const double u = 1.0 / (U[j] - xj), l = 1.0 / (xj - L[j]);
      w += p0[j] * u + q0[j] * l;
      for (int i = 0; i < m; i++) c[i] += A[i * n + j] * (xj - xk[j]);
      if (want_h && xj > al[j] && xj < be[j]) {
        const double h = 2.0 * (p0[j] * u * u * u + q0[j] * l * l * l);
        for (int k = 0; k < m; k++)
          for (int i = 0; i < m; i++) H[i + (size_t)m * k] += A[i * n + j] * A[k * n + j] / h;
      }
    }
    for (int i = 0; i < m; i++) {
      const double ci = cons[i] + c[i];
      w -= lm[i] * ci;
      g[i] = -ci;
    }
    *W = w;
    return 0;
  };
  po::MmaDualResult res;
  const int rc = po::mma_dual_solve(m, lower.data(), upper.data(), tol, max_evals, eval, lam.data(), &res);
  if (rc != 0) return 3;
  printf("%d %d %d %.17g %ld\n", res.status, res.evaluations, res.iterations, res.pg, capped);
  for (int i = 0; i < m; i++) printf("%.17g\n", lam[i]);
  return 0;
}
