// Stand-alone host driver of the MMA dual solver (paropt_amd/csrc/mma_dual.cpp): no device, no HIP.  Reads one
// subproblem from a binary file, evaluates W, grad W and -hess W in plain loops, runs mma_dual_solve and prints the
// result.  Built with -fsanitize=address,undefined by tests/test_mma_dual_host.py.
//
// file: int64 n, m, max_evaluations; double tol; gamma[m], lambda0[m], b[m]; L, U, alpha, beta, p0, q0 [n each];
//       p[m][n]; q[m][n]
// out:  "status evaluations iterations pg" and one line per multiplier (%.17g)
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../paropt_amd/csrc/mma_dual.hpp"

static bool read_doubles(FILE *f, std::vector<double> &v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(double), count, f) == count;
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
  std::vector<double> gamma, lam, b, L, U, al, be, p0, q0, p, q;
  bool ok = read_doubles(f, gamma, m) && read_doubles(f, lam, m) && read_doubles(f, b, m) && read_doubles(f, L, n) &&
            read_doubles(f, U, n) && read_doubles(f, al, n) && read_doubles(f, be, n) && read_doubles(f, p0, n) &&
            read_doubles(f, q0, n) && read_doubles(f, p, (size_t)m * n) && read_doubles(f, q, (size_t)m * n);
  fclose(f);
  if (!ok) return 2;
  std::vector<double> gcol(m);
  auto eval = [&](const double *lm, bool want_h, double *W, double *g, double *H) {
    double w = 0.0;
    for (int i = 0; i < m; i++) {
      w += lm[i] * b[i];
      g[i] = b[i];
    }
    if (want_h)
      for (size_t k = 0; k < (size_t)m * m; k++) H[k] = 0.0;
    for (size_t j = 0; j < n; j++) {
      double P = p0[j], Q = q0[j];
      for (int i = 0; i < m; i++) {
        P += lm[i] * p[i * n + j];
        Q += lm[i] * q[i * n + j];
      }
      const double sp = sqrt(P), sq = sqrt(Q);
      const double xs = (sp * L[j] + sq * U[j]) / (sp + sq);
      const bool is_free = xs > al[j] && xs < be[j];
      const double x = fmin(fmax(xs, al[j]), be[j]);
      const double u = 1.0 / (U[j] - x), l = 1.0 / (x - L[j]);
      w += P * u + Q * l;
      for (int i = 0; i < m; i++) g[i] += p[i * n + j] * u + q[i * n + j] * l;
      if (want_h && is_free) {
        const double h = 2.0 * (P * u * u * u + Q * l * l * l);
        for (int i = 0; i < m; i++) gcol[i] = p[i * n + j] * u * u - q[i * n + j] * l * l;
        for (int k = 0; k < m; k++)
          for (int i = 0; i < m; i++) H[i + (size_t)m * k] += gcol[i] * gcol[k] / h;
      }
    }
    *W = w;
    return 0;
  };
  po::MmaDualResult res;
  const int rc = po::mma_dual_solve(m, gamma.data(), tol, max_evals, eval, lam.data(), &res);
  if (rc != 0) return 3;
  printf("%d %d %d %.17g\n", res.status, res.evaluations, res.iterations, res.pg);
  for (int i = 0; i < m; i++) printf("%.17g\n", lam[i]);
  return 0;
}
