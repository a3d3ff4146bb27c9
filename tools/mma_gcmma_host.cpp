// Stand-alone host driver of the conservative inner iteration (paropt_amd/csrc/mma_gcmma.cpp on top of mma_dual.cpp):
// no device, no HIP.  Reads one subproblem with its expansion point and gradients from a binary file, forms the start
// values of rho, and runs gcmma_inner with every n-sized sum taken in plain loops.  The problem's own functions live
// with the caller: each trial point goes out on stdout and the values there come back on stdin.  Built with
// -fsanitize=address,undefined by tests/test_mma_gcmma_host.py.
//
// file:   int64 n, m, max_evaluations, max_inner, nglobal; double dual_tol, rho_init, rho_min, tol;
//         gamma[m], lambda0[m], b[m], fk[m + 1]; L, U, alpha, beta, p0, q0, xk, g [n each]; p[m][n]; q[m][n]; A[m][n]
// stdout: "rho0 <m + 1 values>"; per trial "x <n values>" (then m + 1 values f_0, g_1..g_m are read from stdin);
//         at the end "done <raises> <capped> <dual evaluations>", "rho <m + 1 values>", "lam <m values>" (%.17g)
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../paropt_amd/csrc/mma_dual.hpp"
#include "../paropt_amd/csrc/mma_gcmma.hpp"

static bool read_doubles(FILE *f, std::vector<double> &v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(double), count, f) == count;
}
static void print_row(const char *tag, const double *v, size_t count) {
  fputs(tag, stdout);
  for (size_t i = 0; i < count; i++) printf(" %.17g", v[i]);
  fputc('\n', stdout);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s subproblem.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t head[5];
  double par[4];
  if (fread(head, sizeof(int64_t), 5, f) != 5 || fread(par, sizeof(double), 4, f) != 4) return 2;
  const size_t n = (size_t)head[0];
  const int m = (int)head[1], max_evals = (int)head[2];
  po::GcmmaParams gp;
  gp.max_inner = (int)head[3];
  gp.rho_init = par[1];
  gp.rho_min = par[2];
  gp.tol = par[3];
  const double dual_tol = par[0];
  std::vector<double> gamma, lam, b, fk, L, U, al, be, p0, q0, xk, g, p, q, A;
  bool ok = read_doubles(f, gamma, m) && read_doubles(f, lam, m) && read_doubles(f, b, m) &&
            read_doubles(f, fk, m + 1) && read_doubles(f, L, n) && read_doubles(f, U, n) && read_doubles(f, al, n) &&
            read_doubles(f, be, n) && read_doubles(f, p0, n) && read_doubles(f, q0, n) && read_doubles(f, xk, n) &&
            read_doubles(f, g, n) && read_doubles(f, p, (size_t)m * n) && read_doubles(f, q, (size_t)m * n) &&
            read_doubles(f, A, (size_t)m * n);
  fclose(f);
  if (!ok) return 2;

  // the start values of rho
  std::vector<double> sums0(m + 1, 0.0), rho(m + 1);
  for (size_t j = 0; j < n; j++) {
    sums0[0] += fabs(g[j]) * (U[j] - L[j]);
    for (int i = 0; i < m; i++) sums0[1 + i] += fabs(A[i * n + j]) * (U[j] - L[j]);
  }
  po::gcmma_rho_start(m, sums0.data(), head[4], gp, rho.data());
  print_row("rho0", rho.data(), m + 1);

  // the primal point at lm for the current rho: P, Q with the sigma term added last
  const double *cur = rho.data();
  auto point = [&](const double *lm, size_t j, double *P, double *Q, double *wU, double *wL, bool *is_free) {
    double Ps = p0[j], Qs = q0[j], sigma = cur[0];
    for (int i = 0; i < m; i++) {
      Ps += lm[i] * p[i * n + j];
      Qs += lm[i] * q[i * n + j];
      sigma += lm[i] * cur[1 + i];
    }
    const double rs = 1.0 / (U[j] - L[j]);
    *wU = (U[j] - xk[j]) * (U[j] - xk[j]) * rs;
    *wL = (xk[j] - L[j]) * (xk[j] - L[j]) * rs;
    *P = Ps + sigma * *wU;
    *Q = Qs + sigma * *wL;
    const double sp = sqrt(*P), sq = sqrt(*Q);
    const double xs = (sp * L[j] + sq * U[j]) / (sp + sq);
    *is_free = xs > al[j] && xs < be[j];
    return fmin(fmax(xs, al[j]), be[j]);
  };
  std::vector<double> gcol(m);
  auto eval = [&](const double *lm, bool want_h, double *W, double *gr, double *H) {
    double w = 0.0, D = 0.0, sigma = cur[0];
    for (int i = 0; i < m; i++) {
      w += lm[i] * b[i];
      gr[i] = b[i];
      sigma += lm[i] * cur[1 + i];
    }
    if (want_h)
      for (size_t k = 0; k < (size_t)m * m; k++) H[k] = 0.0;
    for (size_t j = 0; j < n; j++) {
      double P, Q, wU, wL;
      bool is_free;
      const double x = point(lm, j, &P, &Q, &wU, &wL, &is_free);
      const double u = 1.0 / (U[j] - x), l = 1.0 / (x - L[j]);
      w += (P - sigma * wU) * u + (Q - sigma * wL) * l;
      D += (x - xk[j]) * (x - xk[j]) * u * l;
      for (int i = 0; i < m; i++) gr[i] += p[i * n + j] * u + q[i * n + j] * l;
      if (want_h && is_free) {
        const double h = 2.0 * (P * u * u * u + Q * l * l * l), dx = x - xk[j];
        const double dprime = dx * (u + l) * (2.0 + dx * (u - l)) / (U[j] - L[j]);  // w_U u^2 - w_L l^2
        for (int i = 0; i < m; i++)
          gcol[i] = p[i * n + j] * u * u - q[i * n + j] * l * l + cur[1 + i] * dprime;
        for (int k = 0; k < m; k++)
          for (int i = 0; i < m; i++) H[i + (size_t)m * k] += gcol[i] * gcol[k] / h;
      }
    }
    for (int i = 0; i < m; i++) gr[i] += cur[1 + i] * D;
    *W = w + sigma * D;
    return 0;
  };

  std::vector<double> x(n);
  int dual_evals = 0;
  auto trial = [&](const double *r, double *sums, double *fnew) -> int {
    cur = r;
    po::MmaDualResult res;
    const int rc = po::mma_dual_solve(m, gamma.data(), dual_tol, max_evals, eval, lam.data(), &res);
    if (rc != 0) return rc;
    dual_evals += res.evaluations;
    for (int i = 0; i < m + 2; i++) sums[i] = 0.0;
    for (size_t j = 0; j < n; j++) {
      double P, Q, wU, wL;
      bool is_free;
      x[j] = point(lam.data(), j, &P, &Q, &wU, &wL, &is_free);
      const double u = 1.0 / (U[j] - x[j]), l = 1.0 / (x[j] - L[j]);
      const double dx = x[j] - xk[j];
      const double du = dx * u / (U[j] - xk[j]), dl = -dx * l / (xk[j] - L[j]);
      sums[0] += p0[j] * du + q0[j] * dl;
      for (int i = 0; i < m; i++) sums[1 + i] += p[i * n + j] * du + q[i * n + j] * dl;
      sums[m + 1] += dx * dx * u * l;
    }
    print_row("x", x.data(), n);
    fflush(stdout);
    for (int i = 0; i <= m; i++)
      if (scanf("%lf", &fnew[i]) != 1) return 4;
    return 0;
  };
  int raises = 0;
  bool capped = false;
  const int rc = po::gcmma_inner(m, fk.data(), gp, trial, rho.data(), &raises, &capped);
  if (rc != 0) return 3;
  printf("done %d %d %d\n", raises, capped ? 1 : 0, dual_evals);
  print_row("rho", rho.data(), m + 1);
  print_row("lam", lam.data(), m);
  return 0;
}
