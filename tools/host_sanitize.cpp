// Host-side C++ of the product under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only, no GPU, no HIP
// runtime): the in-repo LU (lu.cpp, the reference's dgetrf/dgetrs sites), the dense algebra of the bordered KKT solve
// and of the linearised KKT residual (bordered.cpp), the one-time symbolic analysis of the sparse Cholesky
// (csr.cpp::csr_analyse) and the option registry (options.cpp).  Built by
// `make -C paropt_amd/csrc sanitize`, run by tests/test_host_sanitize.py.  Exit code 0 = every check passed and no
// sanitizer report.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "core.hpp"
#include "csr.hpp"
#include "ip.hpp"

using namespace po;

static int fails = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      fails++;                                                       \
    }                                                                \
  } while (0)

static uint64_t rng_state = 88172645463325252ULL;
static double rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static void test_lu() {
  for (int n : {1, 2, 3, 7, 20, 42, 64}) {
    std::vector<double> A((size_t)n * n), A0, b(n), x(n);
    for (double &v : A) v = rnd() - 0.5;
    for (int i = 0; i < n; i++) A[(size_t)i * (n + 1)] += (i % 3 == 0) ? 0.0 : 2.0;  // force row exchanges
    A0 = A;
    for (int i = 0; i < n; i++) x[i] = rnd();
    for (int i = 0; i < n; i++) {
      double s = 0.0;
      for (int j = 0; j < n; j++) s += A0[i + (size_t)n * j] * x[j];
      b[i] = s;
    }
    std::vector<int> piv(n);
    const int info = lu_factor(n, A.data(), n, piv.data());
    CHECK(info == 0);
    for (int i = 0; i < n; i++) CHECK(piv[i] >= i && piv[i] < n);
    lu_solve(n, A.data(), n, piv.data(), b.data());
    double err = 0.0;
    for (int i = 0; i < n; i++) err = fmax(err, fabs(b[i] - x[i]));
    CHECK(err < 1e-8);
  }
  // exactly singular: info = index + 1 of the zero pivot, nothing out of bounds, no trap
  std::vector<double> S = {1.0, 2.0, 2.0, 4.0};
  int piv[2];
  CHECK(lu_factor(2, S.data(), 2, piv) == 2);
  CHECK(lu_factor(0, nullptr, 1, nullptr) == 0);
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

// The bordered solve against the system it stands for.  With P^T px = dots + W coef and B = quasi-Newton part, the
// unknowns (pz, w, ps, pt, pzs, pzt) with pz = coef_A, w = coef_Z satisfy
//   (dots + W coef)_A - ps + pt = alpha b.z       (dots + W coef)_Z - M / (d0 d0^T) w = 0
//   pz - pzs = alpha b.s     -pz - pzt = alpha b.t     zs ps + s pzs = alpha b.zs     zt pt + t pzt = alpha b.zt
// assembled here as one dense (5c + k)-square system.
static void test_bordered() {
  const int n = 40;
  for (int c : {0, 1, 5})
    for (int k : {0, 3}) {
      const int m = c + k;
      Bordered kkt;
      kkt.c = c;
      kkt.k = k;
      // W = P^T diag(d) P of a random panel, d > 0
      std::vector<double> Pm((size_t)n * m), d(n);
      for (double &v : Pm) v = rnd() - 0.5;
      for (double &v : d) v = 0.5 + rnd();
      kkt.W.assign((size_t)m * m, 0.0);
      for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++)
          for (int r = 0; r < n; r++)
            kkt.W[i + (size_t)m * j] += Pm[r + (size_t)n * i] * d[r] * Pm[r + (size_t)n * j];
      Dense vars, b;
      vars.resize(c);
      b.resize(c);
      for (std::vector<double> *v : {&vars.z, &vars.s, &vars.t, &vars.zs, &vars.zt})
        for (double &e : *v) e = 0.5 + rnd();
      for (std::vector<double> *v : {&b.z, &b.s, &b.t, &b.zs, &b.zt})
        for (double &e : *v) e = rnd() - 0.5;
      // M = -(I + R R^T / k): Ce = (Schur complement of W) - M / (d0 d0^T) is positive definite
      std::vector<double> d0(k), M((size_t)k * k), R((size_t)k * k);
      for (double &v : d0) v = 1.0 + rnd();
      for (double &v : R) v = rnd() - 0.5;
      for (int j = 0; j < k; j++)
        for (int i = 0; i < k; i++) {
          double v = i == j ? 1.0 : 0.0;
          for (int l = 0; l < k; l++) v += R[i + (size_t)k * l] * R[j + (size_t)k * l] / k;
          M[i + (size_t)k * j] = -v;
        }
      std::vector<double> dots(m > 0 ? m : 1, 0.0);
      for (int i = 0; i < m; i++) dots[i] = rnd() - 0.5;
      std::vector<double> G0, Ce0;
      kkt.factor(vars, d0.data(), M.data(), &G0, &Ce0);
      CHECK(kkt.checkWidth(k) == PO_OK && kkt.checkWidth(k + 1) == PO_ERR_ARG);
      CHECK((int)G0.size() == c * c && (int)Ce0.size() == k * k);
      for (double alpha : {1.0, 0.7}) {
        Bordered::Sol sol;
        kkt.solve(alpha, b, vars, dots.data(), &sol);
        Dense out;
        out.resize(c);
        kkt.backSubstitute(alpha, b, vars, sol, true, out);
        std::vector<double> ptpx;
        kkt.panelDots(dots.data(), sol, false, &ptpx);
        for (int i = 0; i < c; i++) CHECK(out.z[i] == sol.coef[i]);
        // the assembled system, unknowns (pz, w, ps, pt, pzs, pzt)
        const int N = 5 * c + k;
        const int iz = 0, iw = c, is = c + k, it = 2 * c + k, izs = 3 * c + k, izt = 4 * c + k;
        std::vector<double> K((size_t)N * N, 0.0), rhs(N, 0.0), u(N, 0.0);
        auto at = [&](int r, int col) -> double & { return K[r + (size_t)N * col]; };
        for (int i = 0; i < c; i++) {
          for (int j = 0; j < m; j++) at(iz + i, j) = kkt.W[i + (size_t)m * j];
          at(iz + i, is + i) = -1.0;
          at(iz + i, it + i) = 1.0;
          rhs[iz + i] = alpha * b.z[i] - dots[i];
          at(is + i, iz + i) = 1.0;
          at(is + i, izs + i) = -1.0;
          rhs[is + i] = alpha * b.s[i];
          at(it + i, iz + i) = -1.0;
          at(it + i, izt + i) = -1.0;
          rhs[it + i] = alpha * b.t[i];
          at(izs + i, is + i) = vars.zs[i];
          at(izs + i, izs + i) = vars.s[i];
          rhs[izs + i] = alpha * b.zs[i];
          at(izt + i, it + i) = vars.zt[i];
          at(izt + i, izt + i) = vars.t[i];
          rhs[izt + i] = alpha * b.zt[i];
        }
        for (int i = 0; i < k; i++) {
          for (int j = 0; j < m; j++) at(iw + i, j) = kkt.W[(c + i) + (size_t)m * j];
          for (int j = 0; j < k; j++) at(iw + i, iw + j) -= M[i + (size_t)k * j] / (d0[i] * d0[j]);
          rhs[iw + i] = -dots[c + i];
        }
        for (int i = 0; i < c; i++) {
          u[iz + i] = out.z[i];
          u[is + i] = out.s[i];
          u[it + i] = out.t[i];
          u[izs + i] = out.zs[i];
          u[izt + i] = out.zt[i];
        }
        for (int j = 0; j < k; j++) u[iw + j] = sol.coef[c + j];
        double res = 0.0, scale = 0.0, kmax = 0.0, umax = 0.0;
        for (int r = 0; r < N; r++) {
          double v = -rhs[r];
          for (int j = 0; j < N; j++) {
            v += at(r, j) * u[j];
            kmax = fmax(kmax, fabs(at(r, j)));
          }
          res = fmax(res, fabs(v));
          scale = fmax(scale, fabs(rhs[r]));
        }
        for (double v : u) umax = fmax(umax, fabs(v));
        CHECK(res <= 1e-12 * (kmax * umax + scale));
        // P^T px of the step, and its accumulation by a refinement pass
        for (int i = 0; i < m; i++) {
          double v = dots[i];
          for (int j = 0; j < m; j++) v += kkt.W[i + (size_t)m * j] * sol.coef[j];
          CHECK(ptpx[i] == v);
        }
        std::vector<double> acc(ptpx);
        kkt.panelDots(dots.data(), sol, true, &acc);
        for (int i = 0; i < m; i++) CHECK(acc[i] == ptpx[i] + ptpx[i]);
        // without the quasi-Newton correction (GMRES loop): yz alone enters the dense blocks
        Dense part;
        part.resize(c);
        kkt.backSubstitute(alpha, b, vars, sol, false, part);
        for (int i = 0; i < c; i++) CHECK(part.z[i] == sol.yz[i] && part.zs[i] == sol.yz[i] - alpha * b.s[i]);
        if (alpha != 1.0) continue;
        // alpha = 1: the bits of the unscaled expressions of the plain solves
        std::vector<double> yz(c > 0 ? c : 1, 0.0);
        for (int i = 0; i < c; i++)
          yz[i] = (b.z[i] + (b.zs[i] + vars.s[i] * b.s[i]) / vars.zs[i] -
                   (b.zt[i] + vars.t[i] * b.t[i]) / vars.zt[i] - dots[i]);
        if (c > 0) lu_solve(c, kkt.Gf.data(), c, kkt.gpiv.data(), yz.data());
        CHECK(same_bits(yz, sol.yz));
        Dense plain;
        plain.resize(c);
        for (int i = 0; i < c; i++) {
          const double zs1 = yz[i] - b.s[i];
          const double zt1 = -b.t[i] - yz[i];
          plain.z[i] = yz[i] - sol.yz2[i];
          plain.zs[i] = zs1 - sol.yz2[i];
          plain.zt[i] = zt1 + sol.yz2[i];
          plain.s[i] = (b.zs[i] - vars.s[i] * zs1) / vars.zs[i] + (vars.s[i] * sol.yz2[i]) / vars.zs[i];
          plain.t[i] = (b.zt[i] - vars.t[i] * zt1) / vars.zt[i] - (vars.t[i] * sol.yz2[i]) / vars.zt[i];
        }
        CHECK(same_bits(plain.z, out.z) && same_bits(plain.s, out.s) && same_bits(plain.t, out.t) &&
              same_bits(plain.zs, out.zs) && same_bits(plain.zt, out.zt));
      }
    }
}

// The dense rows of the linearised KKT residual (denseResStep): the bits of the expressions the refinement loop and
// checkKKTStep wrote out, on data spread over six decades (a reassociated sum would round differently)
static void test_dense_res_step() {
  auto val = [] { return (rnd() - 0.5) * pow(10.0, 6.0 * rnd() - 3.0); };
  for (int c : {0, 1, 7, 64}) {
    Dense vars, p, r;
    for (Dense *d : {&vars, &p, &r}) {
      d->resize(c);
      for (std::vector<double> *v : {&d->z, &d->s, &d->t, &d->zs, &d->zt})
        for (double &e : *v) e = val();
    }
    std::vector<double> apx(c > 0 ? c : 1);
    for (double &v : apx) v = val();
    Dense want = r;
    for (int i = 0; i < c; i++) {
      want.z[i] = r.z[i] - (apx[i] - p.s[i] + p.t[i]);
      want.s[i] = r.s[i] + (p.zs[i] - p.z[i]);
      want.t[i] = r.t[i] + (p.zt[i] + p.z[i]);
      want.zs[i] = r.zs[i] - (p.s[i] * vars.zs[i] + vars.s[i] * p.zs[i]);
      want.zt[i] = r.zt[i] - (p.t[i] * vars.zt[i] + vars.t[i] * p.zt[i]);
    }
    denseResStep(vars, p, apx.data(), r);
    CHECK(same_bits(r.z, want.z) && same_bits(r.s, want.s) && same_bits(r.t, want.t) &&
          same_bits(r.zs, want.zs) && same_bits(r.zt, want.zt));
  }
}

static void analyse(int64_t n, const std::vector<int> &rowp, const std::vector<int> &cols, bool expect_ok) {
  CsrSymbolic sym;
  const int64_t w = (int64_t)rowp.size() - 1;
  const int rc = csr_analyse(n, w, rowp.data(), cols.data(), &sym);
  CHECK((rc == PO_OK) == expect_ok);
  if (rc != PO_OK) return;
  CHECK((int64_t)sym.perm.size() == w);
  std::vector<char> seen(w, 0);
  for (int64_t i = 0; i < w; i++) {
    CHECK(sym.perm[i] >= 0 && sym.perm[i] < w);
    if (sym.perm[i] >= 0 && sym.perm[i] < w) seen[sym.perm[i]] = 1;
  }
  for (int64_t i = 0; i < w; i++) CHECK(seen[i]);
  CHECK(sym.nnzL >= w && sym.nnzL >= sym.nnzS - 0 * w);
  CHECK((int64_t)sym.Lrowp.size() == w + 1 && sym.Lrowp[w] == sym.nnzL);
  for (int64_t i = 0; i < w; i++) {
    CHECK(sym.Lrowp[i + 1] > sym.Lrowp[i]);
    CHECK(sym.Lcols[sym.Lrowp[i + 1] - 1] == (int)i);  // the diagonal closes the row
    for (int q = sym.Lrowp[i]; q < sym.Lrowp[i + 1] - 1; q++) CHECK(sym.Lcols[q] < sym.Lcols[q + 1]);
  }
}

static void test_csr() {
  {  // chain, span 2 stride 1 (examples/rosenbrock/sparse_rosenbrock.cpp)
    const int n = 500;
    std::vector<int> rowp, cols;
    for (int i = 0; i + 1 < n; i++) {
      rowp.push_back((int)cols.size());
      cols.push_back(i);
      cols.push_back(i + 1);
    }
    rowp.push_back((int)cols.size());
    analyse(n, rowp, cols, true);
  }
  {  // 2-D grid of pairwise constraints (fronts), reversed column order inside the rows
    const int nx = 24, ny = 17;
    std::vector<int> rowp, cols;
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        if (i + 1 < nx) {
          rowp.push_back((int)cols.size());
          cols.push_back(j * nx + i + 1);
          cols.push_back(j * nx + i);
        }
        if (j + 1 < ny) {
          rowp.push_back((int)cols.size());
          cols.push_back((j + 1) * nx + i);
          cols.push_back(j * nx + i);
        }
      }
    rowp.push_back((int)cols.size());
    analyse(nx * ny, rowp, cols, true);
  }
  for (int trial = 0; trial < 20; trial++) {  // random patterns with empty and long rows
    const int n = 40 + (int)(rnd() * 200), w = 1 + (int)(rnd() * 120);
    std::vector<int> rowp, cols;
    for (int r = 0; r < w; r++) {
      rowp.push_back((int)cols.size());
      const int len = (r % 11 == 0) ? 0 : (r % 17 == 1 ? n / 2 : 1 + (int)(rnd() * 6));
      std::vector<char> used(n, 0);
      for (int k = 0; k < len; k++) {
        int c = (int)(rnd() * n);
        while (used[c]) c = (c + 1) % n;
        used[c] = 1;
        cols.push_back(c);
      }
    }
    rowp.push_back((int)cols.size());
    analyse(n, rowp, cols, true);
  }
  {  // malformed input is refused, not read out of bounds
    std::vector<int> rowp = {0, 2, 4}, cols = {0, 1, 1, 7};
    analyse(4, rowp, cols, false);  // column index 7 >= n
    std::vector<int> rowp2 = {0, 3, 2}, cols2 = {0, 1, 2};
    analyse(4, rowp2, cols2, false);  // decreasing row pointer
    std::vector<int> rowp3 = {0, 2}, cols3 = {1, 1};
    analyse(4, rowp3, cols3, false);  // duplicate column in a row
  }
}

static void test_options() {
  Options o;
  o.addTrustRegionDefaults();
  o.addMMADefaults();
  CHECK(o.set("qn_subspace_size", 17) == PO_OK && o.integer("qn_subspace_size") == 17);
  CHECK(o.set("qn_subspace_size", -1) != PO_OK && o.integer("qn_subspace_size") == 17);  // out of range
  CHECK(o.set("abs_res_tol", 1e-9) == PO_OK && o.real("abs_res_tol") == 1e-9);
  CHECK(o.set("abs_res_tol", -1.0) != PO_OK);
  CHECK(o.set("abs_res_tol", 3) != PO_OK);            // wrong type
  CHECK(o.set("qn_type", "sr1") == PO_OK && std::string(o.str("qn_type")) == "sr1");
  CHECK(o.set("qn_type", "newton") != PO_OK);          // not a value of the enum
  CHECK(o.set("qn_type", (const char *)nullptr) != PO_OK);
  CHECK(o.set("no_such_option", 1) != PO_OK);
  CHECK(o.set("no_such_option", 1.0) != PO_OK);
  CHECK(o.set("no_such_option", "x") != PO_OK);
  CHECK(o.set("use_line_search", 5) == PO_OK && o.integer("use_line_search") == 1);  // booleans normalise
  CHECK(o.set("output_file", (const char *)nullptr) == PO_OK && std::string(o.str("output_file")).empty());
  CHECK(o.set("tr_max_size", 2.5) == PO_OK && o.set("mma_max_iterations", 7) == PO_OK);
  std::string longname(4000, 'x');
  CHECK(o.set(longname.c_str(), 1) != PO_OK);  // the error text is truncated, not overrun
}

int main() {
  test_lu();
  test_bordered();
  test_dense_res_step();
  test_csr();
  test_options();
  if (fails) {
    fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  printf("host_sanitize: ok\n");
  return 0;
}
