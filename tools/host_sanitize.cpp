// Host-side C++ of the product under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only, no GPU, no HIP
// runtime): the in-repo LU (lu.cpp, the reference's dgetrf/dgetrs sites), the dense algebra of the bordered KKT solve
// and of the linearised KKT residual (bordered.cpp), the one-time symbolic analysis of the sparse Cholesky
// (csr.cpp::csr_analyse, both factor kinds; sparse_chol.cpp::chol_analyse with and without packed groups), the option
// registry (options.cpp), the owning device array DevArray (core.hpp) and the work-vector owner of the MMA entries
// (WorkVecs, qn.hpp, over vec_new / vec_decref of qn.cpp) over malloc-backed stand-ins for the runtime calls they
// make.  Built by
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
#include "qn.hpp"

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

// the multifrontal analysis of the same pattern: a permutation, supernodes that cover it, every entry of S0 inside L
static void analyse_multifrontal(int64_t n, const std::vector<int> &rowp, const std::vector<int> &cols, bool expect_ok) {
  CsrSymbolic sym;
  const int64_t w = (int64_t)rowp.size() - 1;
  const int rc = csr_analyse(n, w, rowp.data(), cols.data(), &sym, 0, PO_SPARSE_FACTOR_MULTIFRONTAL);
  CHECK((rc == PO_OK) == expect_ok);
  if (rc != PO_OK) return;
  const CholSymbolic &c = sym.chol;
  CHECK(sym.factor_kind == PO_SPARSE_FACTOR_MULTIFRONTAL && c.n == (int)w && sym.Lrowp.empty());
  CHECK((int64_t)sym.perm.size() == w && (int64_t)sym.iperm.size() == w);
  for (int64_t i = 0; i < w; i++) CHECK(sym.perm[i] >= 0 && sym.perm[i] < w && sym.iperm[sym.perm[i]] == (int)i);
  CHECK((int)c.sn_first.size() == c.nsn + 1 && c.sn_first[0] == 0 && c.sn_first[c.nsn] == (int)w);
  CHECK((int64_t)sym.ent_off.size() == sym.nnzS && sym.ent_a.size() == sym.ent_off.size());
  for (int64_t off : sym.ent_off) CHECK(off >= 0 && off < c.Lsize);
}

// chol_analyse on a tridiagonal of 40 (both triangles by columns, as a caller passes a matrix): without packing, and with a positive cap on the
// packed groups (switch 38, which chol_analyse reads)
static void test_chol_analyse() {
  const int n = 40;
  std::vector<int> colp(1, 0), rows;
  for (int j = 0; j < n; j++) {
    if (j > 0) rows.push_back(j - 1);
    rows.push_back(j);
    if (j + 1 < n) rows.push_back(j + 1);
    colp.push_back((int)rows.size());
  }
  for (int cap : {0, 16}) {
    dbg_switch_set(SW_CHOL_PACK, cap);
    CholSymbolic c;
    CHECK(chol_analyse(n, colp.data(), rows.data(), PO_ORDER_ND, nullptr, &c) == PO_OK);
    CHECK(c.n == n && c.pack_cap == cap && (int)c.perm.size() == n);
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; i++) {
      CHECK(c.perm[i] >= 0 && c.perm[i] < n && c.iperm[c.perm[i]] == i);
      if (c.perm[i] >= 0 && c.perm[i] < n) seen[c.perm[i]] = 1;
    }
    for (int i = 0; i < n; i++) CHECK(seen[i]);
    CHECK((int)c.sn_first.size() == c.nsn + 1 && c.sn_first[c.nsn] == n && c.nnzL >= 2 * n - 1);
    // of each entry the copy that is lower after the permutation is read: 2 n - 1 places in L, one source each
    CHECK((int)c.asm_dst.size() == 2 * n - 1 && c.asm_src.size() == c.asm_dst.size() &&
          c.asm_ptr.size() == c.asm_dst.size() + 1);
    for (int64_t off : c.asm_dst) CHECK(off >= 0 && off < c.Lsize);
    // every front is either in a packed group or in its level's list, once
    size_t packed = 0;
    for (size_t g = 0; g < c.grp_first.size(); g++) packed += (size_t)(c.grp_root[g] - c.grp_first[g] + 1);
    CHECK(cap > 0 ? !c.grp_first.empty() : c.grp_first.empty());
    CHECK(packed + c.lev_sn.size() == (size_t)c.nsn);
    int counts[CHF_COUNT];
    chol_kernel_forms(c, 40, counts);
    CHECK((counts[CHF_PACK_FACTOR] > 0) == (cap > 0));
    // the retained matrix's table: 40 diagonal and 39 off-diagonal values, each of the latter in two rows
    chol_matrix_table(&c);
    CHECK((int)c.mat_rowp.size() == n + 1 && c.mat_rowp[n] == 3 * n - 2 && c.mat_maxrow == 3 && c.mat_long.empty());
    CHECK(c.mat_col.size() == c.mat_vidx.size() && (int)c.mat_col.size() == c.mat_rowp[n]);
    for (int i = 0; i < n; i++) {
      for (int p = c.mat_rowp[i]; p < c.mat_rowp[i + 1]; p++) {
        CHECK(c.mat_col[p] >= 0 && c.mat_col[p] < n && c.mat_vidx[p] >= 0 && c.mat_vidx[p] < 2 * n - 1);
        if (p > c.mat_rowp[i]) CHECK(c.mat_col[p] > c.mat_col[p - 1]);
      }
    }
    // with a Schur set (one index, 8 scattered unsorted ones, 33): the set ends perm in the order given, its supernode is
    // the last and in no list, and every entry of the two gather tables lies inside its arena
    const std::vector<std::vector<int>> sets = {{13}, {31, 2, 17, 39, 0, 8, 25, 20}, {}};
    for (std::vector<int> sc : sets) {
      if (sc.empty()) {
        for (int k = 0; k < 33; k++) sc.push_back((7 * k + 3) % n);
      }
      for (int order : {PO_ORDER_ND, PO_ORDER_NATURAL}) {
        CholSymbolic s;
        CHECK(chol_analyse(n, colp.data(), rows.data(), order, nullptr, (int64_t)sc.size(), sc.data(), &s) == PO_OK);
        const int ns = (int)sc.size(), S = s.schur_sn;
        CHECK(s.ns == ns && S == s.nsn - 1 && s.sn_first[S] == n - ns && s.sn_b[S] == 0);
        for (int k = 0; k < ns; k++) CHECK(s.perm[n - ns + k] == sc[k]);
        for (int J : s.lev_sn) CHECK(J != S);
        for (size_t g = 0; g < s.grp_root.size(); g++) CHECK(s.grp_root[g] < S);
        CHECK(s.schur_ptr.size() == s.schur_dst.size() + 1 && s.schur_vptr.size() == (size_t)ns + 1);
        CHECK(s.schur_ptr.back() == (int64_t)s.schur_src.size() && s.schur_vptr.back() == (int64_t)s.schur_vsrc.size());
        for (int64_t off : s.schur_src) CHECK(off >= 0 && off < s.arena);
        for (int64_t off : s.schur_dst) CHECK(off >= s.panel_off[S] && off < s.Lsize);
        for (size_t q = 0; q < s.schur_vsrc.size(); q++) {
          CHECK(s.schur_vsrc[q] >= 0 && s.schur_vsrc[q] + (int64_t)(kCholMaxRhs - 1) * s.schur_vld[q] < s.sol_arena);
        }
        int extra[CHF_SCHUR_COUNT];
        chol_schur_forms(s, 40, extra);
        CHECK(extra[CHF_SCHUR_GATHER] == (s.schur_dst.empty() ? 0 : 1) && extra[CHF_SCHUR_FWD] == 2 * extra[CHF_SCHUR_GATHER]);
      }
    }
    std::vector<int> twice = {4, 9, 4}, outside = {4, n};
    CholSymbolic refused;
    CHECK(chol_analyse(n, colp.data(), rows.data(), PO_ORDER_ND, nullptr, 3, twice.data(), &refused) == PO_ERR_ARG);
    CHECK(chol_analyse(n, colp.data(), rows.data(), PO_ORDER_ND, nullptr, 2, outside.data(), &refused) == PO_ERR_ARG);
  }
  dbg_switch_set(SW_CHOL_PACK, -1);
}

static void analyse(int64_t n, const std::vector<int> &rowp, const std::vector<int> &cols, bool expect_ok) {
  analyse_multifrontal(n, rowp, cols, expect_ok);
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

// Stand-ins for the runtime calls of DevArray: "device" memory is the heap, so the sanitizers see every byte of it.
static long g_dev_allocs = 0;
static long g_fail_alloc_in = 0;  // > 0: the allocation that many calls from now fails
static long g_stream_syncs = 0;
extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) {
  if (g_fail_alloc_in > 0 && --g_fail_alloc_in == 0) return hipErrorOutOfMemory;
  *ptr = malloc(size ? size : 1);
  g_dev_allocs++;
  return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *ptr) {
  if (ptr) g_dev_allocs--;
  free(ptr);
  return hipSuccess;
}
hipError_t hipMemset(void *dst, int value, size_t sizeBytes) {
  memset(dst, value, sizeBytes);
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t sizeBytes, hipMemcpyKind) {
  memcpy(dst, src, sizeBytes);
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int value, size_t sizeBytes, hipStream_t) {
  memset(dst, value, sizeBytes);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  g_stream_syncs++;
  return hipSuccess;
}
}

static void test_dev_array() {
  const long long base = live_bytes().load();
  {
    DevArray<double> empty;  // destroyed empty
    CHECK(empty.get() == nullptr && empty.size() == 0 && !empty);
    empty.reset();
    DevArray<double> a;
    CHECK(a.alloc(10, true) == PO_OK && a.size() == 10);
    CHECK(live_bytes().load() == base + 80);
    for (int i = 0; i < 10; i++) CHECK(a[i] == 0.0);
    double *raw = a;
    CHECK(raw == a.get());
    DevArray<int> t;
    const std::vector<int> v3 = {1, 2, 3};
    CHECK(t.upload(v3) == PO_OK && t.size() == 7);  // size() + 4, zero-filled, then the copy
    for (int i = 0; i < 7; i++) CHECK(t[i] == (i < 3 ? i + 1 : 0));
    CHECK(live_bytes().load() == base + 80 + 28);
    const std::vector<int> v9 = {9, 8, 7, 6, 5, 4, 3, 2, 1};
    CHECK(t.upload(v9) == PO_OK && t.size() == 13 && t[8] == 1 && t[12] == 0);  // over a live array
    CHECK(t.upload(std::vector<int>()) == PO_OK && t.size() == 4 && t[3] == 0);  // an empty table: the padding alone
    CHECK(live_bytes().load() == base + 80 + 16 && g_dev_allocs == 2);
    DevArray<double> b(std::move(a));  // move construction
    CHECK(a.get() == nullptr && a.size() == 0 && b.get() == raw && b.size() == 10);
    DevArray<double> c;
    CHECK(c.alloc(3, false) == PO_OK);
    c = std::move(b);  // move assignment over a live array: its own memory is freed
    CHECK(b.get() == nullptr && c.get() == raw && c.size() == 10 && g_dev_allocs == 2);
    CHECK(live_bytes().load() == base + 80 + 16);
    t.reset();
    CHECK(t.get() == nullptr && t.size() == 0 && live_bytes().load() == base + 80);
    t.reset();  // twice is once
    struct Group {  // what CsrSparse does with its dense columns: an empty group assigned over a full one
      DevArray<double> x, y;
    } g;
    CHECK(g.x.alloc(5, true) == PO_OK && g.y.alloc(6, false) == PO_OK && g_dev_allocs == 3);
    g = Group();
    CHECK(g.x.get() == nullptr && g_dev_allocs == 1);
  }  // c is destroyed full
  CHECK(live_bytes().load() == base && g_dev_allocs == 0);
}

// the work vectors of an MMA entry: m + 1 of them, a failure in the middle, release with and without vectors held
static void test_work_vecs() {
  Ctx *ctx = new Ctx();
  long vecs0 = 0, vecs = 0;
  live_objects(&vecs0, nullptr);
  const int m = 5;
  {
    WorkVecs work(ctx);
    g_stream_syncs = 0;
    CHECK(work.release(PO_OK) == PO_OK && work.release(PO_ERR_ARG) == PO_ERR_ARG && g_stream_syncs == 0);  // empty
    CHECK(work.add(m + 1, 37) == PO_OK && work.v.size() == (size_t)m + 1);
    live_objects(&vecs, nullptr);
    CHECK(vecs == vecs0 + m + 1);
    for (int i = 0; i <= m; i++)
      for (int j = 0; j < 37; j++) CHECK(work.d(i)[j] == 0.0);
    const std::vector<double *> G = work.pointers(1, m);
    CHECK((int)G.size() == m && G[0] == work.d(1) && G[m - 1] == work.d(m));
    g_stream_syncs = 0;
    CHECK(work.release(PO_ERR_USER) == PO_ERR_USER && g_stream_syncs >= 1 && work.v.empty());  // the code is handed on
    live_objects(&vecs, nullptr);
    CHECK(vecs == vecs0);
    g_fail_alloc_in = 3;  // the third of m + 1 allocations fails: two vectors are held, and released
    CHECK(work.add(m + 1, 37) == PO_ERR_HIP && work.v.size() == 2);
    g_fail_alloc_in = 0;
    CHECK(work.add(2, 0) == PO_OK && work.v.size() == 4);  // (empty vectors, and a second group behind the first)
  }  // destroyed holding vectors
  live_objects(&vecs, nullptr);
  CHECK(vecs == vecs0 && g_dev_allocs == 0);
  delete ctx;
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
  test_chol_analyse();
  test_dev_array();
  test_work_vecs();
  test_options();
  if (fails) {
    fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  printf("host_sanitize: ok\n");
  return 0;
}
