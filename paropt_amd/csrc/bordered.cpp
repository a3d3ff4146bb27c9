// Dense algebra of the bordered KKT solve (bordered.hpp).  The loops keep one summation order: every rank and
// every solve path gets the same bits.
#include "bordered.hpp"

#include "core.hpp"

namespace po {

void Bordered::factor(const Dense &vars, const double *d0, const double *M, std::vector<double> *G0,
                      std::vector<double> *Ce0) {
  const int m = c + k;
  Gf.assign((size_t)c * c, 0.0);
  gpiv.assign(c, 0);
  for (int j = 0; j < c; j++)
    for (int i = 0; i < c; i++) Gf[i + (size_t)c * j] = W[i + (size_t)m * j];
  for (int i = 0; i < c; i++) Gf[(size_t)i * (c + 1)] += vars.s[i] / vars.zs[i] + vars.t[i] / vars.zt[i];
  if (G0) *G0 = Gf;
  if (c > 0) lu_factor(c, Gf.data(), c, gpiv.data());
  Cef.clear();
  cpiv.clear();
  if (k == 0) return;
  Cef.assign((size_t)k * k, 0.0);
  cpiv.assign(k, 0);
  std::vector<double> col(c > 0 ? c : 1);
  for (int j = 0; j < k; j++) {
    for (int i = 0; i < c; i++) col[i] = W[i + (size_t)m * (c + j)];  // W_AZ[:, j]
    if (c > 0) lu_solve(c, Gf.data(), c, gpiv.data(), col.data());
    for (int i = 0; i < k; i++) {
      double v = W[(c + i) + (size_t)m * (c + j)];
      for (int l = 0; l < c; l++) v -= W[(c + i) + (size_t)m * l] * col[l];
      v -= M[i + (size_t)k * j] / (d0[i] * d0[j]);
      Cef[i + (size_t)k * j] = v;
    }
  }
  if (Ce0) *Ce0 = Cef;
  lu_factor(k, Cef.data(), k, cpiv.data());
}

int Bordered::checkWidth(int k_now) const {
  if (k_now == k) return PO_OK;
  set_error("internal: panel width changed between setUpKKTSystem and solve (%d vs %d)", k_now, k);
  return PO_ERR_ARG;
}

void Bordered::solve(double alpha, const Dense &b, const Dense &vars, const double *dots, Sol *s) const {
  const int m = c + k;
  s->yz.assign(c > 0 ? c : 1, 0.0);
  s->yz2.assign(c > 0 ? c : 1, 0.0);
  s->zeta.assign(k > 0 ? k : 1, 0.0);
  std::vector<double> &yz = s->yz, &yz2 = s->yz2, &zeta = s->zeta;
  // yz = G^-1 (alpha d3 - A t)
  for (int i = 0; i < c; i++) {
    yz[i] = alpha * (b.z[i] + (b.zs[i] + vars.s[i] * b.s[i]) / vars.zs[i] -
                     (b.zt[i] + vars.t[i] * b.t[i]) / vars.zt[i]) -
            dots[i];
  }
  if (c > 0) lu_solve(c, Gf.data(), c, gpiv.data(), yz.data());
  if (k > 0) {
    // Z^T px0 = Z^T t + W_ZA yz ; zeta = Ce^-1 (Z^T px0) ; yz2 = G^-1 (-W_AZ zeta)
    for (int i = 0; i < k; i++) {
      double v = dots[c + i];
      for (int l = 0; l < c; l++) v += W[(c + i) + (size_t)m * l] * yz[l];
      zeta[i] = v;
    }
    lu_solve(k, Cef.data(), k, cpiv.data(), zeta.data());
    for (int i = 0; i < c; i++) {
      double v = 0.0;
      for (int j = 0; j < k; j++) v += W[i + (size_t)m * (c + j)] * zeta[j];
      yz2[i] = -v;
    }
    if (c > 0) lu_solve(c, Gf.data(), c, gpiv.data(), yz2.data());
  }
  s->coef.assign(m > 0 ? m : 1, 0.0);
  for (int i = 0; i < c; i++) s->coef[i] = yz[i] - yz2[i];
  for (int j = 0; j < k; j++) s->coef[c + j] = -zeta[j];
}

void Bordered::panelDots(const double *dots, const Sol &s, bool accumulate, std::vector<double> *ptpx) const {
  const int m = c + k;
  if (!accumulate) ptpx->assign(m > 0 ? m : 1, 0.0);
  for (int i = 0; i < m; i++) {
    double v = dots[i];
    for (int j = 0; j < m; j++) v += W[i + (size_t)m * j] * s.coef[j];
    (*ptpx)[i] = accumulate ? (*ptpx)[i] + v : v;
  }
}

void Bordered::backSubstitute(double alpha, const Dense &b, const Dense &vars, const Sol &s, bool full,
                              Dense &out) const {
  // full solve (:2165-2170) minus the bx-only solve (:2300-2305)
  for (int i = 0; i < c; i++) {
    const double yz = s.yz[i], y2 = full ? s.yz2[i] : 0.0;
    const double zs1 = yz - alpha * b.s[i];
    const double zt1 = -alpha * b.t[i] - yz;
    out.z[i] = yz - y2;
    out.zs[i] = zs1 - y2;
    out.zt[i] = zt1 + y2;
    out.s[i] = (alpha * b.zs[i] - vars.s[i] * zs1) / vars.zs[i] + (vars.s[i] * y2) / vars.zs[i];
    out.t[i] = (alpha * b.zt[i] - vars.t[i] * zt1) / vars.zt[i] - (vars.t[i] * y2) / vars.zt[i];
  }
}

void denseResStep(const Dense &vars, const Dense &p, const double *apx, Dense &r) {
  for (int i = 0; i < (int)r.z.size(); i++) {
    r.z[i] -= (apx[i] - p.s[i] + p.t[i]);
    r.s[i] += (p.zs[i] - p.z[i]);
    r.t[i] += (p.zt[i] + p.z[i]);
    r.zs[i] -= (p.s[i] * vars.zs[i] + vars.s[i] * p.zs[i]);
    r.zt[i] -= (p.t[i] * vars.zt[i] + vars.t[i] * p.zt[i]);
  }
}

}  // namespace po
