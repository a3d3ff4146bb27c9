// The dense algebra of the bordered (Schur-complement) KKT solve, shared by the four solves of the interior point
// (solveKKT, solveKKTW, solveKKTAlpha, solveKKTAlphaW).  With the panel P = [Ac | Z] (c constraint gradients, k
// quasi-Newton columns) and the weighted Gram W = P^T Dinv P, the solves need only (c+k)-sized algebra on the host
// besides their passes over P:
//   G  = W_AA + diag(s/zs + t/zt)                       (src/ParOptInteriorPoint.cpp:1952-1970)
//   Ce = W_ZZ - W_ZA G^-1 W_AZ - M / (d0 d0^T)          (:2634-2667 via SURVEY.md 3.4)
//   yz = G^-1 (alpha d3 - A t), zeta = Ce^-1 (Z^T t + W_ZA yz), yz2 = G^-1 (-W_AZ zeta)   (:2150-2159)
// and the dense rows of the linearised KKT residual at a step (addKKTResStep :1529-1535).
// No device calls: tools/host_sanitize.cpp checks it on the CPU.
#pragma once
#include <vector>

namespace po {

struct Dense {  // the c-sized blocks of ParOptVars (src/ParOptInteriorPoint.h:373-389)
  std::vector<double> z, s, t, zs, zt;
  void resize(int c) {
    z.assign(c, 0.0);
    s.assign(c, 0.0);
    t.assign(c, 0.0);
    zs.assign(c, 0.0);
    zt.assign(c, 0.0);
  }
};

struct Bordered {
  int c = 0, k = 0;             // k: quasi-Newton columns when W was assembled
  std::vector<double> W;        // (c+k)^2 weighted Gram, column-major
  std::vector<double> Gf, Cef;  // LU factors of G and Ce
  std::vector<int> gpiv, cpiv;

  // what one solve produces: coef = (yz - yz2, -zeta) are the panel coefficients, px = t + Dinv o (P coef)
  struct Sol {
    std::vector<double> yz, yz2, zeta, coef;
  };

  // G, Ce and their LU factors from W and the slacks `vars`; d0, M: the compact quasi-Newton matrices (read when
  // k > 0).  G0 / Ce0 (may be null) receive the matrices as assembled (Ce0 only when k > 0).
  void factor(const Dense &vars, const double *d0, const double *M, std::vector<double> *G0 = nullptr,
              std::vector<double> *Ce0 = nullptr);
  // PO_ERR_ARG (with the error text) unless the panel still has the width W was assembled with
  int checkWidth(int k_now) const;
  // the dense blocks of the right-hand side scaled by alpha (1 on the plain paths), dots = P^T t
  void solve(double alpha, const Dense &b, const Dense &vars, const double *dots, Sol *s) const;
  // P^T px = dots + W coef, assigned or (refinement pass) accumulated into ptpx
  void panelDots(const double *dots, const Sol &s, bool accumulate, std::vector<double> *ptpx) const;
  // the dense blocks of the step; full: with the quasi-Newton correction yz2 (the GMRES loop leaves it out)
  void backSubstitute(double alpha, const Dense &b, const Dense &vars, const Sol &s, bool full, Dense &out) const;
};

// r -= the dense rows of the KKT matrix applied to the step p (addKKTResStep :1529-1535); apx = A px
void denseResStep(const Dense &vars, const Dense &p, const double *apx, Dense &r);

}  // namespace po
