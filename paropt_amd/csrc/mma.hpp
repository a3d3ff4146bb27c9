// Host-side mirror of ParOptMMA (reference src/ParOptMMA.h:22-192, src/ParOptMMA.cpp): the method of
// moving asymptotes.  The object is BOTH the separable rational subproblem -- a ParOptProblem handed
// to the interior-point solver, with its diagonal Hessian (use_diag_hessian = 1, use_line_search = 0,
// .cpp:344-346) -- and the outer driver.  Every n-sized operation is an element-wise kernel (mma.hip)
// or one of the reductions of the interior-point path; the subproblem's objective / constraint values
// are two mdot passes over the coefficient panels [p0 | p_i] and [q0 | q_i].
#pragma once
#include <string>
#include <vector>

#include "ip.hpp"

namespace po {

struct MmaParams {
  double movlim, init_off, contract, relax, min_off, max_off, eps, delta;
};
int k_mma_asymptotes(Ctx *c, const double *x, const double *x1, const double *x2, const double *lb,
                     const double *ub, const MmaParams &p, int first, int64_t n, double *L, double *U);
int k_mma_coef(Ctx *c, const double *x, const double *lb, const double *ub, const double *L, const double *U,
               const double *g, const MmaParams &p, int64_t n, double *alpha, double *beta, double *p0,
               double *q0);
// pi = (U-x)^2 max(0,-A), qi = (x-L)^2 max(0,A) ; *bsum = sum pi/(U-x) + qi/(x-L)
int k_mma_pq(Ctx *c, const double *x, const double *L, const double *U, const double *A, int64_t n, double *pi,
             double *qi, double *bsum);
int k_mma_inv(Ctx *c, const double *x, const double *L, const double *U, int64_t n, double *uinv, double *linv);
// out_0 = ui^2 P_0 - li^2 Q_0 ; out_j = li^2 Q_j - ui^2 P_j (j >= 1)
int k_mma_grad(Ctx *c, const double *x, const double *L, const double *U, const double *const *P,
               const double *const *Q, int nv, int64_t n, double *const *out);
// h = 2 sum_j w_j (ui^3 P_j + li^3 Q_j)
int k_mma_hdiag(Ctx *c, const double *x, const double *L, const double *U, const double *const *P,
                const double *const *Q, const double *w, int nv, int64_t n, double *h);


// ---- the dual of the separable subproblem (mma.hip) ----------------------------------------------------------------
constexpr int kMmaDualFused = 8;  // M_F: widest m whose m (m + 1) / 2 Hessian sums ride in the pass (no scratch, no spill)
constexpr int kMmaDualMax = kMaxPanel - 1;
struct MmaDualData {  // one subproblem: device pointers of n elements, m column pairs, b[m] on the host
  const double *L, *U, *alpha, *beta, *p0, *q0;
  const double *const *p, *const *q;
  const double *b;
  int m;
  int64_t n;
};
// W(lambda), grad[m] and, when H != nullptr, H[m * m] = -hess W (symmetric, column-major); collective.
// form 0: value and gradient only; 1: the Hessian sums in the same pass (m <= kMmaDualFused); 2: the pass stores the
// columns G_i = p_i u^2 - q_i l^2 in G[i] and the weights [free] / h in dvec, H = G^T diag(dvec) G by k_wgram.
// W and grad have the same bits in every form.
// r != nullptr: the rho form (mma_globalization = conservative) -- every approximation carries rho_i d(x) around the
// expansion point xk; *D (optional) receives d at the primal point.  With every rho_i = 0: the bits of the plain form.
struct MmaDualRho {
  const double *xk;   // device, n elements
  const double *rho;  // host, m + 1 values: the objective's, then one per constraint
};
int k_mma_dual(Ctx *c, const MmaDualData &s, const double *lambda, int form, double *W, double *grad, double *H,
               double *const *G, double *dvec, const MmaDualRho *r = nullptr, double *D = nullptr);
// the point pass of the rho form: x, zl, zu at lambda and sums[m + 2] = {Delta_0, Delta_1..m, D},
// Delta_i = f~_i(x) - f~_i(xk) without the rho term, D = d(x); collective
int k_mma_gcmma_point(Ctx *c, const MmaDualData &s, const MmaDualRho &r, const double *lambda, double *x, double *zl,
                      double *zu, double *sums);
// sums[m + 1] = {sum |g| (U - L), sum |A_i| (U - L)}: the start values of rho; collective
int k_mma_gcmma_rho_sums(Ctx *c, const double *L, const double *U, const double *g, const double *const *A, int m,
                         int64_t n, double *sums);
// the primal point and the bound multipliers at lambda
int k_mma_dual_point(Ctx *c, const MmaDualData &s, const double *lambda, double *x, double *zl, double *zu);

typedef int (*MmaIterationFn)(void *user, int iter);

class MMA : public Problem {
 public:
  explicit MMA(Problem *prob);
  ~MMA();
  Options &options() { return ip ? ip->options : opts; }
  int build();
  int optimize();

  // ParOptProblem side (:795-1052)
  bool isSubproblem() override { return true; }
  int getVarsAndBounds(Vec *x, Vec *lb, Vec *ub) override;
  int evalObjCon(Vec *x, double *fobj, double *cons) override;
  int evalObjConGradient(Vec *x, Vec *g, Vec **Ac) override;
  int evalHvecProduct(Vec *x, const double *z, Vec *zw, Vec *px, Vec *hvec) override;
  int evalHessianDiag(Vec *x, const double *z, Vec *zw, Vec *hdiag) override;
  int evalSparseCon(Vec *x, Vec *out) override;
  int addSparseJacobian(double alpha, Vec *x, Vec *px, Vec *out) override;
  int addSparseJacobianTranspose(double alpha, Vec *x, Vec *pzw, Vec *out) override;
  int addSparseInnerProduct(double alpha, Vec *x, Vec *cvec, Vec *A) override;
  int sparseJacobianPanel(Vec *x, Vec *d, const double *const *P, int nv, double *const *U,
                          Vec *work) override;
  int sparseApplyK0(Vec *, Vec *d, Vec *cw, const double *bx, const double *bw, Vec *yx, Vec *yw,
                    Vec *wwork) override {
    return prob->sparseApplyK0(xvec, d, cw, bx, bw, yx, yw, wwork);
  }
  int sparseFactor(Vec *, Vec *d, Vec *cw) override { return prob->sparseFactor(xvec, d, cw); }
  int sparseHalfSolve(double *const *U, int nv, Vec *cw, const double **weights) override {
    return prob->sparseHalfSolve(U, nv, cw, weights);
  }
  bool sparseUserSolver() override { return prob->sparseUserSolver(); }
  int sparseSolvedPanel(const double *const *P, int nv, double *const *Yw, Vec *work) override {
    return prob->sparseSolvedPanel(P, nv, Yw, work);
  }
  const char *sparseFactorInfo() override { return prob->sparseFactorInfo(); }
  long sparseFactorBreakdowns() override { return prob->sparseFactorBreakdowns(); }
  int sparseCorrection(const double *const *U, int nv, const double *alpha, Vec *cw, Vec *out, Vec *acc) override {
    return prob->sparseCorrection(U, nv, alpha, cw, out, acc);
  }

  Problem *prob;
  Options opts;
  InteriorPoint *ip;
  int m;
  int use_true_mma, mma_iter, subproblem_iter;
  Vec *xvec, *x1vec, *x2vec, *lbvec, *ubvec, *gvec, *Lvec, *Uvec, *alphavec, *betavec, *p0vec, *q0vec, *rvec,
      *zlvec, *zuvec, *uinv, *linv, *cwvec, *zwvec;
  std::vector<Vec *> Avecs, pivecs, qivecs;
  double fobj;
  std::vector<double> cons, b, z;
  std::string history;
  MmaIterationFn iter_cb;
  void *iter_cb_user;
  double last_row[5];  // fobj, l1, linfty, l1_lambda, infeas of the last table row
  // mma_subproblem_solver = dual: the subproblem is solved through its dual (mma_dual.hpp) -- no InteriorPoint object
  bool use_dual;
  std::vector<Vec *> Gvecs;  // the m columns of the panel form (m > kMmaDualFused only)
  int dual_solves, dual_iterations, dual_evaluations, dual_last_status;
  double dual_last_pg;
  MmaDualData dualData();
  // mma_globalization = conservative (mma_gcmma.hpp; dual sub-solver only): raises of rho so far, in the last MMA
  // iteration and the most in one, iterations that spent mma_gcmma_max_inner raises, and the m + 1 values of rho the
  // last iteration was accepted with
  int gcmma_inner_total, gcmma_inner_last, gcmma_inner_max, gcmma_cap_hits;
  std::vector<double> gcmma_rho;

 private:
  MmaParams params() ;
  int allocate();
  int initializeSubProblem(Vec *xv);
  int computeKKTError(double *l1, double *linfty, double *infeas);
  void setMultipliers();
  int checkDualCovers();
  int solveDual(const double *rho = nullptr, double *point_sums = nullptr);
  int solveConservative();
  bool have_trial_values;  // fobj_trial / cons_trial hold the problem's values at the point initializeSubProblem takes
  double fobj_trial;
  std::vector<double> cons_trial;
  void flushHistory();
};

}  // namespace po

struct po_mma_s {
  po::MMA *mma;
  std::vector<po_vec> p, q;  // the handle arrays po_mma_get_subproblem hands out
};
