// Host-side mirror of ParOptMMA (reference src/ParOptMMA.h:22-192, src/ParOptMMA.cpp): the method of
// moving asymptotes.  The object is BOTH the separable rational subproblem -- a ParOptProblem handed
// to the interior-point solver, with its diagonal Hessian (use_diag_hessian = 1, use_line_search = 0,
// .cpp:344-346) -- and the outer driver.  Every n-sized operation is an element-wise kernel (mma.hip)
// or one of the reductions of the interior-point path; the subproblem's objective / constraint values
// are two mdot passes over the coefficient panels [p0 | p_i] and [q0 | q_i].
#pragma once
#include <algorithm>
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
inline MmaDualData mma_dual_data(const double *L, const double *U, const double *alpha, const double *beta,
                                 const double *p0, const double *q0, const double *const *p, const double *const *q,
                                 const double *b, int m, int64_t n) {
  return MmaDualData{L, U, alpha, beta, p0, q0, p, q, b, m, n};
}
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

// ---- the dual with grouped ("weighting") sparse constraints (mma_dual_sparse_constraints = groups) -----------------
// Group i owns the local variables start + i (nw + skip) + [0, nw); its linearised constraint is
//   psi_i(x) = a sum_{j in G_i} x_j + c_i >= 0   (= 0 from local constraint nwinequality on),
// and its multiplier zw_i lies in [zlo_i, gamma], zlo_i = 0 for an inequality, -gamma for an equality.  With
// phi_j(x) = P_j / (U_j - x) + Q_j / (x - L_j) the dual function is
//   W(lambda) = sum_groups max_zw min_x [sum_{G_i} phi_j(x_j) - zw_i psi_i(x)] + sum_ungrouped phi_j + lambda . b:
// every group is a one-dimensional root search in zw on top of one-dimensional root searches in x.
constexpr int kGroupNewtonCap = 100;  // steps of one root search (zw of a group, x of an element); hits are counted
struct MmaDualGroups {
  GroupMap map;
  double a = -1.0;            // the one value of the Jacobian's entries
  const double *c = nullptr;  // device, nwcon values
  int64_t nwinequality = 0;
  double gamma = 0.0;
};
struct MmaGroupStats {  // of one group-solve pass, over all ranks
  double zw_psi = 0.0;  // sum zw_i psi_i
  long strict = 0, at_lower = 0, at_gamma = 0, cap_hits = 0;
  long steps = 0;        // evaluations of psi over all groups
  int max_inner = 0;     // most evaluations of psi one group took
  double max_psi = 0.0;  // largest |psi| over the strict groups
  void absorb(const MmaGroupStats &o) {  // the most steps, the cap hits and the largest |psi| over both
    max_inner = std::max(max_inner, o.max_inner);
    cap_hits += o.cap_hits;
    max_psi = std::max(max_psi, o.max_psi);
  }
};
// the group map runs through the tiled solve: one constraint per group (nwblock = 1), period within a tile, every
// group inside the n local variables
bool mma_dual_groups_tile(const GroupMap &m, int64_t n);
// x (n) and zw (nwcon) at lambda; zl, zu (both or neither) receive the bound multipliers with the group term in
// r = P u^2 - Q l^2 - a zw; collective
// r != nullptr: the rho form -- P, Q gain sigma (w_U, w_L) around r->xk; the groups are affine and carry no rho
int k_mma_group_solve(Ctx *c, const MmaDualData &s, const MmaDualGroups &g, const double *lambda, double *x,
                      double *zw, double *zl, double *zu, MmaGroupStats *st, const MmaDualRho *r = nullptr);
// The evaluation: the group solve, then the sums at the stored point in the panel form (G: m columns, dvec: n), and
// with H != nullptr  H = G^T diag(dvec) G - sum over the strict groups of a_g a_g^T / s_g  (Uw: m columns of nwcon,
// sw: nwcon).  x and zw are left at the point of lambda, zl and zu (both or neither) as in the group solve; collective.
// r != nullptr: the rho form of k_mma_dual on top of the groups; *D (optional) receives d at the point.  With every
// rho_i = 0: the bits of the plain form wherever the rho form's second stop of the element search (mma.hip,
// group_el_root) does not act.
int k_mma_dual_groups(Ctx *c, const MmaDualData &s, const MmaDualGroups &g, const double *lambda, double *W,
                      double *grad, double *H, double *const *G, double *dvec, double *x, double *zw,
                      double *const *Uw, double *sw, double *zl, double *zu, MmaGroupStats *st,
                      const MmaDualRho *r = nullptr, double *D = nullptr);
// sums[m + 2] = {Delta_0, Delta_1..m, D} of k_mma_gcmma_point at a stored point x (the final group solve's): one
// read-only pass per conservative trial; collective
int k_mma_gcmma_group_sums(Ctx *c, const MmaDualData &s, const double *xk, const double *x, double *sums);

// ---- the dual with linearised constraints (mma_dual_linearized_constraints = newton) --------------------------------
// minimise sum p0 / (U - x) + q0 / (x - L) over alpha <= x <= beta subject to c_i(x) = cons_i + A_i . (x - xk) >= 0
// (= 0 for an equality).  The Lagrangian stays separable; with t = sum_i lambda_i A_i its element-wise minimiser is
// x = clamp(root of p0 u^2 - q0 l^2 = t, alpha, beta), found by the bracketed Newton iteration of the grouped
// constraints, and
//   W = sum p0 u + q0 l - sum_i lambda_i c_i(x),  dW/dlambda_i = -c_i(x),
//   -hess W = sum over the free elements of A_i A_k / h,  h = 2 (p0 u^3 + q0 l^3).
// P = p0 and Q = q0 do not depend on lambda: an equality's multiplier may take either sign.
struct MmaDualLinear {  // device pointers of n elements, m columns A_i, cons[m] on the host
  const double *L, *U, *alpha, *beta, *p0, *q0, *xk;
  const double *const *A;
  const double *cons;
  int m;
  int64_t n;
};
struct MmaLinearStats {  // the element root searches, over all ranks: accumulated by the passes below
  long cap_hits = 0;     // searches that ran into kGroupNewtonCap
  int max_steps = 0;     // most evaluations one search took
};
// W(lambda), grad[m] and, when H != nullptr, H[m * m] = -hess W (symmetric, column-major); collective.  The root
// searches start from xstart and the point is stored into x (the same vector is allowed).  form 0: value and gradient
// only; 1: the Hessian sums in the same pass (m <= kMmaDualFused); 2: the pass stores the weights [free] / h in dvec and
// H = A^T diag(dvec) A by k_wgram over the A_i themselves.  W and grad have the same bits in every form.
int k_mma_dual_linear(Ctx *c, const MmaDualLinear &s, const double *lambda, int form, const double *xstart, double *x,
                      double *W, double *grad, double *H, double *dvec, MmaLinearStats *st = nullptr);
// the primal point and the bound multipliers at lambda (r = p0 u^2 - q0 l^2 - t); collective
int k_mma_dual_linear_point(Ctx *c, const MmaDualLinear &s, const double *lambda, const double *xstart, double *x,
                            double *zl, double *zu, MmaLinearStats *st = nullptr);

typedef int (*MmaIterationFn)(void *user, int iter);
struct MmaDualResult;  // (mma_dual.hpp)

struct MmaDualStats {  // mma_subproblem_solver = dual: counters over every solve; status and max |pg| of the last one
  int solves = 0, iterations = 0, evaluations = 0, last_status = 0;
  double last_pg = 0.0;
};
// mma_globalization = conservative: raises of rho so far, in the last MMA iteration and the most in one, iterations that
// spent mma_gcmma_max_inner raises, and the m + 1 values of rho the last iteration was accepted with
struct MmaGcmmaStats {
  int inner_total = 0, inner_last = 0, inner_max = 0, cap_hits = 0;
  std::vector<double> rho;
};

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
  // the quasi-definite solver is the wrapped problem's, with its Jacobian taken at the expansion point
  Problem *sparseOwner(Vec **x) override {
    *x = xvec;
    return prob->sparseOwner(x);
  }
  // The subproblem view takes the unfused Jacobian forms, whatever the wrapped problem could fuse: Cdiag by a pass of
  // its own ahead of factor (no factorFromSlacks), the set forms as a zero fill followed by the add forms, no group
  // Gram and no described transpose column (Problem's defaults for a problem that is not `grouped` itself).  Factor,
  // apply, panel and correction are the wrapped problem's solver's.  This is what MMA has always run; results are
  // pinned to it bit for bit (tools/sparse_digest.py).
  bool sparseFusedForms() override { return false; }

  // what the C layer hands out
  int mma_iter = 0, subproblem_iter = 0;
  Vec *xvec = nullptr, *Lvec = nullptr, *Uvec = nullptr, *alphavec = nullptr, *betavec = nullptr, *p0vec = nullptr,
      *q0vec = nullptr, *zlvec = nullptr, *zuvec = nullptr, *zwvec = nullptr;
  std::vector<Vec *> pivecs, qivecs;
  double fobj = 0.0;
  std::vector<double> cons, b, z;
  std::string history;
  MmaIterationFn iter_cb = nullptr;
  void *iter_cb_user = nullptr;
  double last_row[5] = {};  // fobj, l1, linfty, l1_lambda, infeas of the last table row
  MmaDualStats dual;
  MmaGcmmaStats gcmma;
  // mma_dual_sparse_constraints = groups: the classes of the groups at the last solve's point, and over the
  // evaluations of that solve the most steps of one group, the cap hits and the largest |psi| of a strict group
  MmaGroupStats groups;
  // mma_dual_linearized_constraints = newton: the element root searches over every pass of this solver
  MmaLinearStats linear;
  // the dual of the linearised subproblem is what build() allocated for (no p_i, q_i: po_mma_get_linear_subproblem)
  bool linearDual() const { return use_linear; }
  const std::vector<Vec *> &constraintGradients() const { return Avecs; }

 private:
  // how a subproblem is solved: optimize() decides it from mma_subproblem_solver and mma_globalization.  The dual
  // modes (mma_dual.hpp, mma_gcmma.hpp) run without an InteriorPoint object
  enum class Mode { INTERIOR_POINT, DUAL, DUAL_CONSERVATIVE };
  bool optionIs(const char *name, const char *value);
  bool wantDual();
  bool wantGroups();
  bool wantGcmmaGroups();
  bool conservative();
  bool linearised();
  bool wantLinear();
  int dualForm() const { return m <= kMmaDualFused ? 1 : 2; }
  MmaParams params();
  int allocate();
  int initializeSubProblem(Vec *xv);
  int solveSubproblem(Vec **xnew);
  int computeKKTError(double *l1, double *linfty, double *infeas);
  void setMultipliers();
  int checkDualCovers();
  int solveDual(const double *rho = nullptr, double *point_sums = nullptr);
  int solveDualLinear();
  void finishDualSolve(const MmaDualResult &res, const std::vector<double> &lambda);
  int solveConservative();
  void flushHistory();

  Problem *prob;
  Options opts;
  InteriorPoint *ip = nullptr;
  int m;
  int use_true_mma = 1;
  Mode mode = Mode::INTERIOR_POINT;
  bool use_dual = false;  // the sub-solver build() allocated for
  bool use_groups = false;  // ... with the grouped sparse constraints in the dual (nwcon > 0)
  bool use_linear = false;  // ... with linearised constraints in the dual: pivecs, qivecs and Gvecs stay empty
  Vec *x1vec = nullptr, *x2vec = nullptr, *lbvec = nullptr, *ubvec = nullptr, *gvec = nullptr, *rvec = nullptr,
      *uinv = nullptr, *linv = nullptr, *cwvec = nullptr;
  // the grouped dual: c_i of psi_i = a sum x + c_i, the group sums s_g (then the Gram weights), and m columns of nwcon
  Vec *cgvec = nullptr, *swvec = nullptr;
  std::vector<Vec *> Uwvecs;
  std::vector<double *> Uw;
  MmaDualGroups grp;
  std::vector<Vec *> Avecs, Gvecs;  // Gvecs: the m columns of the panel form (dual, m > kMmaDualFused only)
  // the current subproblem as the kernels take it: device-pointer tables over vectors that live from allocate() (G:
  // build()) to the destructor.  P0p = [p0 | p_i], Q0q = [q0 | q_i], the columns alone from entry 1 on (sub.p, sub.q);
  // A = [A_i | zl | zu]; sub.b points at b above
  std::vector<const double *> P0p, Q0q, A;
  std::vector<double *> G;
  MmaDualData sub = {};
  struct {  // the problem's values at the point the next initializeSubProblem takes (the inner iteration's last trial)
    bool have = false;
    double fobj = 0.0;
    std::vector<double> cons;
  } trial;
};

}  // namespace po
