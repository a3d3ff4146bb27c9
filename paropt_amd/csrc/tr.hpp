// Host-side mirror of the reference's trust-region layer (src/ParOptTrustRegion.h:15-493,
// src/ParOptCompactEigenvalueApprox.h:9-206): the subproblem interface, the quadratic and
// compact-eigenvalue subproblems, the infeasibility (steering) problem and the SL1QP driver with the
// adaptive penalty update.  Same method names and argument meaning; every n-sized operation is a
// launch of the kernels the interior-point path already uses (mdot / panel_axpy / panel_lincomb).
#pragma once
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ip.hpp"

namespace po {

int k_tr_bounds(Ctx *c, const double *xk, const double *lb, const double *ub, double tr, int64_t n,
                double *lk, double *uk);
int k_kkt_error(Ctx *c, const double *xk, const double *lb, const double *ub, const double *t,
                double relax, int64_t n, double out[2]);

// c(s) = c0 + g0^T s + 1/2 s^T H M H^T s   (ParOptCompactEigenApprox, .cpp:23-120); M, Minv row-major
class CompactEigenApprox {
 public:
  CompactEigenApprox(Ctx *ctx, int64_t n, int N);
  ~CompactEigenApprox();
  int allocate();
  std::vector<const double *> hPointers() const;
  // the N x N products on the host (.cpp:52-64, 108-120): out = M h, and c + 1/2 h^T M h accumulated term by term
  // onto c (row by row)
  void applyM(const double *h, double *out) const;
  double quadraticForm(const double *h, double c = 0.0) const;
  int multAdd(double alpha, Vec *x, Vec *y) const;                 // y += alpha H M H^T x (.cpp:52-64)
  int evalApproximation(Vec *s, double *value) const;              // c0 + g0.s + 1/2 s^T H M H^T s; s == nullptr: c0
  int evalApproximationGradient(Vec *s, Vec *grad) const;          // g0 + H M H^T s (.cpp:108-120)
  Ctx *ctx;
  int64_t n;
  int N;
  double c0;
  Vec *g0;
  std::vector<double> M, Minv;
  std::vector<Vec *> hvecs;
  std::vector<po_vec> hhandles;
};

// B = B_qn - z0 * H M H^T as one compact matrix over [Z_qn | H]  (ParOptEigenQuasiNewton :122-291)
class EigenQuasiNewton : public CompactQuasiNewton {
 public:
  EigenQuasiNewton(CompactQuasiNewton *qn, CompactEigenApprox *eigh, int index);
  void reset() override;
  int update(Vec *s, Vec *y, int *rc) override;
  int updateMult(Vec *x, const double *z, Vec *zw) override;
  int refresh() override { return qn ? qn->refresh() : PO_OK; }
  int mult(Vec *x, Vec *y) override;
  int multAdd(double alpha, Vec *x, Vec *y) override;
  int getCompactMat(double *b0_, const double **d0_, const double **M_, Vec ***Z_) override;
  int getMaxLimitedMemorySize() override;
  void applyCompactInverse(double *rz) const override;
  int size() const override;
  double diag() const override;
  std::vector<const double *> zPointers() const override;

  CompactQuasiNewton *qn;  // borrowed, may be null
  CompactEigenApprox *eigh;
  int index;
  double z0;
  int use_qn_objective;

 private:
  int qnSize() const { return (qn && use_qn_objective) ? qn->size() : 0; }
  std::vector<double> dall, Mall;
  std::vector<Vec *> Zall;
};

class TrustRegionSubproblem : public Problem {
 public:
  TrustRegionSubproblem(Problem *p);
  virtual ~TrustRegionSubproblem();
  int allocate();
  virtual CompactQuasiNewton *getQuasiNewton() = 0;
  virtual int initModelAndBounds(double tr_size);
  virtual int setTrustRegionBounds(double tr_size);
  virtual int evalTrialStepAndUpdate(int update_flag, Vec *step, const double *z, Vec *zw, double *fobj,
                                     double *cons) = 0;
  virtual int acceptTrialStep(Vec *step, const double *z, Vec *zw) = 0;
  virtual void rejectTrialStep();
  virtual int getQuasiNewtonUpdateType() const { return qn_update_type; }
  // linear model values at a step: f = fk + gk.s, cons = ck + Ak s (one panel-dot pass)
  int evalLinearModel(Vec *step, double *f, double *cons);
  // Ac[i] <- Ak[i] in one launch for every column the solver asks for (Ac == nullptr: the solver kept the constant
  // Jacobian of the first evaluation of this solve; Ac[i] == nullptr: it kept that column, constantJacobianMask) but
  // `skip_index`, the constraint a subclass models itself (-1: none)
  int copyJacobianColumns(Vec **Ac, int skip_index);

  // ParOptProblem side, seen by the interior-point solver
  bool isSubproblem() override { return true; }
  int getVarsAndBounds(Vec *x, Vec *l, Vec *u) override;
  int evalSparseCon(Vec *step, Vec *out) override;
  int addSparseJacobian(double alpha, Vec *x, Vec *px, Vec *out) override;
  int addSparseJacobianTranspose(double alpha, Vec *x, Vec *pzw, Vec *out) override;
  int setSparseJacobianTranspose(double alpha, Vec *, Vec *pzw, Vec *out) override {
    return prob->setSparseJacobianTranspose(alpha, xk, pzw, out);
  }
  int addSparseInnerProduct(double alpha, Vec *x, Vec *cvec, Vec *A) override;
  bool sparseGramGroups(Vec *, GramGroups *g) override { return prob->sparseGramGroups(xk, g); }
  bool sparseTransposeColumn(double alpha, Vec *, Vec *pzw, GroupCol *col) override {
    return prob->sparseTransposeColumn(alpha, xk, pzw, col);
  }
  int setSparseJacobian(double alpha, Vec *, Vec *px, Vec *out) override {
    return prob->setSparseJacobian(alpha, xk, px, out);
  }
  // the quasi-definite solver is the wrapped problem's, with its Jacobian taken at the base point
  Problem *sparseOwner(Vec **x) override {
    *x = xk;
    return prob->sparseOwner(x);
  }
  int writeOutput(int iter, Vec *x) override { return prob->writeOutput(iter, x); }
  // the model evaluations issue their reductions through the internal launchers and finish with
  // BatchScope::end_then: inside the interior point's line-search batch they share its collective + host sync
  bool reductionsBatchable() override { return prob->reductionsBatchable(); }

  Problem *prob;
  int m;
  Vec *xk, *lk, *uk, *lb, *ub, *gk, *gt, *t, *xtemp;
  std::vector<Vec *> Ak, At;
  double fk, ft;
  std::vector<double> ck, ct;

 protected:
  int evalTrialPoint(Vec *step, double *fobj, double *cons);
  int lagrangianGradientDifference(const double *z, Vec *zw);  // into t (:187-205)
  void acceptModel();
  // ---- the compact model over B = b0 I - Z C Z^T (a CompactQuasiNewton), shared by the quadratic and the eigenvalue
  // subproblem:  f(s) = fk + gk.s + 1/2 (b0 s.s - (Z^T s)^T C (Z^T s)),  g(s) = gk + b0 s - Z C Z^T s
  // Columns of the model pass, rebuilt per call (acceptModel swaps buffers, a user-written subproblem re-borrows
  // its vectors): [gk | Ak], then with `zp` also [Z | extra (if any) | step]
  std::vector<const double *> modelPanel(const std::vector<const double *> *zp, const double *extra, Vec *step) const;
  // f(s) and the linear c(s) in ONE pass over modelPanel (B == nullptr: the linear model, no cache); leaves Z^T s in
  // the cache.  `modelled(Z^T s, k, extra.s)`, if given, runs where the values land, after fobj and cons are written.
  int evalCompactModel(const CompactQuasiNewton *B, const double *extra, Vec *step, double *fobj, double *cons,
                       std::function<void(const double *, int, double)> modelled = nullptr);
  // b0 s.s - sum_i rz[i] (C rz)[i], subtracted term by term in index order
  static double curvatureTerm(const CompactQuasiNewton *B, const double *rz, int k, double sts);
  // [b0 | -C rz]: the coefficients of [step | Z] in the gradient
  static std::vector<double> gradientCoefficients(const CompactQuasiNewton *B, const double *rz, int k);
  // rz = Z^T step: what evalCompactModel(step) just took, else one panel-dot pass
  int stepProducts(Vec *step, const std::vector<const double *> &zp, double *rz);
  int qn_update_type;
  // landing areas of the model reductions (the values may arrive at the flush of an enclosing batch)
  std::vector<double> eo_dots, lin_dots;
  // Z^T step of the last evalObjCon(step): evalObjConGradient at the same step buffer (the accepted trial point)
  // does not stream the panel again.  Dropped whenever the model or the quasi-Newton panel changes.
  std::vector<double> zts_cache;
  const double *zts_ptr = nullptr;
  bool zts_valid = false;
};

class QuadraticSubproblem : public TrustRegionSubproblem {  // :27-466
 public:
  QuadraticSubproblem(Problem *p, CompactQuasiNewton *qn_) : TrustRegionSubproblem(p), qn(qn_) {
    linear_constraints = 1;  // c(s) = ck + Ak s: the Jacobian is constant within a subproblem solve
  }
  CompactQuasiNewton *getQuasiNewton() override { return qn; }
  int evalTrialStepAndUpdate(int update_flag, Vec *step, const double *z, Vec *zw, double *fobj,
                             double *cons) override;
  int acceptTrialStep(Vec *step, const double *z, Vec *zw) override;
  int evalObjCon(Vec *step, double *fobj, double *cons) override;
  int evalObjConGradient(Vec *step, Vec *g, Vec **Ac) override;
  CompactQuasiNewton *qn;
};

typedef int (*EigenModelUpdate)(void *user, Vec *x, CompactEigenApprox *approx);

class EigenSubproblem : public TrustRegionSubproblem {  // ParOptCompactEigenvalueApprox.cpp:295-724
 public:
  EigenSubproblem(Problem *p, EigenQuasiNewton *approx_)
      : TrustRegionSubproblem(p), approx(approx_), update_model(nullptr), update_user(nullptr) {}
  CompactQuasiNewton *getQuasiNewton() override { return approx; }
  int initModelAndBounds(double tr_size) override;
  int evalTrialStepAndUpdate(int update_flag, Vec *step, const double *z, Vec *zw, double *fobj,
                             double *cons) override;
  int acceptTrialStep(Vec *step, const double *z, Vec *zw) override;
  int evalObjCon(Vec *step, double *fobj, double *cons) override;
  int evalObjConGradient(Vec *step, Vec *g, Vec **Ac) override;
  // every constraint model but the eigenvalue one is linear in the step
  const std::vector<char> *constantJacobianMask() override {
    const_mask.assign(m, 1);
    if (approx->index >= 0 && approx->index < m) const_mask[approx->index] = 0;
    return &const_mask;
  }
  std::vector<char> const_mask;
  EigenQuasiNewton *approx;
  EigenModelUpdate update_model;
  void *update_user;
};


// A subproblem written by the USER (round 5): the seven virtuals of ParOptTrustRegionSubproblem
// (src/ParOptTrustRegion.h:15-151) and the ParOptProblem side the interior point solves, as a callback table
// (po_trsub_create_callbacks; the facade's ParOptTrustRegionSubproblem subclasses and Python's TrustRegionSubproblem
// arrive here).  The driver and the steering problem read the linear model through the base-class members (xk, fk, gk,
// ck, Ak, lb, ub): they are BORROWED from the user's getLinearModel after every call that moves the base point.
class CallbackSubproblem : public TrustRegionSubproblem {
 public:
  CallbackSubproblem(Problem *p, const po_trsub_callbacks &cb_) : TrustRegionSubproblem(p), cb(cb_) {}
  ~CallbackSubproblem();
  int allocateModel();  // no storage of its own: borrows the user's model vectors
  CompactQuasiNewton *getQuasiNewton() override;
  int initModelAndBounds(double tr_size) override;
  int setTrustRegionBounds(double tr_size) override;
  int evalTrialStepAndUpdate(int update_flag, Vec *step, const double *z, Vec *zw, double *fobj,
                             double *cons) override;
  int acceptTrialStep(Vec *step, const double *z, Vec *zw) override;
  void rejectTrialStep() override;
  int getQuasiNewtonUpdateType() const override;
  int getVarsAndBounds(Vec *x, Vec *l, Vec *u) override;
  int evalObjCon(Vec *step, double *fobj, double *cons) override;
  int evalObjConGradient(Vec *step, Vec *g, Vec **Ac) override;
  bool reductionsBatchable() override { return false; }  // user code: every reduction returns its value at once
  // sparse_constraints_are_model: `prob` already IS the model's problem side (called with the step)
  int evalSparseCon(Vec *step, Vec *out) override {
    return cb.sparse_constraints_are_model ? prob->evalSparseCon(step, out) : TrustRegionSubproblem::evalSparseCon(step, out);
  }
  int addSparseJacobian(double alpha, Vec *x, Vec *px, Vec *out) override {
    return cb.sparse_constraints_are_model ? prob->addSparseJacobian(alpha, x, px, out)
                                           : TrustRegionSubproblem::addSparseJacobian(alpha, x, px, out);
  }
  int addSparseJacobianTranspose(double alpha, Vec *x, Vec *pzw, Vec *out) override {
    return cb.sparse_constraints_are_model ? prob->addSparseJacobianTranspose(alpha, x, pzw, out)
                                           : TrustRegionSubproblem::addSparseJacobianTranspose(alpha, x, pzw, out);
  }
  int addSparseInnerProduct(double alpha, Vec *x, Vec *cvec, Vec *A) override {
    return cb.sparse_constraints_are_model ? prob->addSparseInnerProduct(alpha, x, cvec, A)
                                           : TrustRegionSubproblem::addSparseInnerProduct(alpha, x, cvec, A);
  }
  po_trsub_callbacks cb;

  // re-reads getLinearModel (called by the driver's own entry points; po_trsub_sync_linear_model for a model the
  // user changed outside the driver)
  int syncLinearModel();

 private:
  void dropModel();
};

class InfeasSubproblem : public Problem {  // :468-650
 public:
  enum { CONSTANT_OBJECTIVE = 0, LINEAR_OBJECTIVE = 1, SUBPROBLEM_OBJECTIVE = 2 };
  enum { LINEAR_CONSTRAINT = 0, SUBPROBLEM_CONSTRAINT = 1 };
  InfeasSubproblem(TrustRegionSubproblem *sub_, int objective_, int constraint_);
  bool isSubproblem() override { return true; }
  int getVarsAndBounds(Vec *x, Vec *l, Vec *u) override { return sub->getVarsAndBounds(x, l, u); }
  int evalObjCon(Vec *step, double *fobj, double *cons) override;
  int evalObjConGradient(Vec *step, Vec *g, Vec **Ac) override;
  bool reductionsBatchable() override { return sub->reductionsBatchable(); }
  const std::vector<char> *constantJacobianMask() override {
    return constraint == SUBPROBLEM_CONSTRAINT ? sub->constantJacobianMask() : nullptr;
  }
  std::vector<double> eo_cs, eo_cl;  // landing areas (see TrustRegionSubproblem::eo_dots)
  double eo_fs = 0.0, eo_fl = 0.0;
  int evalSparseCon(Vec *step, Vec *out) override { return sub->evalSparseCon(step, out); }
  int addSparseJacobian(double a, Vec *x, Vec *px, Vec *out) override {
    return sub->addSparseJacobian(a, x, px, out);
  }
  int addSparseJacobianTranspose(double a, Vec *x, Vec *pzw, Vec *out) override {
    return sub->addSparseJacobianTranspose(a, x, pzw, out);
  }
  int setSparseJacobianTranspose(double a, Vec *x, Vec *pzw, Vec *out) override {
    return sub->setSparseJacobianTranspose(a, x, pzw, out);
  }
  int addSparseInnerProduct(double a, Vec *x, Vec *cvec, Vec *A) override {
    return sub->addSparseInnerProduct(a, x, cvec, A);
  }
  bool sparseGramGroups(Vec *x, GramGroups *g) override { return sub->sparseGramGroups(x, g); }
  bool sparseTransposeColumn(double alpha, Vec *x, Vec *pzw, GroupCol *col) override {
    return sub->sparseTransposeColumn(alpha, x, pzw, col);
  }
  int setSparseJacobian(double a, Vec *x, Vec *px, Vec *out) override { return sub->setSparseJacobian(a, x, px, out); }
  Problem *sparseOwner(Vec **x) override { return sub->sparseOwner(x); }
  TrustRegionSubproblem *sub;
  int objective, constraint;
  double obj_scale;
};

typedef int (*TrIterationFn)(void *user, int iter);

class TrustRegion {
 public:
  // everything assembled from the options, as ParOptOptimizer does for algorithm = "tr"
  explicit TrustRegion(Problem *prob);
  // ParOptTrustRegion(subproblem, options) (src/ParOptTrustRegion.cpp:660-718): the caller owns the subproblem
  // (and, through it, the quasi-Newton object); the interior-point solver arrives with optimize(ip)
  explicit TrustRegion(TrustRegionSubproblem *subproblem);
  ~TrustRegion();
  Options &options() { return ip ? ip->options : opts; }
  // compact eigenvalue model for constraint `index` with N curvature directions (before optimize)
  int setEigenModel(int N, int index, EigenModelUpdate update, void *user);
  // ext != nullptr: ParOptTrustRegion::optimize(ParOptInteriorPoint*) (.cpp:2365-2384) -- the caller's solver, built
  // on the subproblem, is used (borrowed); the trust-region options set on this object are carried into its registry
  int optimize(InteriorPoint *ext = nullptr);
  int build();  // quasi-Newton, subproblem, interior point from the current options (idempotent)
  int initialize();  // ParOptTrustRegion::initialize (.cpp:1086-1099)
  void setPenaltyGamma(double gamma);           // .cpp:1049-1055
  void setPenaltyGammaArray(const double *g);   // .cpp:1062-1068

  Problem *prob;
  Ctx *ctx;
  Options opts;  // registry until the interior-point object exists, then ip->options is the one
  CompactQuasiNewton *qn = nullptr;
  CompactEigenApprox *eigh = nullptr;
  EigenQuasiNewton *eqn = nullptr;
  TrustRegionSubproblem *sub;
  InfeasSubproblem *infeas = nullptr;
  InteriorPoint *ip = nullptr;
  po_qn_s qn_handle;

  int m, nineq;
  std::vector<double> penalty_gamma;
  double tr_size = 0.1;
  int iter_count = 0, subproblem_iters = 0, adaptive_subproblem_iters = 0;
  std::string history;
  TrIterationFn iter_cb = nullptr;
  void *iter_cb_user = nullptr;
  // last iteration's table row (for observers): fobj, infeas, l1, linfty, smax, tr, rho, model_reduc,
  // zav, zmax, gav, gmax
  double row[12] = {};
  std::string row_info;
  // last line of the interior point's iteration table in the two subproblem solves of the latest iteration
  // ([0] steering / restoration solve, [1] the QP): how each solve ended (po_tr_get_last_solve_lines)
  std::string last_solve_line[2];
  void captureSolveLine(int which);

 private:
  TrustRegion(Problem *prob, TrustRegionSubproblem *subproblem);  // (subproblem == nullptr: built from the options)
  bool own_sub, own_ip = true, state_ready = false;
  int initState();  // penalty parameters and radius from the options (the reference's constructor)
  // the tail of build() and of optimize(ext): scratch, the interior-point solver (a new one on the subproblem, or
  // the caller's `ext`), the quasi-Newton handle, the state
  int attachSolver(InteriorPoint *ext);
  int eig_N = 0, eig_index = 0;
  EigenModelUpdate eig_update = nullptr;
  void *eig_user = nullptr;
  Vec *tvec = nullptr;
  // violation of dense constraint i at the values c: max(0, -c_i) for an inequality, |c_i| for an equality
  double violation(const double *c, int i) const { return i < nineq ? std::max(0.0, -c[i]) : fabs(c[i]); }
  double infeasOf(const double *c, const double *weights) const;
  // One interior-point solve of the problem instance and options its caller has set: optimize, the last table line
  // into last_solve_line[which], and where the solver left the step and the multipliers (its own storage).
  // rc != PO_OK: the solve failed (not: stopped at its iteration limit) and nothing else is set.
  struct Solution {
    int rc;
    Vec *step;
    const double *z;
    Vec *zw;
  };
  Solution solveSubproblem(int which);
  // the tail of an iteration: multiplier and penalty statistics behind the caller's first eight columns, the
  // quasi-Newton update token in front of the caller's info, the table row, the iteration count
  void finishRow(const double head[8], const double *z, const std::string &info_tail, double t0);
  int computeKKTError(const double *z, Vec *zw, double *l1, double *linfty);
  int minimizeInfeas(std::vector<double> *best_con_infeas);
  int sl1qpOptimize();
  int filterOptimize();
  // filter set :896-966
  struct FilterElement {
    double f, h;
  };
  std::vector<FilterElement> filter;
  int acceptableByPair(double f_new, double h_new, double f_old, double h_old);
  int acceptableByFilter(double f, double h);
  void addToFilter(double f, double h);
  void appendRow(const double vals[12], const std::string &info, double seconds);
  int sl1qpUpdate(Vec *step, const double *z, Vec *zw, double *infeas, double *l1, double *linfty);
};

}  // namespace po

struct po_tr_s {
  po::TrustRegion *tr;
  void *eig_holder;  // capi_tr.cpp: storage behind the eigenvalue-model callbacks, owned by the handle
};
struct po_eig_s {
  po::CompactEigenApprox *e;
};
