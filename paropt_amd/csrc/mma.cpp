// Method of moving asymptotes on the device (see mma.hpp); control flow of ParOptMMA::optimize /
// initializeSubProblem / computeKKTError (reference src/ParOptMMA.cpp:318-757), quirks included.
#include "mma.hpp"

#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "mma_dual.hpp"
#include "mma_gcmma.hpp"
#include "tr.hpp"

namespace po {

MMA::MMA(Problem *p)
    : Problem(p), cons(p->ncon, 0.0), b(p->ncon, 0.0), z(p->ncon, 0.0), prob(p), m(p->ncon) {
  opts.addMMADefaults();
  opts.set("output_file", "");
  gcmma.rho.assign(m + 1, 0.0);
  trial.cons.assign(m, 0.0);
}

MMA::~MMA() {
  delete ip;
  Vec *all[] = {xvec, x1vec, x2vec, lbvec, ubvec, gvec, Lvec, Uvec, alphavec, betavec, p0vec,
                q0vec, rvec, zlvec, zuvec, uinv, linv, cwvec, zwvec};
  for (Vec *v : all) vec_decref(v);
  for (Vec *v : Avecs) vec_decref(v);
  for (Vec *v : pivecs) vec_decref(v);
  for (Vec *v : qivecs) vec_decref(v);
  for (Vec *v : Gvecs) vec_decref(v);
  for (Vec *v : Uwvecs) vec_decref(v);
  vec_decref(cgvec);
  vec_decref(swvec);
}

int MMA::allocate() {  // initialize() :131-232
  const int64_t n = nlocal;
  Vec **all[] = {&xvec, &x1vec, &x2vec, &lbvec, &ubvec, &gvec, &Lvec, &Uvec, &alphavec, &betavec,
                 &p0vec, &q0vec, &rvec, &zlvec, &zuvec, &uinv, &linv};
  for (Vec **v : all) {
    *v = vec_new(ctx, n);
    if (!*v) return PO_ERR_HIP;
  }
  for (int i = 0; i < m; i++) {
    Vec *a = vec_new(ctx, n);
    if (!a) return PO_ERR_HIP;
    Avecs.push_back(a);
    if (use_linear) continue;  // (the linear form never reads p_i, q_i)
    Vec *pv = vec_new(ctx, n), *qv = vec_new(ctx, n);
    if (!pv || !qv) return PO_ERR_HIP;
    pivecs.push_back(pv);
    qivecs.push_back(qv);
  }
  if (nwcon > 0) {
    cwvec = vec_new(ctx, nwcon);
    zwvec = vec_new(ctx, nwcon);
    if (!cwvec || !zwvec) return PO_ERR_HIP;
  }
  PO_TRY(k_fill(ctx, alphavec->d, n, 0.0));
  PO_TRY(k_fill(ctx, betavec->d, n, 1.0));
  if (prob->getVarsAndBounds(xvec, lbvec, ubvec) != 0) return PO_ERR_USER;
  if (!prob->useUpperBounds()) PO_TRY(k_fill(ctx, ubvec->d, n, 10.0));
  if (!prob->useLowerBounds()) PO_TRY(k_fill(ctx, lbvec->d, n, -9.0));
  // the tables of the subproblem: none of these vectors is replaced before the destructor
  P0p.push_back(p0vec->d);
  Q0q.push_back(q0vec->d);
  for (int i = 0; i < m; i++) {
    if (!use_linear) {
      P0p.push_back(pivecs[i]->d);
      Q0q.push_back(qivecs[i]->d);
    }
    A.push_back(Avecs[i]->d);
  }
  A.push_back(zlvec->d);  // (the two columns computeKKTError adds to the constraint gradients)
  A.push_back(zuvec->d);
  sub = mma_dual_data(Lvec->d, Uvec->d, alphavec->d, betavec->d, p0vec->d, q0vec->d, P0p.data() + 1, Q0q.data() + 1,
                      b.data(), m, n);
  return PO_OK;
}

// what the options ask for: every option string is compared here
bool MMA::optionIs(const char *name, const char *value) { return std::string(options().str(name)) == value; }
bool MMA::wantDual() { return optionIs("mma_subproblem_solver", "dual"); }
bool MMA::wantGroups() { return optionIs("mma_dual_sparse_constraints", "groups"); }
bool MMA::wantGcmmaGroups() { return optionIs("mma_gcmma_sparse_constraints", "groups"); }
bool MMA::conservative() { return optionIs("mma_globalization", "conservative"); }
bool MMA::linearised() { return options().integer("mma_use_constraint_linearization") != 0; }
bool MMA::wantLinear() { return linearised() && optionIs("mma_dual_linearized_constraints", "newton"); }

int MMA::build() {
  if (ip || xvec) return PO_OK;
  if (m + 1 > kMaxPanel) {
    set_error("MMA: %d constraints exceed the panel width %d", m, kMaxPanel - 1);
    return PO_ERR_ARG;
  }
  use_dual = wantDual();
  use_groups = use_dual && wantGroups() && nwcon > 0;
  use_linear = use_dual && wantLinear();
  PO_TRY(allocate());
  if (use_linear) return PO_OK;  // 17 + c vectors: the panel form's columns are the A_i themselves
  if (use_dual) {  // no interior point and none of its 15 + c vectors; uinv / linv serve as the new point / the weights
    if (use_groups) {  // 2 + c vectors of nwcon on top of the panel form's c columns
      cgvec = vec_new(ctx, nwcon);
      swvec = vec_new(ctx, nwcon);
      if (!cgvec || !swvec) return PO_ERR_HIP;
      for (int i = 0; i < m; i++) {
        Vec *u = vec_new(ctx, nwcon);
        if (!u) return PO_ERR_HIP;
        Uwvecs.push_back(u);
        Uw.push_back(u->d);
      }
    }
    if (m > kMmaDualFused || use_groups) {
      for (int i = 0; i < m; i++) {
        Vec *g = vec_new(ctx, nlocal);
        if (!g) return PO_ERR_HIP;
        Gvecs.push_back(g);
        G.push_back(g->d);
      }
    }
    return PO_OK;
  }
  ip = new InteriorPoint(this);
  ip->options = opts;
  PO_TRY(ip->allocate());
  return PO_OK;
}

// ---- the dual sub-solver --------------------------------------------------------------------------
int MMA::checkDualCovers() {
  const char *why = nullptr;
  const GroupMap *gm = prob->groupedLibraryForm();
  if (nwcon > 0 && !wantGroups()) {
    why = "sparse constraints are not part of the closed-form primal point";
  } else if (nwcon > 0 && conservative() && !wantGcmmaGroups()) {
    why = "sparse constraints in groups run under mma_globalization = conservative only with "
          "mma_gcmma_sparse_constraints = groups";
  } else if (nwcon > 0 && (!gm || gm->nwcon != nwcon || !mma_dual_groups_tile(*gm, nlocal))) {
    why = "sparse constraints run through the dual only in the grouped form: one constraint per group of nw "
          "consecutive variables with one Jacobian value (setWeighting, or a CSR pattern recognised as such), "
          "nwblock = 1, nw + skip within the 512 variables of a tile, and no quasi-definite solver of the problem's own";
  }
  if (wantLinear() && nwcon > 0 && wantGroups()) {
    why = "the dual of the linearised subproblem (mma_dual_linearized_constraints = newton) takes no sparse "
          "constraints, grouped ones included";
  } else if (why) {
  } else if (wantLinear()) {  // P = p0, Q = q0 whatever the multipliers: equalities included
    if (conservative())
      why = "mma_globalization = conservative does not run on linearised constraints: a linearisation is not "
            "conservative and would need a rho of its own";
  } else if (ninequality < m) {
    why = "a dense equality constraint has a free multiplier, which can make P or Q negative";
  } else if (linearised()) {
    why = "linearised constraints have no rational dual";
  }
  if (!why) return PO_OK;
  set_error("MMA: mma_subproblem_solver = dual does not cover this problem: %s", why);
  return PO_ERR_ARG;
}

// the multipliers and the counters a finished dual solve leaves behind
void MMA::finishDualSolve(const MmaDualResult &res, const std::vector<double> &lambda) {
  z = lambda;
  subproblem_iter += res.evaluations;
  dual.solves++;
  dual.iterations += res.iterations;
  dual.evaluations += res.evaluations;
  dual.last_status = res.status;
  dual.last_pg = res.pg;
}

// rho != nullptr: the subproblem in the conservative approximations f~_i + rho_i d around xvec; point_sums[m + 2] then
// receives {Delta_0..m, D} of the solution (mma_gcmma.hpp).  Grouped sparse constraints are affine in the grouped form,
// so their approximation is exact: they carry no rho and take no part in the acceptance test
int MMA::solveDual(const double *rho, double *point_sums) {
  Options &o = options();
  const int form = dualForm();
  std::vector<double> gamma(m, o.real("penalty_gamma")), lambda(z);
  MmaDualResult res;
  const MmaDualRho r{xvec->d, rho};
  MmaGroupStats over;  // (max_inner, cap_hits, max_psi over the evaluations of this solve)
  auto eval = [&](const double *lam, bool want_h, double *W, double *g, double *H) -> int {
    if (use_groups) {
      MmaGroupStats st;
      PO_TRY(k_mma_dual_groups(ctx, sub, grp, lam, W, g, want_h ? H : nullptr, G.data(), linv->d, uinv->d, zwvec->d,
                               Uw.data(), swvec->d, nullptr, nullptr, &st, rho ? &r : nullptr));
      over.absorb(st);
      return PO_OK;
    }
    return k_mma_dual(ctx, sub, lam, want_h ? form : 0, W, g, H, G.empty() ? nullptr : G.data(), linv->d,
                      rho ? &r : nullptr);
  };
  PO_TRY(mma_dual_solve(m, gamma.data(), o.real("mma_dual_tol"), o.integer("mma_dual_max_iterations"), eval,
                        lambda.data(), &res));
  if (use_groups) {
    PO_TRY(k_mma_group_solve(ctx, sub, grp, lambda.data(), uinv->d, zwvec->d, zlvec->d, zuvec->d, &groups,
                             rho ? &r : nullptr));
    if (rho) PO_TRY(k_mma_gcmma_group_sums(ctx, sub, xvec->d, uinv->d, point_sums));
    groups.absorb(over);
  } else if (rho) PO_TRY(k_mma_gcmma_point(ctx, sub, r, lambda.data(), uinv->d, zlvec->d, zuvec->d, point_sums));
  else PO_TRY(k_mma_dual_point(ctx, sub, lambda.data(), uinv->d, zlvec->d, zuvec->d));
  finishDualSolve(res, lambda);
  return PO_OK;
}

// The subproblem with linearised constraints (mma.hpp): inequalities in [0, gamma], equalities in [-gamma, gamma].  The
// root searches of the first evaluation start from xvec, those of every later pass from the point the pass before it
// left in uinv.
int MMA::solveDualLinear() {
  Options &o = options();
  const int form = dualForm();
  const double gamma = o.real("penalty_gamma");
  std::vector<double> lower(m, 0.0), upper(m, gamma), lambda(z);
  for (int i = ninequality; i < m; i++) lower[i] = -gamma;
  const MmaDualLinear lin{Lvec->d, Uvec->d, alphavec->d, betavec->d, p0vec->d, q0vec->d, xvec->d, A.data(),
                          cons.data(), m, nlocal};
  MmaDualResult res;
  const double *start = xvec->d;
  auto eval = [&](const double *lam, bool want_h, double *W, double *g, double *H) -> int {
    PO_TRY(k_mma_dual_linear(ctx, lin, lam, want_h ? form : 0, start, uinv->d, W, g, H, linv->d, &linear));
    start = uinv->d;
    return PO_OK;
  };
  PO_TRY(mma_dual_solve(m, lower.data(), upper.data(), o.real("mma_dual_tol"), o.integer("mma_dual_max_iterations"),
                        eval, lambda.data(), &res));
  PO_TRY(k_mma_dual_linear_point(ctx, lin, lambda.data(), start, uinv->d, zlvec->d, zuvec->d, &linear));
  finishDualSolve(res, lambda);
  return PO_OK;
}

// One MMA iteration of the conservative variant: rho from the gradients at xvec, then subproblem solves (each
// warm-started from the last multipliers) until the problem's own values at the new point lie under the
// approximations.  No gradient is evaluated and no coefficient vector is rewritten in here.
int MMA::solveConservative() {
  Options &o = options();
  GcmmaParams gp;
  gp.rho_init = o.real("mma_gcmma_rho_init");
  gp.rho_min = o.real("mma_gcmma_rho_min");
  gp.tol = o.real("mma_gcmma_tol");
  gp.max_inner = o.integer("mma_gcmma_max_inner");
  std::vector<double> sums(m + 1), fk(m + 1);
  PO_TRY(k_mma_gcmma_rho_sums(ctx, Lvec->d, Uvec->d, gvec->d, A.data(), m, nlocal, sums.data()));
  gcmma_rho_start(m, sums.data(), nglobal, gp, gcmma.rho.data());
  fk[0] = fobj;
  for (int i = 0; i < m; i++) fk[1 + i] = -cons[i];
  auto try_rho = [&](const double *rho, double *psums, double *fnew) -> int {
    PO_TRY(solveDual(rho, psums));
    if (prob->evalObjCon(uinv, &trial.fobj, trial.cons.data()) != 0) {
      fprintf(stderr, "ParOptMMA: Objective evaluation failed\n");
      return PO_ERR_USER;
    }
    fnew[0] = trial.fobj;
    for (int i = 0; i < m; i++) fnew[1 + i] = -trial.cons[i];
    return PO_OK;
  };
  int raises = 0;
  bool capped = false;
  PO_TRY(gcmma_inner(m, fk.data(), gp, try_rho, gcmma.rho.data(), &raises, &capped));
  trial.have = true;  // (the next initializeSubProblem takes uinv: no second evaluation there)
  gcmma.inner_total += raises;
  gcmma.inner_last = raises;
  gcmma.inner_max = std::max(gcmma.inner_max, raises);
  if (capped) gcmma.cap_hits++;
  return PO_OK;
}

MmaParams MMA::params() {
  Options &o = options();
  MmaParams p;
  p.movlim = o.real("mma_move_limit");
  p.init_off = o.real("mma_init_asymptote_offset");
  p.contract = o.real("mma_asymptote_contract");
  p.relax = o.real("mma_asymptote_relax");
  p.min_off = o.real("mma_min_asymptote_offset");
  p.max_off = o.real("mma_max_asymptote_offset");
  p.eps = o.real("mma_eps_regularization");
  p.delta = o.real("mma_delta_regularization");
  return p;
}

int MMA::computeKKTError(double *l1, double *linfty, double *infeas) {  // :406-484
  const double relax = options().real("mma_bound_relax");
  const int64_t n = nlocal;
  std::vector<double> cf;  // over [A_i | zl | zu]
  for (int i = 0; i < m; i++) cf.push_back(-z[i]);
  if (relax <= 0.0) {
    cf.push_back(-1.0);
    cf.push_back(1.0);
  }
  PO_TRY(k_panel_axpy(ctx, rvec->d, 1.0, gvec->d, 0.0, cf.data(), A.data(), (int)cf.size(), n));
  if (nwcon > 0) {
    if (prob->addSparseJacobianTranspose(-1.0, xvec, zwvec, rvec) != 0) return PO_ERR_USER;
  }
  if (relax <= 0.0) {
    PO_TRY(k_reduce1(ctx, RED_ASUM, rvec->d, nullptr, n, l1));
    PO_TRY(k_reduce1(ctx, RED_AMAX, rvec->d, nullptr, n, linfty));
  } else {
    double out[2];
    PO_TRY(k_kkt_error(ctx, xvec->d, lbvec->d, ubvec->d, rvec->d, relax, n, out));
    *l1 = out[0];
    *linfty = out[1];
  }
  *infeas = 0.0;
  for (int i = 0; i < m; i++) *infeas += fabs(std::min(0.0, cons[i]));
  return PO_OK;
}

int MMA::initializeSubProblem(Vec *xv) {  // :523-757
  const int64_t n = nlocal;
  PO_TRY(k_copy(ctx, x2vec->d, x1vec->d, n));
  PO_TRY(k_copy(ctx, x1vec->d, xvec->d, n));
  if (xv && xv != xvec) PO_TRY(k_copy(ctx, xvec->d, xv->d, n));
  if (trial.have) {  // the inner iteration evaluated the problem at this point last
    fobj = trial.fobj;
    cons = trial.cons;
    trial.have = false;
  } else if (prob->evalObjCon(xvec, &fobj, cons.data()) != 0) {
    fprintf(stderr, "ParOptMMA: Objective evaluation failed\n");
    return PO_ERR_USER;
  }
  if (prob->evalObjConGradient(xvec, gvec, Avecs.data()) != 0) {
    fprintf(stderr, "ParOptMMA: Gradient evaluation failed\n");
    return PO_ERR_USER;
  }
  if (nwcon > 0 && prob->evalSparseCon(xvec, cwvec) != 0) return PO_ERR_USER;
  if (use_groups) {  // psi_i(x) = a sum_{G_i} x + c_i, c_i = cw_i(x^k) - a sum_{G_i} x^k
    const GroupMap *gm = prob->groupedLibraryForm();
    if (!gm || gm->nwcon != nwcon) {
      set_error("MMA: mma_dual_sparse_constraints = groups: the sparse constraints lost their grouped form (the "
                "entries of the Jacobian are no longer all equal)");
      return PO_ERR_ARG;
    }
    grp.map = *gm;
    grp.a = prob->group_alpha;
    grp.c = cgvec->d;
    grp.nwinequality = nwinequality;
    grp.gamma = options().real("penalty_gamma");
    PO_TRY(k_copy(ctx, cgvec->d, cwvec->d, nwcon));
    PO_TRY(k_group_sum(ctx, grp.map, cgvec->d, 1, 0.0, -grp.a, xvec->d));
  }
  {  // the table row :571-596
    double l1 = 0.0, linfty = 0.0, infeas = 0.0, l1_lambda = 0.0;
    PO_TRY(computeKKTError(&l1, &linfty, &infeas));
    for (int i = 0; i < m; i++) l1_lambda += fabs(z[i]);
    const double vals[5] = {fobj, l1, linfty, l1_lambda, infeas};
    for (int i = 0; i < 5; i++) last_row[i] = vals[i];
    if (ctx->rank == 0) {
      char line[256];
      if (mma_iter % 10 == 0) {
        snprintf(line, sizeof(line), "\n%5s %8s %15s %9s %9s %9s %9s\n", "MMA", "sub-iter", "fobj", "l1-opt",
                 "linft-opt", "l1-lambd", "infeas");
        history += line;
      }
      snprintf(line, sizeof(line), "%5d %8d %15.6e %9.3e %9.3e %9.3e %9.3e\n", mma_iter, subproblem_iter, fobj,
               l1, linfty, l1_lambda, infeas);
      history += line;
    }
    if (iter_cb) iter_cb(iter_cb_user, mma_iter);
  }
  const MmaParams p = params();
  PO_TRY(k_mma_asymptotes(ctx, xvec->d, x1vec->d, x2vec->d, lbvec->d, ubvec->d, p, mma_iter < 2 ? 1 : 0, n,
                          Lvec->d, Uvec->d));
  PO_TRY(k_mma_coef(ctx, xvec->d, lbvec->d, ubvec->d, Lvec->d, Uvec->d, gvec->d, p, n, alphavec->d,
                    betavec->d, p0vec->d, q0vec->d));
  if (use_true_mma) {
    for (int i = 0; i < m; i++) {
      double bs = 0.0;
      PO_TRY(k_mma_pq(ctx, xvec->d, Lvec->d, Uvec->d, Avecs[i]->d, n, pivecs[i]->d, qivecs[i]->d, &bs));
      b[i] = -(cons[i] + bs);
    }
  }
  mma_iter++;
  if (ip) PO_TRY(ip->resetDesignAndBounds());  // the interior point restarts from xvec inside the new move limits
  return PO_OK;
}

void MMA::setMultipliers() {  // :384-400
  Vec *x = nullptr, *zl = nullptr, *zu = nullptr;
  const double *zz = nullptr;
  ip->getOptimizedPoint(&x, &zz, &zl, &zu);
  for (int i = 0; i < m; i++) z[i] = zz[i];
  Vec *wv[5];
  ip->getOptimizedSparse(wv);
  if (wv[0] && zwvec) k_copy(ctx, zwvec->d, wv[0]->d, nwcon);
  if (zl) k_copy(ctx, zlvec->d, zl->d, nlocal);
  if (zu) k_copy(ctx, zuvec->d, zu->d, nlocal);
}

// The new point stays where the sub-solver left it: *xnew is the interior point's own vector or uinv.
int MMA::solveSubproblem(Vec **xnew) {
  switch (mode) {
    case Mode::INTERIOR_POINT: {
      const int rc = ip->optimize(nullptr);
      if (rc != 0 && rc != 1) return rc;
      setMultipliers();
      ip->getOptimizedPoint(xnew, nullptr, nullptr, nullptr);
      return PO_OK;
    }
    case Mode::DUAL: PO_TRY(use_linear ? solveDualLinear() : solveDual()); break;
    case Mode::DUAL_CONSERVATIVE: PO_TRY(solveConservative()); break;
  }
  *xnew = uinv;
  return PO_OK;
}

int MMA::optimize() {  // :318-379
  const bool want_dual = wantDual();
  if (conservative() && !want_dual) {  // (an inner raise would rewrite the interior point's 2 m + 2 coefficient vectors)
    set_error("MMA: mma_globalization = conservative requires mma_subproblem_solver = dual");
    return PO_ERR_ARG;
  }
  if (want_dual) PO_TRY(checkDualCovers());  // refused before anything is allocated or run
  PO_TRY(build());
  if (want_dual != use_dual || (use_dual && nwcon > 0 && wantGroups() != use_groups) ||
      (use_dual && wantLinear() != use_linear)) {
    set_error("MMA: mma_subproblem_solver cannot change once the solver's vectors exist");
    return PO_ERR_ARG;
  }
  mode = !use_dual ? Mode::INTERIOR_POINT : conservative() ? Mode::DUAL_CONSERVATIVE : Mode::DUAL;
  Options &o = options();
  const int max_it = o.integer("mma_max_iterations");
  const double infeas_tol = o.real("mma_infeas_tol"), l1_tol = o.real("mma_l1_tol"),
               linfty_tol = o.real("mma_linfty_tol");
  use_true_mma = linearised() ? 0 : 1;
  if (mode == Mode::INTERIOR_POINT) {  // the subproblem hands the interior point its diagonal Hessian (.cpp:344-346)
    PO_TRY(o.set("use_diag_hessian", 1));
    PO_TRY(o.set("use_line_search", 0));
  }
  history.clear();
  PO_TRY(initializeSubProblem(xvec));
  for (int i = 0; i < max_it; i++) {
    Vec *xnew = nullptr;
    PO_TRY(solveSubproblem(&xnew));
    PO_TRY(initializeSubProblem(xnew));
    // the reference calls computeKKTError(&infeas, &l1, &linfty) on a function declared as
    // (l1, linfty, infeas) (:364-366): the names below therefore hold permuted quantities
    double infeas = 0.0, l1 = 0.0, linfty = 0.0;
    PO_TRY(computeKKTError(&infeas, &l1, &linfty));
    if (infeas < infeas_tol && (l1 < l1_tol || linfty < linfty_tol)) break;
  }
  flushHistory();
  return 0;
}

void MMA::flushHistory() {
  write_history_file(ctx, options().str("mma_output_file"), "ParOptMMA", history);
}

// ---- the subproblem ---------------------------------------------------------------------------------
int MMA::getVarsAndBounds(Vec *x, Vec *lb, Vec *ub) {  // :795-799
  if (!xvec) {  // before build(): the interior point's constructor probe
    k_fill(ctx, x->d, nlocal, 0.5);
    k_fill(ctx, lb->d, nlocal, 0.0);
    k_fill(ctx, ub->d, nlocal, 1.0);
    return 0;
  }
  PO_TRY(k_copy(ctx, x->d, xvec->d, nlocal));
  PO_TRY(k_copy(ctx, lb->d, alphavec->d, nlocal));
  PO_TRY(k_copy(ctx, ub->d, betavec->d, nlocal));
  return 0;
}

int MMA::evalObjCon(Vec *xv, double *fval, double *cvals) {  // :804-866
  const int64_t n = nlocal;
  if (k_mma_inv(ctx, xv->d, Lvec->d, Uvec->d, n, uinv->d, linv->d) != PO_OK) return 1;
  const int nv = use_true_mma ? m + 1 : 1;
  std::vector<double> du(nv, 0.0), dl(nv, 0.0);
  if (k_mdot(ctx, uinv->d, P0p.data(), nv, n, du.data()) != PO_OK) return 1;
  if (k_mdot(ctx, linv->d, Q0q.data(), nv, n, dl.data()) != PO_OK) return 1;
  *fval = du[0] + dl[0];
  if (use_true_mma) {
    for (int i = 0; i < m; i++) cvals[i] = -((du[1 + i] + dl[1 + i]) + b[i]);
  } else if (m > 0) {
    // linearised constraints: cons + A (x - x0)
    const double mone[1] = {-1.0};
    const double *vv[1] = {xvec->d};
    if (k_panel_axpy(ctx, rvec->d, 1.0, xv->d, 0.0, mone, vv, 1, n) != PO_OK) return 1;
    if (k_mdot(ctx, rvec->d, A.data(), m, n, cvals) != PO_OK) return 1;
    for (int i = 0; i < m; i++) cvals[i] += cons[i];
  }
  return 0;
}

int MMA::evalObjConGradient(Vec *xv, Vec *gv, Vec **Ac) {  // :871-924
  subproblem_iter++;
  const int64_t n = nlocal;
  const int nv = use_true_mma ? m + 1 : 1;
  std::vector<double *> out(1, gv->d);  // [g | Ac_i]: the caller's vectors
  for (int i = 0; i < m; i++) out.push_back(Ac[i]->d);
  if (k_mma_grad(ctx, xv->d, Lvec->d, Uvec->d, P0p.data(), Q0q.data(), nv, n, out.data()) != PO_OK) return 1;
  if (!use_true_mma && m > 0) {
    if (k_panel_lincomb(ctx, out.data() + 1, 1.0, A.data(), 0.0, nullptr, m, n) != PO_OK) return 1;
  }
  return 0;
}

int MMA::evalHvecProduct(Vec *xv, const double *, Vec *, Vec *px, Vec *hvec) {  // :929-962 (objective only)
  const double one[1] = {1.0};
  if (k_mma_hdiag(ctx, xv->d, Lvec->d, Uvec->d, P0p.data(), Q0q.data(), one, 1, nlocal, hvec->d) != PO_OK) return 1;
  return k_mul(ctx, hvec->d, 1.0, hvec->d, px->d, nlocal) == PO_OK ? 0 : 1;
}

int MMA::evalHessianDiag(Vec *xv, const double *zz, Vec *, Vec *hdiag) {  // :967-1010
  const int nv = use_true_mma ? m + 1 : 1;
  std::vector<double> w(1, 1.0);
  for (int i = 1; i < nv; i++) w.push_back(zz[i - 1]);
  return k_mma_hdiag(ctx, xv->d, Lvec->d, Uvec->d, P0p.data(), Q0q.data(), w.data(), nv, nlocal, hdiag->d) == PO_OK ? 0
                                                                                                                   : 1;
}

int MMA::evalSparseCon(Vec *x, Vec *out) {  // :1015-1021
  if (nwcon <= 0) return 0;
  if (k_copy(ctx, out->d, cwvec->d, nwcon) != PO_OK) return 1;
  if (prob->addSparseJacobian(1.0, xvec, x, out) != 0) return 1;
  return prob->addSparseJacobian(-1.0, xvec, xvec, out);
}
int MMA::addSparseJacobian(double alpha, Vec *, Vec *px, Vec *out) {
  return nwcon > 0 ? prob->addSparseJacobian(alpha, xvec, px, out) : 0;
}
int MMA::addSparseJacobianTranspose(double alpha, Vec *, Vec *pzw, Vec *out) {
  return nwcon > 0 ? prob->addSparseJacobianTranspose(alpha, xvec, pzw, out) : 0;
}
int MMA::addSparseInnerProduct(double alpha, Vec *, Vec *cvec, Vec *A) {
  return nwcon > 0 ? prob->addSparseInnerProduct(alpha, xvec, cvec, A) : 0;
}

}  // namespace po
