// Interior-point iteration with every design-sized operation on the GPU (see ip.hpp).
//
// The control flow follows ParOptInteriorPoint::optimize (reference
// src/ParOptInteriorPoint.cpp:4399-5333) decision by decision; the linear algebra does NOT follow
// the reference's operation sequence but the fused form of DESIGN.md "Fused KKT step":
//   * ONE weighted Gram W = P^T diag(Dinv) P of the panel P = [Ac | Z] (MFMA) yields both Schur
//     complements G (:1932-1970) and Ce (:2634-2667) after O((c+k)^3) host work;
//   * every bordered solve K0^-1 b plus its Sherman-Morrison-Woodbury correction (:2700-2737) is
//     one panel-dot pass, tiny replicated host algebra, and one panel-axpy pass;
//   * iterative refinement (:4985-4991) folds the residual of the linearised system straight into
//     the right-hand side of the next solve;
//   * step scalings are applied lazily as scalars (no passes over the step vectors).
#include "ip.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

namespace po {

// ================================================================================================
// construction
// ================================================================================================
static const int LS_SUCCESS = 1, LS_FAILURE = 2, LS_MIN_STEP = 4, LS_MAX_ITERS = 8,
                 LS_NO_IMPROVEMENT = 16, LS_SHORT_STEP = 32;  // src/ParOptInteriorPoint.h:220-225
static_assert(LS_FAILURE == 2, "IterRecord::line_fail starts as LS_FAILURE (ip.hpp)");

InteriorPoint::InteriorPoint(Problem *p)
    : prob(p), ctx(p->ctx), n(p->nlocal), c(p->ncon), qn(nullptr), x(nullptr), zl(nullptr),
      zu(nullptr), lb(nullptr), ub(nullptr), g(nullptr), fobj(0.0), barrier_param(0.1),
      rho_penalty_search(0.0), niter(0), neval(0), ngeval(0),
      iter_cb(nullptr),
      iter_cb_user(nullptr), px(nullptr), pzl(nullptr), pzu(nullptr), Dinv(nullptr), rx(nullptr),
      tvec(nullptr), xt(nullptr), y_qn(nullptr), s_qn(nullptr), vA(nullptr), qn_created(false), qn_owned(true),
      comp_prod(0), comp_count(0), max_rx(0), max_rzl(0), max_rzu(0),
      corrector_active(false), norm_type(0), phase_t0(0) {
  qn_handle.qn = nullptr;
  hdiag = nullptr;
  inexact_newton_step = false;
  nhvec = 0;
  nw = p->nwcon;
  has_w = false;
  nw_global = 0.0;
  gsw = gtw = Cw = wd2 = wyw = wtmp = wtmp2 = d1v = nullptr;
  for (int i = 0; i < 5; i++) wvar[i] = wresv[i] = wstepv[i] = wscalev[i] = nullptr;
  for (int i = 0; i < 10; i++) w_merit_last[i] = 0.0;
  for (int i = 0; i < 7; i++) w_sums[i] = 0.0;
  for (int i = 0; i < 5; i++) w_maxs[i] = 0.0;
  use_lower = prob->useLowerBounds();
  use_upper = prob->useUpperBounds();
  kkt.c = c;
  vars.resize(c);
  res.resize(c);
  step.resize(c);
  refine.resize(c);
  cvals.assign(c, 0.0);
  step_mins[0] = step_mins[1] = 1.0;
  setPenaltyGamma(options.real("penalty_gamma"));
}

InteriorPoint::Forms InteriorPoint::readForms() {
  Forms f;
  f.analytic_panel_dots = !dbg_switch(SW_EXPLICIT_DOTS);
  f.fuse_merit = !dbg_switch(SW_NO_FUSED_MERIT);
  f.lean_step = !dbg_switch(SW_NO_LEAN_STEP);
  f.recompute_dt = !dbg_switch(SW_NO_RECOMPUTE_DT);
  f.recompute_first_step = !dbg_switch(SW_NO_RECOMPUTE);
  f.recompute_rhs = f.recompute_first_step && !dbg_switch(SW_NO_RECOMPUTE_RHS);
  f.fuse_mult_update = !dbg_switch(SW_NO_FUSED_UPDATE);
  return f;
}

int InteriorPoint::allocate() {
  Vec **all[] = {&x, &zl, &zu, &lb, &ub, &g, &px, &pzl, &pzu, &Dinv, &rx, &tvec, &xt, &y_qn, &s_qn, &vA};
  for (Vec **v : all) {
    *v = vec_new(ctx, n);
    if (!*v) return PO_ERR_HIP;
  }
  for (int j = 0; j < c; j++) {
    Vec *a = vec_new(ctx, n);
    if (!a) return PO_ERR_HIP;
    Ac.push_back(a);
  }
  // constructor state of the reference (:415-447): bounds checked once, multipliers = 1
  barrier_param = options.real("init_barrier_param");
  PO_TRY(initAndCheckDesignAndBounds());
  PO_TRY(k_fill(ctx, zl->d, n, 1.0));
  PO_TRY(k_fill(ctx, zu->d, n, 1.0));
  for (int i = 0; i < c; i++) vars.z[i] = vars.s[i] = vars.t[i] = vars.zs[i] = vars.zt[i] = 1.0;
  PO_TRY(allocateW());
  return PO_OK;
}

InteriorPoint::~InteriorPoint() {
  Vec *all[] = {x, zl, zu, lb, ub, g, px, pzl, pzu, Dinv, rx, tvec, xt, y_qn, s_qn, vA, acz};
  for (Vec *v : all) vec_decref(v);
  for (Vec *v : Ac) vec_decref(v);
  Vec *wall[] = {gsw, gtw, Cw, wd2, wyw, wtmp, wtmp2, d1v, cwx};
  for (Vec *v : wall) vec_decref(v);
  for (int i = 0; i < 5; i++) {
    vec_decref(wvar[i]);
    vec_decref(wresv[i]);
    vec_decref(wstepv[i]);
    vec_decref(wscalev[i]);
  }
  for (Vec *v : Uw) vec_decref(v);
  for (Vec *v : Yw) vec_decref(v);
  for (Vec *v : gmresW) vec_decref(v);
  vec_decref(hdiag);
  Vec *hall[] = {hvec_xp, hvec_csr_data, hvec_csr_cw};
  for (Vec *v : hall) vec_decref(v);
  for (int s = 0; s < 2; s++)
    for (Vec *v : hvec_work[s]) vec_decref(v);
  if (qn_owned) delete qn;
  if (user_events_ready)
    for (int i = 0; i < 2 * kUserRing; i++) (void)hipEventDestroy(user_ev[i]);
}

void InteriorPoint::setPenaltyGamma(double gamma) {  // :1127-1151
  if (gamma < 0.0) return;
  gamma_s.assign(c, gamma);
  gamma_t.assign(c, gamma);
  for (int i = 0; i < c && i < prob->ninequality; i++) gamma_s[i] = 0.0;
  if (has_w) k_w_gamma(ctx, gsw->d, gtw->d, gamma, prob->nwinequality, nw);  // :1139-1150
}

int InteriorPoint::setQuasiNewton(CompactQuasiNewton *qn_) {  // :1193-1234
  if (qn_owned) delete qn;
  qn = qn_;
  qn_owned = false;
  qn_created = true;
  qn_handle.qn = qn;
  return refreshQuasiNewton();  // a user-written approximation is validated at hand-over
}

int InteriorPoint::refreshQuasiNewton() {
  // (no width check on c + k: panels wider than one kernel's pointer table go through the launchers' slabs, for a
  // user-written approximation as for the built-in ones)
  return qn ? qn->refresh() : PO_OK;
}

int InteriorPoint::resetProblemInstance(Problem *p) {  // :745-764
  if (p->nlocal != prob->nlocal || p->ncon != prob->ncon || p->nwcon != prob->nwcon ||
      p->ninequality != prob->ninequality || p->nwinequality != prob->nwinequality) {
    set_error("ParOpt: Incompatible problem instance");
    return PO_ERR_ARG;
  }
  prob = p;
  stateReplaced();
  return PO_OK;
}

void InteriorPoint::setPenaltyGammaArray(const double *gamma) {  // :1160-1172 (dense blocks only)
  for (int i = 0; i < c; i++) {
    if (gamma[i] >= 0.0) {
      gamma_s[i] = i < prob->ninequality ? 0.0 : gamma[i];
      gamma_t[i] = gamma[i];
    }
  }
}

int InteriorPoint::createQuasiNewton() {  // ctor :262-292
  if (qn_created) return PO_OK;
  qn_created = true;
  qn = make_quasi_newton(ctx, n, options);
  qn_handle.qn = qn;
  return PO_OK;
}

Bounds InteriorPoint::bounds() const {
  Bounds b;
  b.x = x->d;
  b.lb = lb->d;
  b.ub = ub->d;
  b.zl = zl->d;
  b.zu = zu->d;
  b.max_bound = options.real("max_bound_value");
  b.use_lower = use_lower;
  b.use_upper = use_upper;
  if (dbg_switch(SW_UNIFORM_BOUNDS) != 0) {
    b.lb_uni = bounds_uni[0];
    b.ub_uni = bounds_uni[1];
    b.lb_c = bounds_val[0];
    b.ub_c = bounds_val[1];
  }
  return b;
}

std::vector<const double *> InteriorPoint::panel(bool use_qn, int *k) const {
  std::vector<const double *> p;
  for (Vec *a : Ac) p.push_back(a->d);
  *k = 0;
  if (qn && use_qn) {
    std::vector<const double *> z = qn->zPointers();
    *k = (int)z.size();
    p.insert(p.end(), z.begin(), z.end());
  }
  return p;
}

std::vector<const double *> &InteriorPoint::LazyPanel::get() {
  if (!asked) {
    int k = 0;
    P = ip->panel(use_qn, &k);
    asked = true;
  }
  return P;
}

int InteriorPoint::stepPanelDots(LazyPanel &P, std::vector<double> &dots) {
  const int mq = c + ((qn && P.use_qn) ? qn->size() : 0);
  dots.assign(mq > 0 ? mq : 1, 0.0);
  if (forms.analytic_panel_dots && step_flags.ptpx_valid && mq == c + kkt.k) {
    for (int i = 0; i < mq; i++) dots[i] = ptpx[i];
  } else if (mq > 0) {
    PO_TRY(k_mdot(ctx, px->d, P.get().data(), mq, n, dots.data()));
  }
  return PO_OK;
}

std::vector<double> InteriorPoint::compactInverse(const double *ztp, int kq) const {
  std::vector<double> rz(ztp, ztp + kq);
  qn->applyCompactInverse(rz.data());
  return rz;
}

int InteriorPoint::residualCoefs(ResTerm term, const double *z, const double *ztpx, int kq, std::vector<double> &coef,
                                 double *diag) {
  for (int i = 0; i < c; i++) coef[i] = z[i];
  *diag = options.real("qn_sigma");
  if (term == RES_QN) {
    *diag += qn->diag();
    std::vector<double> rz = compactInverse(ztpx, kq);
    for (int j = 0; j < kq; j++) coef[c + j] = rz[j];
  } else if (term != RES_SIGMA) {
    *diag = 0.0;
    if (term == RES_HVEC) {
      PO_TRY(hvecProduct(vars.z.data(), nullptr, px, xt));
    } else {
      PO_TRY(k_mul(ctx, xt->d, 1.0, hdiag->d, px->d, n));
    }
    coef[c + kq] = -1.0;
  }
  return PO_OK;
}

void InteriorPoint::phaseBegin() {
  phase_t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void InteriorPoint::phaseEnd(const char *name) {
  // every phase ends in a host-synchronising reduction or is followed by one, so host wall time
  // attributes the stream work to the phase that issued it (documented in DESIGN.md)
  const double t1 =
      std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  for (size_t i = 0; i < phase_names.size(); i++) {
    if (phase_names[i] == name) {
      phase_seconds[i] += t1 - phase_t0;
      phase_t0 = t1;
      return;
    }
  }
  phase_names.push_back(name);
  phase_seconds.push_back(t1 - phase_t0);
  phase_t0 = t1;
}

void InteriorPoint::userBegin() {
  ctx->in_user = 1;
  if (!user_timing) return;
  if (!user_events_ready) {
    for (int i = 0; i < 2 * kUserRing; i++)
      if (hipEventCreate(&user_ev[i]) != hipSuccess) return;
    user_events_ready = true;
  }
  if (user_pending == kUserRing) userHarvest();
  (void)hipEventRecord(user_ev[2 * user_pending], ctx->stream);
}
void InteriorPoint::userEnd() {
  ctx->in_user = 0;
  if (!user_timing || !user_events_ready) return;
  (void)hipEventRecord(user_ev[2 * user_pending + 1], ctx->stream);
  user_pending++;
}
void InteriorPoint::userHarvest() {
  for (int i = 0; i < user_pending; i++) {
    float ms = 0.0f;
    if (hipEventSynchronize(user_ev[2 * i + 1]) == hipSuccess &&
        hipEventElapsedTime(&ms, user_ev[2 * i], user_ev[2 * i + 1]) == hipSuccess)
      user_seconds += 1e-3 * ms;
  }
  user_pending = 0;
}

// ================================================================================================
// bounds / starting point
// ================================================================================================
int InteriorPoint::initAndCheckDesignAndBounds() {  // :4277-4361
  bounds_uni[0] = bounds_uni[1] = 0;
  int rc = prob->getVarsAndBounds(x, lb, ub);
  if (rc != 0) {
    set_error("getVarsAndBounds failed with code %d", rc);
    return PO_ERR_USER;
  }
  const double rel_bound = 0.001 * barrier_param;
  int flag = 0;
  PO_TRY(k_check_bounds(ctx, x->d, lb->d, ub->d, zl->d, zu->d, options.real("max_bound_value"),
                        rel_bound, use_lower && use_upper, n, &flag, bounds_uni, bounds_val));
  check_flag |= flag;
  if (ctx->rank == 0) {
    if (flag & 1) history += "ParOpt Warning: Variable bounds are inconsistent\n";
    if (flag & 2) history += "ParOpt Warning: Variables may be too close to lower bound\n";
    if (flag & 4) history += "ParOpt Warning: Variables may be too close to upper bound\n";
  }
  return PO_OK;
}

int InteriorPoint::clampCounts(double out[8]) {
  const double eps = options.real("design_precision");
  PO_TRY(k_clamp_count(ctx, x->d, lb->d, ub->d, use_lower ? zl->d : nullptr, use_upper ? zu->d : nullptr, eps, n,
                       out));
  for (int j = 4; j < 8; j++) out[j] = 0.0;
  for (int i = 0; i < c; i++) {
    if (vars.s[i] == eps) out[4] += 1.0;
    if (vars.t[i] == eps) out[5] += 1.0;
    if (vars.zs[i] == eps) out[6] += 1.0;
    if (vars.zt[i] == eps) out[7] += 1.0;
  }
  return PO_OK;
}

// A host mirror the caller still holds for one of the solver's vectors (getOptimizedPoint + getArray) is the vector's
// data while it is live: after an internal writer has changed the device copy the mirror is refreshed, so that the
// caller's pointer shows the new values (the reference has one buffer) and optimize()'s upload of live mirrors cannot
// put the old ones back (vec_mirror_refresh).
int InteriorPoint::resetDesignAndBounds() {  // :1249-1251
  stateReplaced();
  bounds_uni[0] = bounds_uni[1] = 0;  // (found again by the next optimize())
  int rc = prob->getVarsAndBounds(x, lb, ub);
  if (rc != 0) return PO_ERR_USER;
  PO_TRY(vec_mirror_refresh(x));
  PO_TRY(vec_mirror_refresh(lb));
  return vec_mirror_refresh(ub);
}

void InteriorPoint::resetQuasiNewtonHessian() {
  if (qn) qn->reset();
}

int InteriorPoint::initLeastSquaresMultipliers() {  // :5366-5534 (w = 0)
  iterate_flags.acz_valid = false;
  const double mu0 = options.real("init_barrier_param");
  PO_TRY(k_fill(ctx, zl->d, n, mu0));
  PO_TRY(k_fill(ctx, zu->d, n, mu0));
  for (int i = 0; i < c; i++) vars.z[i] = vars.s[i] = vars.t[i] = vars.zs[i] = vars.zt[i] = mu0;
  PO_TRY(k_zero_inactive(ctx, lb->d, ub->d, zl->d, zu->d, options.real("max_bound_value"), n));
  if (has_w) return initLeastSquaresMultipliersW();
  if (c == 0) return PO_OK;
  const double small = 1e-4;
  PO_TRY(k_fill(ctx, Dinv->d, n, 1.0));
  int k = 0;
  std::vector<const double *> A = panel(false, &k);
  std::vector<double> G((size_t)c * c, 0.0);
  PO_TRY(k_wgram(ctx, Dinv->d, A.data(), c, n, G.data()));
  for (int i = 0; i < c; i++) G[(size_t)i * (c + 1)] += small;
  std::vector<int> piv(c);
  lu_factor(c, G.data(), c, piv.data());
  // rhs = -(g - zl + zu); z = G^-1 ( -A rhs )
  const double al[2] = {1.0, -1.0};
  const double *vv[2] = {zl->d, zu->d};
  PO_TRY(k_panel_axpy(ctx, tvec->d, -1.0, g->d, 0.0, al, vv, 2, n));
  std::vector<double> z(c, 0.0);
  PO_TRY(k_mdot(ctx, tvec->d, A.data(), c, n, z.data()));
  for (int i = 0; i < c; i++) z[i] = -z[i];
  lu_solve(c, G.data(), c, piv.data(), z.data());
  for (int i = 0; i < c; i++) {
    const double gam = 10.0 * std::max(gamma_s[i], gamma_t[i]);
    vars.z[i] = (z[i] < -gam || z[i] > gam) ? 0.0 : z[i];
  }
  return PO_OK;
}

int InteriorPoint::initAffineStepMultipliers() {  // :5536-5656
  const double amin = options.real("start_affine_multiplier_min");
  PO_TRY(initLeastSquaresMultipliers());
  PO_TRY(k_zero_inactive(ctx, lb->d, ub->d, zl->d, zu->d, options.real("max_bound_value"), n));
  PO_TRY(computeResidual(0.0, true));
  bool use_qn = !(options.integer("sequential_linear_method") ||
                  !options.integer("use_qn_gmres_precon") || options.integer("use_diag_hessian"));
  if (options.integer("use_diag_hessian")) PO_TRY(ensureHdiag());
  PO_TRY(setUpKKTSystem(use_qn));
  denseResidual(0.0, res);
  if (has_w) {
    PO_TRY(solveKKTW(res, 0.0, use_qn, false, 1.0, step));
    PO_TRY(k_w_affine(ctx, wv(), wp(), amin, nw));  // :5601-5628
  } else {
    PO_TRY(solveKKT(res, 0.0, use_qn, false, 1.0, step));
  }
  iterate_flags.acz_valid = false;
  for (int i = 0; i < c; i++) {
    vars.z[i] = vars.z[i] + step.z[i];
    vars.s[i] = std::max(amin, fabs(vars.s[i] + step.s[i]));
    vars.t[i] = std::max(amin, fabs(vars.t[i] + step.t[i]));
    vars.zs[i] = std::max(amin, fabs(vars.zs[i] + step.zs[i]));
    vars.zt[i] = std::max(amin, fabs(vars.zt[i] + step.zt[i]));
  }
  PO_TRY(k_affine_mult(ctx, bounds(), zl->d, pzl->d, zu->d, pzu->d, amin, n));
  double comp = 0.0;
  PO_TRY(getComplementarity(&comp));
  barrier_param = comp;
  return PO_OK;
}

// ================================================================================================
// residuals and norms
// ================================================================================================
void InteriorPoint::denseResidual(double mu, Dense &r) const {  // :1403-1409
  for (int i = 0; i < c; i++) {
    r.z[i] = -(cvals[i] - vars.s[i] + vars.t[i]);
    r.s[i] = -(gamma_s[i] - vars.zs[i] + vars.z[i]);
    r.t[i] = -(gamma_t[i] - vars.zt[i] - vars.z[i]);
    r.zs[i] = -(vars.s[i] * vars.zs[i] - mu);
    r.zt[i] = -(vars.t[i] * vars.zt[i] - mu);
  }
}

// the barrier parameter the monotone strategy switches to from the current one (:4693-4707)
double InteriorPoint::nextMonotoneMu() const {
  const double abs_res_tol = options.real("abs_res_tol");
  const double mu_frac = options.real("monotone_barrier_fraction") * barrier_param;
  const double mu_pow = pow(barrier_param, options.real("monotone_barrier_power"));
  double new_mu = mu_frac;
  if (mu_pow < mu_frac) new_mu = mu_pow;
  if (new_mu < 0.1 * abs_res_tol) new_mu = 0.09999 * abs_res_tol;
  return new_mu;
}

// the fraction-to-boundary rule tau = max(min_frac, 1 - mu) (:4822-4826)
static double fractionToBoundary(double mu, double min_frac) {
  double tau = min_frac;
  if (1.0 - mu >= tau) tau = 1.0 - mu;
  return tau;
}

int InteriorPoint::computeResidual(double mu, bool vectors, Vec *yqn_complete, const MultUpdate *upd) {
  const double beta_mu = options.real("rel_bound_barrier") * mu;
  double *out = res_out.as_array();  // a member: inside a BatchScope the values arrive at the flush (after_reduce below)
  // speculative maxima for the next barrier parameter (see ip.hpp): only beside the norms of the CURRENT one
  const bool spec = vectors && spec_enabled && !has_w && mu == barrier_param;
  const double mu2 = spec ? nextMonotoneMu() : 0.0;
  const double beta_mu2 = spec ? options.real("rel_bound_barrier") * mu2 : -1.0;
  iterate_flags.spec_valid = false;
  scratch_flags.spec_dt_valid = false;  // (rx is about to change: a Dinv / t pair left by an earlier pass is stale)
  // sparse and design blocks of the residual share one collective + sync (the problem's sparse callbacks run in
  // between: built-in problems only)
  BatchScope wbatch(ctx, has_w && prob->reductionsBatchable());
  if (has_w) PO_TRY(computeResidualW(mu));
  bool acz_mode = false, acz_rebuilt = false;
  if (vectors) {
    std::vector<const double *> A;
    std::vector<double> zc;
    // A problem that declared its dense constraints linear (constant Jacobian): A^T z is kept in `acz` and
    // follows the multiplier steps (computeStepAndUpdate), so the residual does not stream the c constraint
    // gradients; it is rebuilt from the gradients every kAczRefresh uses to bound the round-off drift.
    if (prob->linear_constraints && iterate_flags.ac_valid && c > 0) {
      if (!acz) acz = vec_new(ctx, n);
      if (!acz) return PO_ERR_HIP;
      if (!iterate_flags.acz_valid || acz_age >= kAczRefresh) {
        std::vector<const double *> Ap;
        for (Vec *a : Ac) Ap.push_back(a->d);
        PO_TRY(k_panel_axpy(ctx, acz->d, 0.0, nullptr, 0.0, vars.z.data(), Ap.data(), c, n));
        iterate_flags.acz_valid = true;
        acz_age = 0;
        acz_rebuilt = true;
      }
      acz_age++;
      A.push_back(acz->d);
      zc.push_back(1.0);
      acz_mode = true;
    } else {
      for (Vec *a : Ac) A.push_back(a->d);
      zc = vars.z;
    }
    GroupCol gcol;  // + Aw^T zw as one more panel column (:1358-1361): described (structured problems) or stored
    const bool have_gcol = has_w && !acz_mode && prob->sparseTransposeColumn(1.0, x, wvar[0], &gcol);
    if (has_w && !have_gcol) {
      if (prob->setSparseJacobianTranspose(1.0, x, wvar[0], tvec) != 0) return PO_ERR_USER;
      A.push_back(tvec->d);
      zc.push_back(1.0);
    }
    const KktResArgs ra{.b = bounds(), .g = g->d, .A = A.data(), .z = zc.data(), .nc = (int)A.size(),
                        .beta_mu = beta_mu, .n = n, .rx = rx->d, .out = out,
                        .yqn = yqn_complete ? yqn_complete->d : nullptr, .beta_mu2 = beta_mu2,
                        .gcol = have_gcol ? &gcol : nullptr, .gcoef = 1.0};
    if (upd) {
      // the bound multipliers take their step in the same pass (see kkt_res_update_kernel); A^T z follows the dense
      // multiplier step by recurrence unless it has just been rebuilt from the new multipliers
      const double az_acz = (acz_mode && upd->acz_follow && !acz_rebuilt) ? upd->az : 0.0;
      // (lean step: px and the old point -- xt after the swap of computeStepAndUpdate -- instead of pzl / pzu)
      // No quasi-Newton update follows (a fixed approximation, the sequential linear method): the diagonal of the next
      // KKT system is known already, so this pass also leaves Dinv and t = Dinv o d1 of the next first solve behind
      // (spec_dt_*: setUpKKTSystem skips its pass over the bound data when diagonal and barrier parameter still match)
      const bool spec_dt = spec_dt_want && !has_w && !options.integer("use_diag_hessian") &&
                           dbg_switch(SW_SPEC_DT) != 0;
      const double sdiag = spec_dt ? options.real("qn_sigma") + ((qn && !options.integer("sequential_linear_method"))
                                                                    ? qn->diag() : 0.0) : 0.0;
      const double sbmu = spec_dt ? options.real("rel_bound_barrier") * spec_dt_mu : 0.0;
      KktResArgs ru = ra;
      if (acz_mode) ru.nc = 0;  // A^T z is read from acz
      ru.update = {.zl = zl->d, .pzl = pzl->d, .zu = zu->d, .pzu = pzu->d, .a = upd->a, .eps = upd->eps,
                   .va = (yqn_complete || az_acz != 0.0) ? vA->d : nullptr, .az = upd->az,
                   .acz = acz_mode ? acz->d : nullptr, .az_acz = az_acz,
                   .pxs = step_flags.pz_stored ? nullptr : px->d, .xold = step_flags.pz_stored ? nullptr : xt->d,
                   .beta_mu_step = step_beta_mu, .dinv_out = spec_dt ? Dinv->d : nullptr,
                   .t_out = spec_dt ? tvec->d : nullptr, .spec_diag = sdiag, .spec_beta_mu = sbmu};
      PO_TRY(k_kkt_res_update(ctx, ru));
      if (spec_dt) {
        scratch_flags.spec_dt_valid = true;
        spec_dt_diag = sdiag;
        spec_dt_bmu = sbmu;
      }
    } else {
      PO_TRY(k_kkt_res(ctx, ra));
    }
  } else {
    PO_TRY(k_res_norms(ctx, bounds(), beta_mu, n, out));
  }
  after_reduce(ctx, [this, vectors, spec, mu2] {
    const ResidualSums &o = res_out;
    if (vectors) {
      l1_rx = o.l1_rx;
      l2_rx = o.l2_rx;
      max_rx = o.max_rx;
    }
    if (spec) {
      spec_mu = mu2;
      spec_max[0] = o.spec_max_rzl;
      spec_max[1] = o.spec_max_rzu;
      iterate_flags.spec_valid = true;
    }
    comp_prod = o.comp_prod;
    comp_count = o.comp_count;
    l1_rzl = o.l1_rzl;
    l1_rzu = o.l1_rzu;
    l2_rzl = o.l2_rzl;
    l2_rzu = o.l2_rzu;
    max_rzl = o.max_rzl;
    max_rzu = o.max_rzu;
  });
  // (inside computeStepAndUpdate's batch the norms arrive with the quasi-Newton products: everything above that reads
  // them runs through after_reduce)
  return wbatch.end_nested();
}

void InteriorPoint::resNorms(const Dense &r, double *max_prime, double *max_dual,
                             double *max_infeas, double *res_norm) const {  // :1588-1723
  double mp = 0.0, md = 0.0, mi = 0.0;
  if (norm_type == 0) {  // infinity
    mp = max_rx;
    for (int i = 0; i < c; i++) {
      mp = std::max(mp, std::max(fabs(r.s[i]), fabs(r.t[i])));
      mi = std::max(mi, fabs(r.z[i]));
      md = std::max(md, std::max(fabs(r.zs[i]), fabs(r.zt[i])));
    }
    if (use_lower) md = std::max(md, max_rzl);
    if (use_upper) md = std::max(md, max_rzu);
    if (has_w) {  // :1599-1612
      mi = std::max(mi, w_maxs[0]);
      md = std::max(md, std::max(std::max(w_maxs[1], w_maxs[2]), std::max(w_maxs[3], w_maxs[4])));
    }
  } else if (norm_type == 1) {  // l1
    mp = l1_rx;
    for (int i = 0; i < c; i++) {
      mp += fabs(r.s[i]);
      mp += fabs(r.t[i]);
      mi += fabs(r.z[i]);
      md += fabs(r.zs[i]);
      md += fabs(r.zt[i]);
    }
    if (use_lower) md += l1_rzl;
    if (use_upper) md += l1_rzu;
    if (has_w) {
      mi += w_sums[1];
      md += w_sums[3] + w_sums[4] + w_sums[5] + w_sums[6];
    }
  } else {  // l2
    double prime = 0.0, infeas = 0.0, dual = 0.0;
    for (int i = 0; i < c; i++) {
      prime += r.s[i] * r.s[i] + r.t[i] * r.t[i];
      infeas += r.z[i] * r.z[i];
      dual += r.zs[i] * r.zs[i] + r.zt[i] * r.zt[i];
    }
    mp = l2_rx + prime;
    mi = infeas;
    md = dual;
    if (use_lower) md += l2_rzl;
    if (use_upper) md += l2_rzu;
    if (has_w) {  // the reference squares the l1 norms of the sparse dual blocks here (:1633-1638)
      mi += w_sums[2];
      md += w_sums[3] * w_sums[3] + w_sums[4] * w_sums[4] + w_sums[5] * w_sums[5] +
            w_sums[6] * w_sums[6];
    }
    mp = sqrt(mp);
    mi = sqrt(mi);
    md = sqrt(md);
  }
  *max_prime = mp;
  *max_dual = md;
  *max_infeas = mi;
  *res_norm = std::max(mp, std::max(md, mi));
}

double InteriorPoint::compFromSums(double prod, double count, const Dense &v,
                                   double wprod) const {  // :2742-2820
  prod = prod / options.real("rel_bound_barrier");
  if (has_w) {
    prod += wprod;
    count += 2.0 * nw_global;
  }
  for (int i = 0; i < c; i++) {
    prod += v.s[i] * v.zs[i] + v.t[i] * v.zt[i];
    count += 2.0;
  }
  return count != 0.0 ? prod / count : 0.0;
}

int InteriorPoint::getComplementarity(double *comp) {
  double out[11];
  PO_TRY(k_res_norms(ctx, bounds(), 0.0, n, out));
  double wprod = 0.0;
  if (has_w) PO_TRY(wCompStep(0.0, 0.0, &wprod));
  *comp = compFromSums(out[0], out[1], vars, wprod);
  return PO_OK;
}

// ================================================================================================
// the KKT system
// ================================================================================================
// Step 1 of setUpKKTSystem: Dinv for the diagonal `diag` (+ h_i with use_hdiag, :1840-1842) and, where the right-hand
// side of the solve that follows is known already (rx, the bounds and *rhs_mu), its vector out of the same pass over
// the bound data.  kz: quasi-Newton columns of the panel.  Sets t_is_plain_dinv_d1 (with t0_diag), consumes spec_dt_valid.
int InteriorPoint::formDinvAndRhs(double diag, bool use_hdiag, const double *rhs_mu, int kz, RhsFormed *formed) {
  const double *h = use_hdiag ? hdiag->d : nullptr;
  const double bmu = rhs_mu ? options.real("rel_bound_barrier") * (*rhs_mu) : 0.0;
  // dense constraints: t = Dinv o d1 rides through the Gram pass as one more, pre-weighted, column, so that P^T t -- the
  // mdot pass at the head of solveKKT -- comes out of the pass over P that the Schur complements need anyway
  const bool want_t = rhs_mu && !has_w && c + kz > 0;
  // sparse constraints: the block solve applies to the RAW right-hand side d1 (used when the fused first solve is taken)
  const bool want_raw_d1 = has_w && rhs_mu && !corrector_active;
  const bool have_spec_dt = scratch_flags.spec_dt_valid;
  scratch_flags.spec_dt_valid = false;  // consumed here, or overwritten below
  scratch_flags.t_is_plain_dinv_d1 = false;
  *formed = RHS_NONE;
  if (want_t) {
    // (the residual pass of this iterate may have left exactly this Dinv and t behind: kkt_res_update_kernel)
    const bool left_behind = have_spec_dt && !use_hdiag && spec_dt_diag == diag && spec_dt_bmu == bmu;
    if (!left_behind) PO_TRY(k_dinv_d1(ctx, bounds(), diag, h, rx->d, bmu, n, Dinv->d, tvec->d));
    scratch_flags.t_is_plain_dinv_d1 = !use_hdiag;
    t0_diag = diag;
    *formed = RHS_T;
  } else if (want_raw_d1) {
    PO_TRY(k_dinv_d1(ctx, bounds(), diag, h, rx->d, bmu, n, Dinv->d, d1v->d, 1));
    *formed = RHS_RAW_D1;
  } else {
    PO_TRY(k_dinv(ctx, bounds(), diag, n, Dinv->d, h));
  }
  return PO_OK;
}

// Step 2 of setUpKKTSystem: W = V^T Dinv V in one launch, unpacked into kkt.W (and t0dots) in the order [Ac | Z] once
// the reduction has arrived.
int InteriorPoint::gramPass(const GramPlan &plan, bool *groups_done) {
  const int m = (int)plan.V.size(), mt = m + (plan.with_t ? 1 : 0), k = plan.kform;
  const bool with_t = plan.with_t;
  std::vector<const double *> V(plan.V);
  if (with_t) V.push_back(tvec->d);
  Wt_buf.assign((size_t)mt * mt, 0.0);
  PO_TRY(k_wgram(ctx, Dinv->d, V.data(), mt, n, Wt_buf.data(), k > 0 ? plan.S.data() : nullptr,
                 k > 0 ? plan.Zout.data() : nullptr, k, plan.b0, with_t ? 1 : 0, plan.may_defer, plan.groups,
                 groups_done));
  t0dots.assign(with_t ? m : 0, 0.0);
  after_reduce(ctx, [this, m, mt, k, with_t] {
    // index in [Ac | Z] -> index in the launch order: [Z | Ac] when the pass formed Z, the same order otherwise
    auto at = [&](int i) { return k == 0 ? i : (i < c ? k + i : i - c); };
    for (int j = 0; j < m; j++)
      for (int i = 0; i < m; i++) kkt.W[i + (size_t)m * j] = Wt_buf[at(i) + (size_t)mt * at(j)];
    for (int i = 0; with_t && i < m; i++) t0dots[i] = Wt_buf[at(i) + (size_t)mt * m];
  });
  return PO_OK;
}

int InteriorPoint::setUpKKTSystem(bool use_qn, bool diag_only, const double *rhs_mu) {  // setUpKKTDiagSystem + setUpKKTSystem
  if (qn) PO_TRY(refreshQuasiNewton());
  step_flags.ptpx_valid = false;
  scratch_flags.t0_valid = false;
  const bool use_hdiag = options.integer("use_diag_hessian") && hdiag;  // h_i replaces b0 (:1840-1842)
  const double b0 = (!use_hdiag && qn && (use_qn || diag_only)) ? qn->diag() : 0.0;
  const bool with_z = use_qn && !diag_only;  // the low-rank part of the quasi-Newton approximation enters the panel
  // 1. Dinv and, where it is known already, the right-hand side of the first solve
  RhsFormed rhs = RHS_NONE;
  PO_TRY(formDinvAndRhs(b0 + options.real("qn_sigma"), use_hdiag, rhs_mu, (qn && with_z) ? qn->size() : 0, &rhs));
  const bool fuse_t = rhs == RHS_T, raw_d1_w = rhs == RHS_RAW_D1;
  // The panel.  L-SR1 leaves its columns Z_j = Y_j - b0 S_j unformed after an update; when this Gram pass is their
  // first consumer they are formed on the fly (and written out for the later passes): the launch takes [Z | Ac].
  // Otherwise panel() forms what is unformed and the launch takes [Ac | Z].
  GramPlan plan;
  std::vector<const double *> Yp, Sp;
  std::vector<double *> Zo;
  double b0z = 0.0;
  const bool fuse_z = qn && with_z && !has_w && qn->pendingZ(&Yp, &Sp, &Zo, &b0z) && !Yp.empty() && Yp.size() <= 12 &&
                      c + (int)Yp.size() + (fuse_t ? 1 : 0) <= kWgramMaxVecs;
  int k = 0;
  std::vector<const double *> P;  // [Ac | Z] with every column formed (left empty when the Gram pass forms Z)
  if (fuse_z) {
    plan.kform = k = (int)Yp.size();
    plan.V = Yp;
    for (Vec *a : Ac) plan.V.push_back(a->d);
    plan.S = Sp;
    plan.Zout = Zo;
    plan.b0 = b0z;
  } else {
    plan.V = P = panel(with_z, &k);  // (forms unformed columns: the Gram launch below reads them)
  }
  const int m = c + k;
  kkt.k = k;
  // Sparse constraints: the right-hand side of the first solve goes through the quasi-definite block solve,
  // t = [K0^-1 (d1, d2)]_x, which needs Cw -- so the factor comes first, then t (and the sparse multiplier part
  // wyw), then the Gram pass with t as its pre-weighted last column, as on the dense path.
  bool fuse_tw = false;
  // sparse constraints: the sparse residual norms of the new barrier parameter, the Gram pass and its sparse correction
  // share ONE collective + host sync (three before); the host algebra on W waits for the flush below
  BatchScope wbatch(ctx, has_w && prob->reductionsBatchable());
  if (has_w) {  // Cw = 1/(sw/zsw + tw/ztw + Aw Dinv Aw^T) (:1912-1930)
    PO_TRY(prob->sparseFactorFromSlacks(x, Dinv, wv(), Cw));  // Cdiag (:1912-1927) + mat->factor (:1930)
    fuse_tw = rhs_mu && m > 0 && m + 1 <= kWgramMaxVecs && !corrector_active;
    if (fuse_tw) {
      PO_TRY(computeResidualW(*rhs_mu, true, true));  // ... with d2 of the block solve below (wd2)
      if (!raw_d1_w)
        PO_TRY(k_d1(ctx, bounds(), rx->d, nullptr, options.real("rel_bound_barrier") * (*rhs_mu), n, d1v->d));
      PO_TRY(applyK0(d1v->d, wd2->d, tvec, wyw));
    }
  }
  // structured sparse constraints: the panel image U = Aw (Dinv o P) of the Gram correction rides in the Gram pass
  // itself (one pass over the panel instead of two) where the problem and the kernel allow it
  GramGroups gram_groups;
  std::vector<double *> Ugs;
  if (has_w && m > 0 && prob->sparseGramGroups(x, &gram_groups)) {
    PO_TRY(panelImageVectors(m, Ugs));
    gram_groups.ncols = m;
    gram_groups.U = Ugs.data();
    plan.groups = &gram_groups;
  }
  // 2. the Gram pass; with the right-hand side t at hand, P^T t of the first solve comes out of it
  plan.with_t = (fuse_t || fuse_tw) && m > 0 && m + 1 <= kWgramMaxVecs;
  plan.may_defer = wbatch.open;
  bool panel_done = false;
  kkt.W.assign((size_t)m * m, 0.0);
  t0dots.clear();
  if (m > 0) PO_TRY(gramPass(plan, &panel_done));
  if (fuse_z) qn->pendingZDone();
  if (plan.with_t) {
    scratch_flags.t0_valid = true;
    t0_mu = *rhs_mu;
  }
  // W -= U^T Cw U (d1v is free again: scratch of the panel image; tvec holds t)
  if (has_w) PO_TRY(sparseGramCorrection(P, m, fuse_tw ? d1v : tvec, wbatch.open, panel_done));
  PO_TRY(wbatch.end());
  // test aid: a relative perturbation of 1e-9 in one Gram entry, which the known-answer tests must detect
  // (tests/test_gpu_kat.py::test_kat_detects_a_perturbed_gram)
  // -- reachable only through po_debug_set_switch and only inside po_ip_debug_kkt (no environment variable)
  if (m > 1 && debug_keep_schur && dbg_switch(SW_PERTURB_W) != 0) {
    kkt.W[1] *= 1.0 + 1e-9;
    kkt.W[m] = kkt.W[1];
  }
  const double *d0 = nullptr, *M = nullptr;
  if (k > 0) {
    double b0_;
    qn->getCompactMat(&b0_, &d0, &M, nullptr);
  }
  kkt.factor(vars, d0, M, debug_keep_schur ? &Gmat0 : nullptr, debug_keep_schur ? &Ce0 : nullptr);
  if (k == 0) Ce0.clear();
  return PO_OK;
}

// One application of [K0 + quasi-Newton correction]^-1 (computeKKTStep :2700-2737 with both
// solveKKTDiagSystem overloads :2074-2369 folded together).
//   first pass : b is the residual (rx on the device, dense blocks in `b`)  -> writes px, pzl, pzu
//   refine pass: tvec already holds Dinv*d1' (k_res_step)                    -> accumulates
int InteriorPoint::solveKKT(const Dense &b, double mu, bool use_qn, bool refine_pass, double tau,
                            Dense &out, bool fuse_residual) {
  const double beta_mu = options.real("rel_bound_barrier") * mu;
  const int k = (qn && use_qn) ? qn->size() : 0;
  PO_TRY(kkt.checkWidth(k));
  const int m = c + k;
  // The panel [Ac | Z] is only asked for when a pass needs it: zPointers() FORMS unformed L-SR1 columns (one pass
  // over 3k vectors, k of them written).
  std::vector<const double *> P;
  bool have_panel = false;
  auto need_panel = [&]() {
    if (!have_panel) {
      int k2 = 0;
      P = panel(use_qn, &k2);
      have_panel = true;
    }
  };
  const bool corr = corrector_active && !refine_pass;
  // (corrector_fused: the corrector products are formed inside the two passes below from the affine step in
  // (px, pzl, pzu), nothing was stored in s_qn / y_qn)
  const bool corr_fused = corr && corrector_fused && m >= 1 && m <= kCorrDotsMax;
  const double *cl = (corr && !corr_fused) ? s_qn->d : nullptr;
  const double *cu = (corr && !corr_fused) ? y_qn->d : nullptr;
  if (corr && corrector_fused && !corr_fused) {
    set_error("internal: fused corrector solve with a panel of %d columns", m);
    return PO_ERR_ARG;
  }
  // t = Dinv o d1 and P^T t were produced by setUpKKTSystem's Gram pass when the right-hand side was known then
  const bool have_t0 = !refine_pass && scratch_flags.t0_valid && t0_mu == mu && !corr && (int)t0dots.size() == m;
  std::vector<double> dots(m > 0 ? m : 1, 0.0);
  if (corr_fused) {
    // corrector products, t = Dinv o d1 and P^T t in ONE pass (the bits of k_corrector + k_d1 + k_mdot)
    need_panel();
    PO_TRY(k_corr_d1_dots(ctx, bounds(), px->d, pzl->d, pzu->d, rx->d, Dinv->d, beta_mu, P.data(), m, n, tvec->d,
                          dots.data()));
  } else {
    if (!refine_pass && !have_t0) PO_TRY(k_d1(ctx, bounds(), rx->d, Dinv->d, beta_mu, n, tvec->d, cl, cu));
    if (have_t0) {
      for (int i = 0; i < m; i++) dots[i] = t0dots[i];
    } else if (refine_pass && step_flags.tdots_valid && (int)tdots.size() == m) {
      dots = tdots;  // P^T t' came out of the fused first pass (k_solve2_dots)
    } else if (m > 0) {
      need_panel();
      PO_TRY(k_mdot(ctx, tvec->d, P.data(), m, n, dots.data()));
    }
  }
  // tvec / Dinv are dinv_d1's for this mu
  if (!refine_pass) scratch_flags.first_t_recomputable = have_t0 && scratch_flags.t_is_plain_dinv_d1;
  if (!refine_pass) scratch_flags.t0_valid = false;  // tvec is overwritten by the passes below
  const bool deferred = refine_pass && step_flags.step_deferred;  // the first pass stored no step
  const Bordered::Sol sol = solveBordered(b, dots.data(), refine_pass);
  // Fused refinement residual: the coefficients of addKKTResStep (:1475-1483) are known before
  // the axpy pass starts (A-part = p.z = alpha_A; Z-part = d0 M^-1 d0 Z^T px with Z^T px = ptpx),
  // so the same pass over P also emits the right-hand side t' of the refinement solve.
  const bool seq_lin = options.integer("sequential_linear_method");
  const int kq = (qn && !seq_lin) ? qn->size() : 0;
  // (a panel wider than one kernel's argument tables takes the plain sequence: the launchers collapse it, kernels.hip)
  const bool fuse = fuse_residual && !refine_pass && forms.analytic_panel_dots && kq == k &&
                    !options.integer("use_diag_hessian") && !inexact_newton_step && m <= kMaxPanel;
  step_flags.vA_valid = true;
  std::vector<double> coef(m > 0 ? m : 1, 0.0);
  double diag = options.real("qn_sigma");
  if (fuse) PO_TRY(residualCoefs(qn && !seq_lin ? RES_QN : RES_SIGMA, sol.coef.data(), ptpx.data() + c, k, coef, &diag));
  need_panel();
  const SolvePass sp{P, sol.coef, m, beta_mu, tau};
  if (fuse && m > 0 && !corr) {
    PO_TRY(fusedFirstPass(sp, coef, diag));
  } else if (deferred) {
    PO_TRY(recomputingRefinementPass(sp, corr));
  } else if (corr_fused) {
    PO_TRY(correctorSolve(sp));
  } else {
    PO_TRY(storedStepSolve(sp, refine_pass, fuse ? coef.data() : nullptr, diag, cl, cu));
  }
  step_flags.residual_fused = fuse;
  kkt.backSubstitute(1.0, b, vars, sol, true, out);
  return PO_OK;
}

// The head of the bordered solve that solveKKT and solveKKTW share: every record of the previous step is dropped, the
// dense algebra yields the panel coefficients (sol.coef) from dots = P^T t, and ptpx = P^T px of the step about to be
// written follows analytically, P^T (t + Dinv P coef) = dots + W coef (step_flags.ptpx_valid).
Bordered::Sol InteriorPoint::solveBordered(const Dense &b, const double *dots, bool refine_pass) {
  stepWillChange();
  Bordered::Sol sol;
  kkt.solve(1.0, b, vars, dots, &sol);
  kkt.panelDots(dots, sol, refine_pass, &ptpx);
  step_flags.ptpx_valid = true;
  return sol;
}

// Fused first pass -- taken for the first solve of a step whose refinement residual can be written as panel
// coefficients (`fuse` in solveKKT), m > 0, no corrector.  One pass: t' = refinement rhs and P^T t' for the refinement
// solve.  Sets tdots_valid and step_deferred (with alpha_first, coef_first, diag_first).
int InteriorPoint::fusedFirstPass(const SolvePass &sp, const std::vector<double> &coef, double diag) {
  const int m = sp.m;
  // The step itself (px, pzl, pzu, A^T pz) is NOT stored: the refinement pass recomputes it from (t, alpha) in registers
  // (k_solve2r) -- four output streams less, and an HBM write costs about four reads here.  t' goes to xt (free during
  // the solves), t stays in tvec.
  std::vector<double> out(m + 2, 0.0);
  const bool defer = forms.recompute_first_step;
  // ... and with recompute_rhs not even t': the pass only takes the products P^T t', the refinement pass forms t'
  // again from the residual coefficients (an output stream costs about four input streams)
  double *tp_out = !defer ? tvec->d : (forms.recompute_rhs ? nullptr : xt->d);
  // Dinv and t re-formed in the element epilogue from the bound data and rx it loads anyway (same bits)
  const bool redo_dt1 = forms.recompute_dt && defer && forms.recompute_rhs && scratch_flags.first_t_recomputable;
  PO_TRY(k_solve2_dots(ctx, {.b = bounds(), .t = redo_dt1 ? nullptr : tvec->d, .dinv = Dinv->d,
                             .alpha = sp.alpha.data(), .coef2 = coef.data(), .P = sp.P.data(), .nv = m,
                             .beta_mu = sp.beta_mu, .tau = sp.tau, .rx = rx->d, .diag = diag, .n = n, .px = px->d,
                             .pzl = pzl->d, .pzu = pzu->d, .tout = tp_out, .va = vA->d, .nca = c, .out = out.data(),
                             .store_step = defer ? 0 : 1, .dinv_diag = t0_diag}));
  tdots.assign(out.begin(), out.begin() + m);
  step_flags.tdots_valid = true;
  step_mins[0] = out[m];
  step_mins[1] = out[m + 1];
  step_flags.step_deferred = defer;
  if (defer) {
    alpha_first = sp.alpha;
    coef_first = coef;
    diag_first = diag;
  }
  return PO_OK;
}

// Recomputing refinement pass -- taken for the refinement solve after a fused first pass that stored no step
// (step_deferred): the first step is re-formed from (t, alpha_first) and the refinement applied on top in one sweep.
// Sets fused_merit_valid when it takes the merit sums, and clears pz_stored (with step_beta_mu) for a lean step.
int InteriorPoint::recomputingRefinementPass(const SolvePass &sp, bool corr) {
  // the same sweep takes the sums the complementarity check of scaleKKTStep and the merit derivative need of the
  // final step (see solve2r_kernel): no separate pass over the step afterwards
  const bool take_merit = forms.fuse_merit && forms.recompute_rhs && !corr;
  // lean step: (pzl, pzu) stay in registers; their only consumer left, the multiplier update, re-forms them
  const bool lean = forms.lean_step && lean_step_allowed && take_merit && iterate_flags.iterate_logs_valid;
  // Dinv and the first right-hand side t re-formed in registers from data the pass loads anyway (same bits)
  const bool redo_dt = forms.recompute_dt && forms.recompute_rhs && scratch_flags.first_t_recomputable;
  if (lean) {
    step_flags.pz_stored = false;
    step_beta_mu = sp.beta_mu;
  }
  PO_TRY(k_solve2r(ctx, {.b = bounds(), .t1 = redo_dt ? nullptr : tvec->d,
                         .t2 = forms.recompute_rhs ? nullptr : xt->d, .dinv = Dinv->d, .a1 = alpha_first.data(),
                         .a2 = sp.alpha.data(), .P = sp.P.data(), .nv = sp.m, .beta_mu = sp.beta_mu, .tau = sp.tau,
                         .n = n, .px = px->d, .pzl = lean ? nullptr : pzl->d, .pzu = lean ? nullptr : pzu->d,
                         .va = vA->d, .nca = c, .out = step_mins, .ar = coef_first.data(), .rx = rx->d,
                         .diag = diag_first, .g = take_merit ? g->d : nullptr,
                         .merit_out = take_merit ? fused_merit.as_array() : nullptr, .dinv_diag = t0_diag}));
  if (take_merit) {
    after_reduce(ctx, [this] {
      step_mins[0] = fused_merit.max_x;
      step_mins[1] = fused_merit.max_z;
      step_flags.fused_merit_valid = true;
    });
  }
  return PO_OK;
}

// Corrector solve -- taken for the first solve of a Mehrotra corrector whose products were not stored
// (corrector_fused, 1 <= m <= kCorrDotsMax): the corrector terms are re-formed from the affine step this pass
// overwrites, and it takes the sums of scaleKKTStep / evalMeritInitDeriv of the step it has in registers (k_comp_merit
// and its round trip disappear).  Sets fused_merit_valid and, when it took them, iterate_logs_valid.
int InteriorPoint::correctorSolve(const SolvePass &sp) {
  const bool want_logs = !iterate_flags.iterate_logs_valid;
  PO_TRY(k_solve2c(ctx, {.b = bounds(), .t = tvec->d, .dinv = Dinv->d, .alpha = sp.alpha.data(), .P = sp.P.data(),
                         .nv = sp.m, .beta_mu = sp.beta_mu, .tau = sp.tau, .n = n, .px = px->d, .pzl = pzl->d,
                         .pzu = pzu->d, .va = vA->d, .nca = c, .g = g->d, .want_logs = want_logs ? 1 : 0,
                         .out = corr_out.as_array()}));
  after_reduce(ctx, [this, want_logs] {
    const CorrectorSums &o = corr_out;
    fused_merit = {.S10 = o.S10, .S01 = o.S01, .S11 = o.S11, .ppos = o.ppos, .pneg = o.pneg, .gpx = o.gpx,
                   .pxpx = o.pxpx, .max_x = o.max_x, .max_z = o.max_z, .px_amax = o.px_amax};
    step_mins[0] = o.max_x;
    step_mins[1] = o.max_z;
    if (want_logs) {  // the barrier sums of the iterate, as k_comp_merit takes them
      iterate_logs[0] = o.pos_log;
      iterate_logs[1] = o.neg_log;
      iterate_flags.iterate_logs_valid = true;
    }
    step_flags.fused_merit_valid = true;
  });
  return PO_OK;
}

// Stored-step solve -- every other case: the first solve or a refinement on top of the step in (px, pzl, pzu), with
// stored corrector products (cl, cu) if any; coef2 != nullptr: the same pass writes the refinement right-hand side t'
// over tvec.  Sets no flag of its own.
int InteriorPoint::storedStepSolve(const SolvePass &sp, bool refine_pass, const double *coef2, double diag,
                                   const double *cl, const double *cu) {
  return k_solve2(ctx, {.b = bounds(), .t = tvec->d, .dinv = Dinv->d, .alpha = sp.alpha.data(), .P = sp.P.data(),
                        .nv = sp.m, .beta_mu = sp.beta_mu, .refine = refine_pass ? 1 : 0, .tau = sp.tau, .n = n,
                        .px = px->d, .pzl = pzl->d, .pzu = pzu->d, .out = step_mins, .coef2 = coef2, .rx = rx->d,
                        .diag = diag, .tout = tvec->d, .va = vA->d, .nca = c, .cl = cl, .cu = cu});
}

int InteriorPoint::computeKKTStepWithRefinement(double mu, bool use_qn, double tau) {
  const int nref = options.integer("iterative_refinement_steps");
  const double beta_mu = options.real("rel_bound_barrier") * mu;
  const bool with_qn = qn && !options.integer("sequential_linear_method");
  const int mq = c + (with_qn ? qn->size() : 0);
  // -H px (inexact Newton step) or -h o px in place of the quasi-Newton term.  The sparse path leaves the inexact
  // Newton step out, which the reference does not (:1461), and tests hdiag besides the option
  const bool diag_hess = options.integer("use_diag_hessian") && (!has_w || hdiag);
  const ResTerm term = (!has_w && inexact_newton_step) ? RES_HVEC
                       : diag_hess                     ? RES_HDIAG
                       : with_qn                       ? RES_QN
                                                       : RES_SIGMA;
  // (setUpKKTSystem did it for the fused first solve)
  if (has_w && !(scratch_flags.t0_valid && t0_mu == mu)) PO_TRY(computeResidualW(mu));
  denseResidual(mu, res);
  PO_TRY(has_w ? solveKKTW(res, mu, use_qn, false, tau, step, nref > 0)
               : solveKKT(res, mu, use_qn, false, tau, step, nref > 0));
  for (int it = 0; it < nref; it++) {  // :4985-4991
    LazyPanel Pq{this, with_qn};
    if (has_w) Pq.get();  // (the sparse path takes it up front, streamed or not)
    std::vector<double> dots;  // A px for r'.z, Z^T px for B px
    PO_TRY(stepPanelDots(Pq, dots));
    std::vector<double> coef(mq + 2, 0.0);
    double diag = 0.0;
    PO_TRY(residualCoefs(term, step.z.data(), dots.data() + c, mq - c, coef, &diag));
    int mres = mq;
    if (term == RES_HVEC || term == RES_HDIAG) {
      Pq.get().push_back(xt->d);
      mres++;
    }
    // addKKTResStep (:1451-1583): the design rows, Dinv o d1' into tvec or -- sparse path -- the raw d1' into d1v with
    // the extra column Aw^T pzw; already there when the first solve ran in its fused form
    if (!(it == 0 && step_flags.residual_fused)) {
      if (has_w) {
        if (prob->setSparseJacobianTranspose(1.0, x, wstepv[0], tvec) != 0) return PO_ERR_USER;
        Pq.get().push_back(tvec->d);
        coef[mres++] = 1.0;
      }
      PO_TRY(k_res_step(ctx, bounds(), rx->d, px->d, pzl->d, pzu->d, has_w ? nullptr : Dinv->d, coef.data(),
                        Pq.get().data(), mres, diag, beta_mu, n, has_w ? d1v->d : tvec->d));
    }
    if (has_w) {
      // sparse rows (:1492-1527); only the blocks are rebuilt here.  w_sums / w_maxs are deliberately LEFT at the
      // norms of the iterate's own barrier parameter (the affine solve of the Mehrotra strategies runs this with
      // mu = 0, and nothing reads the norms before the next computeResidual evaluates them again)
      PO_TRY(computeResidualW(mu, false));
      if (prob->addSparseJacobian(-1.0, x, px, wresv[0]) != 0) return PO_ERR_USER;
      PO_TRY(k_w_res_step(ctx, wv(), wp(), wr(), nw, wd2->d));  // ... and d2 of the refinement's block solve
      scratch_flags.wd2_ready = true;
    }
    Dense r2;
    r2.resize(c);
    denseResidual(mu, r2);
    denseResStep(vars, step, dots.data(), r2);
    PO_TRY(has_w ? solveKKTW(r2, mu, use_qn, true, tau, refine) : solveKKT(r2, mu, use_qn, true, tau, refine));
    for (int i = 0; i < c; i++) {
      step.z[i] += refine.z[i];
      step.s[i] += refine.s[i];
      step.t[i] += refine.t[i];
      step.zs[i] += refine.zs[i];
      step.zt[i] += refine.zt[i];
    }
  }
  sx = sz = 1.0;
  return PO_OK;
}

int InteriorPoint::checkKKTStep(int iteration, double mu) {
  const double beta_mu = options.real("rel_bound_barrier") * mu;
  // lean step: materialise the bound-multiplier steps exactly as the update will form them
  if (!step_flags.pz_stored) {
    PO_TRY(k_form_pz(ctx, bounds(), px->d, step_beta_mu, n, pzl->d, pzu->d));
    step_flags.pz_stored = true;
  }
  const bool seq_lin = options.integer("sequential_linear_method");
  int kq = 0;
  std::vector<const double *> Pq = panel(qn && !seq_lin, &kq);
  const int mq = c + kq;
  std::vector<double> dots(mq > 0 ? mq : 1, 0.0), coef(mq > 0 ? mq : 1, 0.0);
  if (mq > 0) PO_TRY(k_mdot(ctx, px->d, Pq.data(), mq, n, dots.data()));  // explicit: this is a check
  double diag = 0.0;
  const bool with_qn = qn && !seq_lin && !options.integer("use_diag_hessian");
  PO_TRY(residualCoefs(with_qn ? RES_QN : RES_SIGMA, step.z.data(), dots.data() + c, kq, coef, &diag));
  if (has_w) {  // the sparse multiplier step enters r'x through Aw^T pzw: one more column
    if (prob->setSparseJacobianTranspose(1.0, x, wstepv[0], xt) != 0) return PO_ERR_USER;
    Pq.push_back(xt->d);
    coef.push_back(1.0);
  }
  double mx[3];
  PO_TRY(computeResidual(mu, true));  // fresh rx, as the reference recomputes it (:6216)
  PO_TRY(k_step_check(ctx, bounds(), rx->d, px->d, pzl->d, pzu->d, coef.data(), Pq.data(), (int)Pq.size(), diag,
                      beta_mu, n, mx));
  Dense r;
  r.resize(c);
  denseResidual(mu, r);
  denseResStep(vars, step, dots.data(), r);
  double mz = 0.0, ms = 0.0, mt = 0.0, mzs = 0.0, mzt = 0.0;
  for (int i = 0; i < c; i++) {
    mz = std::max(mz, fabs(r.z[i]));
    ms = std::max(ms, fabs(r.s[i]));
    mt = std::max(mt, fabs(r.t[i]));
    mzs = std::max(mzs, fabs(r.zs[i]));
    mzt = std::max(mzt, fabs(r.zt[i]));
  }
  if (ctx->rank == 0) {
    char line[640];
    snprintf(line, sizeof(line),
             "\nResidual step check for iteration %d:\n"
             "max |stationarity (x block)|:             %10.4e\n"
             "max |dense constraints (z block)|:        %10.4e\n"
             "max |slack duals (s block)|:              %10.4e\n"
             "max |slack duals (t block)|:              %10.4e\n"
             "max |slack complementarity (zs block)|:   %10.4e\n"
             "max |slack complementarity (zt block)|:   %10.4e\n"
             "max |lower-bound complementarity (zl)|:   %10.4e\n"
             "max |upper-bound complementarity (zu)|:   %10.4e\n",
             iteration, mx[0], mz, ms, mt, mzs, mzt, mx[1], mx[2]);
    history += line;
  }
  return PO_OK;
}

int InteriorPoint::checkGradients(double dh, std::string *report) {  // :6196-6199
  scratchLent();  // (tvec and xt are its scratch)
  return prob->checkGradients(dh, x, options.integer("use_hvec_product"), xt, tvec, report);
}

int InteriorPoint::checkMeritFuncGradient(Vec *xpt, double dh, double out[2]) {  // :3280-3432
  if (xpt) PO_TRY(k_copy(ctx, x->d, xpt->d, n));
  iterateReplaced();
  if (prob->evalObjCon(x, &fobj, cvals.data()) != 0) {
    fprintf(stderr, "ParOpt: Function and constraint evaluation failed\n");
    return PO_ERR_USER;
  }
  neval++;
  if (prob->evalObjConGradient(x, g, Ac.data()) != 0) {
    fprintf(stderr, "ParOpt: Gradient evaluation failed\n");
    return PO_ERR_USER;
  }
  ngeval++;
  iterate_flags.ac_valid = true;
  if (xpt) {  // a direction of our own: px = -g / |g|, fixed slack steps, zero elsewhere (:3327-3352)
    double g2 = 0.0;
    PO_TRY(k_reduce1(ctx, RED_SUMSQ, g->d, nullptr, n, &g2));
    PO_TRY(k_panel_axpy(ctx, px->d, g2 > 0.0 ? -1.0 / sqrt(g2) : 0.0, g->d, 0.0, nullptr, nullptr, 0, n));
    for (int i = 0; i < c; i++) {
      step.s[i] = -0.259 * (1 + (i % 3));
      step.t[i] = -0.349 * (4 - (i % 2));
    }
    if (has_w && nw > 0) {
      std::vector<double> hs((size_t)nw), ht((size_t)nw);
      for (int64_t i = 0; i < nw; i++) {
        hs[i] = -0.419 * (1 + (i % 5));
        ht[i] = -0.7513 * (1 + (i % 19));
      }
      PO_HIP(hipMemcpyAsync(wstepv[1]->d, hs.data(), sizeof(double) * (size_t)nw, hipMemcpyHostToDevice, ctx->stream));
      PO_HIP(hipMemcpyAsync(wstepv[2]->d, ht.data(), sizeof(double) * (size_t)nw, hipMemcpyHostToDevice, ctx->stream));
      PO_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  sx = sz = 1.0;
  stepWillChange();  // (a lean step keeps px only; nothing below reads pzl / pzu)
  double m0 = 0.0, dm0 = 0.0;
  PO_TRY(evalMeritInitDeriv(1.0, &m0, &dm0));
  // the merit function at (x + dh px, s + dh ps, t + dh pt, sw + dh psw, tw + dh ptw) (:3386-3409)
  const double eps = 0.0;  // no clamping: the reference evaluates the perturbed point as it is
  double sums[2], wsums[5];
  std::vector<double> rs(c), rt(c), cs(cvals);
  for (int i = 0; i < c; i++) {
    rs[i] = vars.s[i] + dh * step.s[i];
    rt[i] = vars.t[i] + dh * step.t[i];
  }
  {
    // k_trial clamps into [lb + eps, ub - eps]; with eps = 0 an interior point is left alone
    PO_TRY(k_trial(ctx, bounds(), px->d, dh, eps, n, xt->d, sums));
  }
  double ftemp = 0.0;
  if (prob->evalObjCon(xt, &ftemp, cs.data()) != 0) {
    fprintf(stderr, "ParOpt: Function and constraint evaluation failed\n");
    return PO_ERR_USER;
  }
  neval++;
  if (has_w) {
    if (prob->evalSparseCon(xt, wtmp) != 0) return PO_ERR_USER;
    PO_TRY(k_w_trial(ctx, wv(), wp(), dh, eps, gsw->d, gtw->d, wtmp->d, nw, wsums));
  }
  const double m1 = evalMeritFromSums(ftemp, cs.data(), rs.data(), rt.data(), sums[0], sums[1], has_w ? wsums : nullptr);
  const double fd = (m1 - m0) / dh;
  if (ctx->rank == 0) {
    fprintf(stdout, "Merit function test\n");
    fprintf(stdout, "dm FD: %15.8e  Actual: %15.8e  Err: %8.2e  Rel err: %8.2e\n", fd, dm0, fabs(fd - dm0),
            fabs((fd - dm0) / fd));
    fflush(stdout);
  }
  if (out) {
    out[0] = fd;
    out[1] = dm0;
  }
  return PO_OK;
}

int InteriorPoint::debugKKTStep(double mu) {
  PO_TRY(createQuasiNewton());
  PO_TRY(computeResidual(mu, true));
  PO_TRY(setUpKKTSystem(true));
  denseResidual(mu, res);
  if (has_w) {
    PO_TRY(solveKKTW(res, mu, true, false, 0.95, step));
  } else {
    PO_TRY(solveKKT(res, mu, true, false, 0.95, step));
  }
  sx = sz = 1.0;
  return PO_OK;
}

int InteriorPoint::debugSetState(const double *z, const double *s, const double *t, const double *zs,
                                 const double *zt, double mu) {
  PO_TRY(createQuasiNewton());
  for (int i = 0; i < c; i++) {
    vars.z[i] = z[i];
    vars.s[i] = s[i];
    vars.t[i] = t[i];
    vars.zs[i] = zs[i];
    vars.zt[i] = zt[i];
  }
  barrier_param = mu;
  {
    const std::string nt = options.str("norm_type");
    norm_type = nt == "infinity" ? 0 : (nt == "l1" ? 1 : 2);
  }
  // nothing carried between the passes of an iteration survives a state written from outside
  stateReplaced();
  spec_enabled = false;
  corrector_active = false;
  inexact_newton_step = false;
  if (prob->evalObjCon(x, &fobj, cvals.data()) != 0) return PO_ERR_USER;
  if (prob->evalObjConGradient(x, g, Ac.data()) != 0) return PO_ERR_USER;
  iterate_flags.ac_valid = true;
  return PO_OK;
}

int InteriorPoint::debugKKT(double mu, int mode, double tau) {
  struct KeepSchur {  // G and Ce as assembled are copied for the dump of THIS call only
    bool &f;
    explicit KeepSchur(bool &f_) : f(f_) { f = true; }
    ~KeepSchur() { f = false; }
  } keep(debug_keep_schur);
  if (mode == 0) {
    PO_TRY(debugKKTStep(mu));
  } else if (mode == 2) {
    // the predictor-corrector step of optimize() from the injected state (round 6): residual and complementarity of the
    // iterate, KKT system for the affine right-hand side (mu = 0), then mehrotraStep -- affine solve + refinement, the
    // Mehrotra rule, corrector right-hand side and solve.  Leaves the new barrier parameter in barrier_param.
    PO_TRY(createQuasiNewton());
    const bool use_qn = !options.integer("sequential_linear_method");
    barrier_param = mu;
    PO_TRY(computeResidual(mu, true));
    const double comp = compFromSums(comp_prod, comp_count, vars, w_sums[0]);
    const double rhs_mu = 0.0;
    PO_TRY(setUpKKTSystem(use_qn, false, &rhs_mu));
    double tau_new = tau;
    PO_TRY(mehrotraStep(use_qn, comp, true, options.real("min_fraction_to_boundary"), options.real("abs_res_tol"),
                        &tau_new));
    (void)tau_new;
    PO_TRY(batch_flush(ctx));
  } else {
    PO_TRY(createQuasiNewton());
    PO_TRY(computeResidual(mu, true));
    PO_TRY(setUpKKTSystem(true, false, &mu));
    lean_step_allowed = false;  // (pzl, pzu) are stored: the test reads them
    PO_TRY(computeKKTStepWithRefinement(mu, true, tau));
    PO_TRY(batch_flush(ctx));
  }
  denseResidual(mu, res);
  resNorms(res, &debug_norms[0], &debug_norms[1], &debug_norms[2], &debug_norms[3]);
  return PO_OK;
}

// The Mehrotra strategies' step from a set-up KKT system (optimize() :4956-5045): affine (mu = 0) predictor with one
// refinement, probe to the boundary (tau = 1), complementarity there, sigma = (comp_affine / comp)^3 >= 0.01, the new
// barrier parameter, then either the corrector solve (predictor-corrector: affine products in the residual, no
// refinement) or a plain solve at the new parameter.  Leaves the step in (px, pzl, pzu, step), the new barrier
// parameter in barrier_param and the fraction to the boundary that goes with it in *tau_out.
int InteriorPoint::mehrotraStep(bool use_qn, double comp, bool corrector, double min_frac, double abs_res_tol,
                                double *tau_out) {
  // affine (mu = 0) predictor step, probed all the way to the boundary (:4956-5009)
  PO_TRY(computeKKTStepWithRefinement(0.0, use_qn, 1.0));
  double max_x = std::min(1.0, step_mins[0]), max_z = std::min(1.0, step_mins[1]);
  for (int i = 0; i < c; i++) {
    if (step.s[i] < 0.0) max_x = std::min(max_x, -vars.s[i] / step.s[i]);
    if (step.t[i] < 0.0) max_x = std::min(max_x, -vars.t[i] / step.t[i]);
    if (step.zs[i] < 0.0) max_z = std::min(max_z, -vars.zs[i] / step.zs[i]);
    if (step.zt[i] < 0.0) max_z = std::min(max_z, -vars.zt[i] / step.zt[i]);
  }
  double cs[2];
  if (step_flags.fused_merit_valid && !has_w && dbg_switch(SW_MPC_POLY) != 0) {
    // the refinement pass of the affine solve took the complementarity polynomial of its step (solve2r_kernel):
    // S00 + ax S10 + az S01 + ax az S11 at the probe lengths, S00 / the bound count from the residual pass of this
    // iterate -- no pass over the step and no host round trip (round 6; scaleKKTStep uses the same form)
    cs[0] = comp_prod + max_x * fused_merit.S10 + max_z * fused_merit.S01 + max_x * max_z * fused_merit.S11;
    cs[1] = comp_count;
  } else {
    PO_TRY(k_comp_step(ctx, bounds(), px->d, pzl->d, pzu->d, max_x, max_z, n, cs));
  }
  double prod = cs[0] / options.real("rel_bound_barrier"), count = cs[1];
  if (has_w) {
    double wprod = 0.0;
    PO_TRY(wCompStep(max_x, max_z, &wprod));
    prod += wprod;
    count += 2.0 * nw_global;
  }
  for (int i = 0; i < c; i++) {
    prod += ((vars.s[i] + max_x * step.s[i]) * (vars.zs[i] + max_z * step.zs[i]) +
             (vars.t[i] + max_x * step.t[i]) * (vars.zt[i] + max_z * step.zt[i]));
    count += 2.0;
  }
  const double comp_affine = count != 0.0 ? prod / count : 0.0;
  const double s1 = comp_affine / comp;
  double sigma = s1 * s1 * s1;
  if (sigma < 0.01) sigma = 0.01;
  barrier_param = sigma * comp;
  if (barrier_param < 0.09999 * abs_res_tol) barrier_param = 0.09999 * abs_res_tol;
  const double tau = fractionToBoundary(barrier_param, min_frac);
  *tau_out = tau;
  if (corrector) {
    // corrector: res.zl -= px*pzl, res.zu += px*pzu, res.zs -= ps*pzs, res.zt -= pt*pzt of the
    // affine step (:1729-1789); no refinement with the corrector (:5040-5041)
    // (one-pass corrector right-hand side + corrector solve with the merit sums: see solveKKT)
    corrector_fused = !has_w && c + kkt.k >= 1 && c + kkt.k <= kCorrDotsMax &&
                      dbg_switch(SW_MPC_FUSE) != 0;
    if (!corrector_fused) PO_TRY(k_corrector(ctx, bounds(), px->d, pzl->d, pzu->d, n, s_qn->d, y_qn->d));
    denseResidual(barrier_param, res);
    for (int i = 0; i < c; i++) {
      res.zs[i] -= step.s[i] * step.zs[i];
      res.zt[i] -= step.t[i] * step.zt[i];
    }
    if (has_w) {
      PO_TRY(computeResidualW(barrier_param));
      PO_TRY(k_w_corrector(ctx, wp(), wr(), nw));
    }
    corrector_active = true;
    int rcs = has_w ? solveKKTW(res, barrier_param, use_qn, false, tau, step)
                    : solveKKT(res, barrier_param, use_qn, false, tau, step);
    corrector_active = false;
    corrector_fused = false;
    PO_TRY(rcs);
    sx = sz = 1.0;
  } else {
    PO_TRY(computeKKTStepWithRefinement(barrier_param, use_qn, tau));
  }
  return PO_OK;
}

// ================================================================================================
// step lengths
// ================================================================================================
int InteriorPoint::scaleKKTStep(double tau, double comp, double *alpha_x, double *alpha_z, int *ceq,
                                bool inexact) {  // :3196-3274 with computeMaxStep :2942-3103
  double ax = std::min(1.0, step_mins[0]), az = std::min(1.0, step_mins[1]);
  for (int i = 0; i < c; i++) {
    if (step.s[i] < 0.0) ax = std::min(ax, -tau * vars.s[i] / step.s[i]);
    if (step.t[i] < 0.0) ax = std::min(ax, -tau * vars.t[i] / step.t[i]);
    if (step.zs[i] < 0.0) az = std::min(az, -tau * vars.zs[i] / step.zs[i]);
    if (step.zt[i] < 0.0) az = std::min(az, -tau * vars.zt[i] / step.zt[i]);
  }
  *ceq = 0;
  if (inexact) {  // Newton step: one common step length (:3240-3248)
    if (ax > az) {
      ax = az;
    } else {
      az = ax;
    }
    sx = ax;
    sz = az;
    for (int i = 0; i < c; i++) {
      step.s[i] *= ax;
      step.t[i] *= ax;
      step.z[i] *= az;
      step.zs[i] *= az;
      step.zt[i] *= az;
    }
    *alpha_x = ax;
    *alpha_z = az;
    return PO_OK;
  }
  const double max_bnd = 100.0;
  if (ax > az) {
    if (ax > max_bnd * az) {
      ax = max_bnd * az;
    } else if (ax < az / max_bnd) {
      ax = az / max_bnd;
    }
  } else {
    if (az > max_bnd * ax) {
      az = max_bnd * ax;
    } else if (az < ax / max_bnd) {
      az = ax / max_bnd;
    }
  }
  double out[9], wprod = 0.0;
  if (step_flags.fused_merit_valid && iterate_flags.iterate_logs_valid && (!has_w || step_flags.w_comp_valid)) {
    // (sparse constraints: the slacks' share of the polynomial came out of the step kernel, S00 = the complementarity
    // sum of the iterate's sparse slacks from its residual pass)
    if (has_w) wprod = w_sums[0] + ax * w_comp_poly[0] + az * w_comp_poly[1] + ax * az * w_comp_poly[2];
    // everything was taken by the refinement pass: the complementarity at the scaled step is
    // S00 + ax S10 + az S01 + ax az S11 with S00 / the bound count from the residual pass of this iterate.
    // Tolerance: near convergence S00 and the S10 / S01 terms nearly cancel, so the polynomial carries a relative
    // error of a few ulp of S00 where the direct sum of products has a few ulp of the result; the value only feeds the
    // comp_new > 10 comp test below (a factor-of-ten threshold), and the cmpEq tokens of all reference trajectories are
    // reproduced with it (tests/test_gpu_ip.py; A/B against the plain pass: test_write_saving_fusions_...).
    // Validity: comp_prod / iterate_logs belong to (x, zl, zu) as the last residual pass saw them.  Every internal
    // writer of the iterate clears the flags; an iteration callback or a getArray view must not WRITE the iterate
    // mid-solve (po_ip_set_iteration_callback: an observer) -- resetDesignAndBounds / readSolutionFile between solves
    // refresh mirrors and flags (vec_mirror_refresh)
    out[0] = comp_prod + ax * fused_merit.S10 + az * fused_merit.S01 + ax * az * fused_merit.S11;
    out[1] = comp_count;
    merit_cache = {.pos_log = iterate_logs[0], .neg_log = iterate_logs[1], .ppos = fused_merit.ppos,
                   .pneg = fused_merit.pneg, .gpx = fused_merit.gpx, .pxpx = fused_merit.pxpx,
                   .px_amax = fused_merit.px_amax};
    step_flags.merit_cache_valid = true;
  } else if (!has_w) {
    // one pass also yields the merit pieces and the step norm the line search is about to ask for
    PO_TRY(k_comp_merit(ctx, bounds(), px->d, pzl->d, pzu->d, ax, az, g->d, n, out));
    merit_cache = MeritSums::fromCompMerit(out);
    step_flags.merit_cache_valid = true;
  } else {
    BatchScope batch(ctx);  // design and sparse parts of the complementarity: one collective + sync
    // (the design pass also yields the merit pieces and max|px| the line search is about to ask for, as on the
    // dense path: the separate merit pass and its max|px| reduction disappear)
    PO_TRY(k_comp_merit(ctx, bounds(), px->d, pzl->d, pzu->d, ax, az, g->d, n, out));
    PO_TRY(wCompStep(ax, az, &wprod));  // :2866-2889
    PO_TRY(batch.end());
    merit_cache = MeritSums::fromCompMerit(out);
    step_flags.merit_cache_valid = true;
  }
  double prod = out[0] / options.real("rel_bound_barrier"), count = out[1];
  if (has_w) {
    prod += wprod;
    count += 2.0 * nw_global;
  }
  for (int i = 0; i < c; i++) {
    prod += ((vars.s[i] + ax * step.s[i]) * (vars.zs[i] + az * step.zs[i]) +
             (vars.t[i] + ax * step.t[i]) * (vars.zt[i] + az * step.zt[i]));
    count += 2.0;
  }
  const double comp_new = count != 0.0 ? prod / count : 0.0;
  if (comp_new > 10.0 * comp) {
    *ceq = 1;
    if (ax > az) {
      ax = az;
    } else {
      az = ax;
    }
  }
  // the n-sized parts of the step are scaled lazily; the dense parts right away
  sx = ax;
  sz = az;
  for (int i = 0; i < c; i++) {
    step.s[i] *= ax;
    step.t[i] *= ax;
    step.z[i] *= az;
    step.zs[i] *= az;
    step.zt[i] *= az;
  }
  *alpha_x = ax;
  *alpha_z = az;
  return PO_OK;
}

// ================================================================================================
// merit function and line search
// ================================================================================================
double InteriorPoint::evalMeritFromSums(double fk, const double *ck, const double *sk,
                                        const double *tk, double pos, double neg,
                                        const double *wsums) const {
  // evalMeritFunc :3569-3636 after the reduction of the bound terms; wsums (k_w_trial layout) =
  // {pos log, neg log, |cw - sw + tw|^2, gsw.sw, gtw.tw} of the sparse slacks (not scaled by beta)
  const double beta = options.real("rel_bound_barrier");
  pos *= beta;
  neg *= beta;
  if (wsums) {
    pos += wsums[0];
    neg += wsums[1];
  }
  for (int i = 0; i < c; i++) {
    if (sk[i] > 1.0) pos += log(sk[i]); else neg += log(sk[i]);
    if (tk[i] > 1.0) pos += log(tk[i]); else neg += log(tk[i]);
  }
  double dense_infeas = 0.0;
  for (int i = 0; i < c; i++) {
    const double cv = ck[i] - sk[i] + tk[i];
    dense_infeas += cv * cv;
  }
  double sparse_infeas = 0.0, wgam = 0.0;
  if (wsums) {
    sparse_infeas = sqrt(wsums[2]);
    wgam = wsums[3] + wsums[4];
  }
  const double infeas = sqrt(dense_infeas + sparse_infeas * sparse_infeas);
  double merit = (fk + wgam) - barrier_param * (pos + neg) + rho_penalty_search * infeas;
  for (int i = 0; i < c; i++) merit += gamma_s[i] * sk[i] + gamma_t[i] * tk[i];
  return merit;
}

int InteriorPoint::evalMeritInitDeriv(double max_x, double *merit_, double *pmerit_) {  // :3652-3924
  const double beta = options.real("rel_bound_barrier");
  const double abs_res_tol = options.real("abs_res_tol");
  const double frac = options.real("penalty_descent_fraction");
  const bool seq_lin = options.integer("sequential_linear_method");
  double out[6];
  double wm[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int kq = (qn && !seq_lin) ? qn->size() : 0;
  const int mq = c + kq;
  std::vector<double> dots;
  {
    // design part, panel products (when not known analytically) and sparse part: one collective + sync (the
    // problem's sparse callbacks run in between: built-in problems only)
    BatchScope batch(ctx, has_w && prob->reductionsBatchable());
    if (step_flags.merit_cache_valid) {
      out[0] = merit_cache.pos_log;
      out[1] = merit_cache.neg_log;
      out[2] = sx * merit_cache.ppos;
      out[3] = sx * merit_cache.pneg;
      out[4] = sx * merit_cache.gpx;
      out[5] = sx * sx * merit_cache.pxpx;
    } else {
      PO_TRY(k_merit0(ctx, bounds(), px->d, sx, g->d, n, out));
      if (batch.open) {  // max|px| for the line search's minimum step rides in this batch (its own sync otherwise)
        PO_TRY(k_reduce1(ctx, RED_AMAX, px->d, nullptr, n, &px_amax_w));
        step_flags.px_amax_valid = true;
      }
    }
    LazyPanel Pq{this, qn && !seq_lin};
    PO_TRY(stepPanelDots(Pq, dots));
    if (has_w && step_flags.w_merit_cache_valid) {
      // taken at sx = 1 in the refinement batch (solveKKTW); every sum that depends on the step is linear in sx > 0
      for (int i = 0; i < 10; i++) wm[i] = w_merit_cache[i];
      wm[2] *= sx;
      wm[3] *= sx;
      wm[6] *= sx;
      wm[7] *= sx;
      wm[9] *= sx;
    } else if (has_w) {  // :3735-3765, 3489-3503
      const double *cw = nullptr;
      PO_TRY(sparseConAtIterate(&cw));
      PO_TRY(prob->setSparseJacobian(1.0, x, px, wtmp2));
      PO_TRY(k_w_merit(ctx, wv(), wp(), sx, gsw->d, gtw->d, cw, wtmp2->d, nw, wm));
    }
    PO_TRY(batch.end());
  }
  double pos = out[0] * beta, neg = out[1] * beta, ppos = out[2] * beta, pneg = out[3] * beta;
  const double gpx = out[4], pxpx = out[5];
  for (int i = 0; i < mq; i++) dots[i] *= sx;
  if (has_w) {
    pos += wm[0];
    neg += wm[1];
    ppos += wm[2];
    pneg += wm[3];
  }
  for (int i = 0; i < c; i++) {
    if (vars.s[i] > 1.0) pos += log(vars.s[i]); else neg += log(vars.s[i]);
    if (step.s[i] > 0.0) ppos += step.s[i] / vars.s[i]; else pneg += step.s[i] / vars.s[i];
    if (vars.t[i] > 1.0) pos += log(vars.t[i]); else neg += log(vars.t[i]);
    if (step.t[i] > 0.0) ppos += step.t[i] / vars.t[i]; else pneg += step.t[i] / vars.t[i];
  }
  // evalInfeasDeriv :3465-3509
  double dense_infeas = 0.0, pdense = 0.0;
  for (int i = 0; i < c; i++) {
    const double cval = cvals[i] - vars.s[i] + vars.t[i];
    const double pcval = dots[i] - step.s[i] + step.t[i];
    dense_infeas += cval * cval;
    pdense += cval * pcval;
  }
  const double sparse_infeas = has_w ? sqrt(wm[8]) : 0.0;
  const double psparse = wm[9];
  const double infeas = sqrt(dense_infeas + sparse_infeas * sparse_infeas);
  const double infeas_proj = infeas > 0.0 ? (pdense + psparse) / infeas : 0.0;
  // pTBp = 0.5 px^T B px  (:3820-3821), B px never formed
  double pTBp = 0.0;
  if (options.integer("use_diag_hessian") && hdiag) {  // sum px^2 h (no factor 1/2, :3810-3818)
    PO_TRY(k_mul(ctx, xt->d, 1.0, hdiag->d, px->d, n));
    PO_TRY(k_reduce1(ctx, RED_DOT, xt->d, px->d, n, &pTBp));
    pTBp *= sx * sx;
  } else if (qn && !seq_lin) {
    double v = qn->diag() * pxpx;
    if (kq > 0) {
      std::vector<double> cf = compactInverse(dots.data() + c, kq);
      for (int j = 0; j < kq; j++) v -= dots[c + j] * cf[j];
    }
    pTBp = 0.5 * v;
  }
  double merit = (fobj + (wm[4] + wm[5])) - barrier_param * (pos + neg);
  double pmerit = (gpx + (wm[6] + wm[7])) - barrier_param * (ppos + pneg);
  for (int i = 0; i < c; i++) {
    merit += gamma_s[i] * vars.s[i] + gamma_t[i] * vars.t[i];
    pmerit += gamma_s[i] * step.s[i] + gamma_t[i] * step.t[i];
  }
  double numer = pmerit;
  if (pTBp > 0.0) numer += 0.5 * pTBp;
  double rho_hat = 0.0;
  const bool small = infeas < 0.1 * abs_res_tol;
  if (small) {
    const double denom = -(1.0 - frac) * max_x * infeas;
    if (numer >= 0.0 && denom < 0.0) rho_hat = -(numer / denom);
  } else {
    double denom = infeas_proj + frac * max_x * infeas;
    if (numer >= 0.0) {
      if (denom < 0.0) {
        rho_hat = -(numer / denom);
      } else {
        denom = -(1.0 - frac) * max_x * infeas;
        rho_hat = -(numer / denom);
      }
    }
  }
  if (rho_hat > rho_penalty_search) {
    rho_penalty_search = rho_hat;
  } else {
    rho_penalty_search *= 0.5;
    if (rho_penalty_search < rho_hat) rho_penalty_search = rho_hat;
  }
  const double min_rho = options.real("min_rho_penalty_search");
  if (rho_penalty_search < min_rho) rho_penalty_search = min_rho;
  merit += rho_penalty_search * infeas;
  if (small) {
    pmerit -= rho_penalty_search * max_x * infeas;
  } else {
    pmerit += rho_penalty_search * infeas_proj;
  }
  *merit_ = merit;
  *pmerit_ = pmerit;
  return PO_OK;
}

static void clampStepDense(std::vector<double> &out, const std::vector<double> &v, double alpha,
                           const std::vector<double> &p, double eps, bool lower) {
  for (size_t i = 0; i < v.size(); i++) {
    double val = v[i] + alpha * p[i];
    if (lower && val <= 0.0 + eps) val = 0.0 + eps;
    out[i] = val;
  }
}

// One trial point of the line search: xt = clamp(x + alpha sx px) with its barrier sums and, when the quasi-Newton
// update wants it (sq), s = alpha sx px from the same pass; f and c at xt; with_sparse: cw(xt) in wtmp and the sparse
// slack sums.  t.fail_obj is what evalObjCon returned; a failed evaluation takes no sparse part.
int InteriorPoint::evalTrial(double alpha, bool with_sparse, double eps, double *sq, TrialSums &t) {
  const bool batchable = prob->reductionsBatchable();
  const auto sparse_part = [&]() -> int {
    if (prob->evalSparseCon(xt, wtmp) != 0) return PO_ERR_USER;
    iterate_flags.trial_cw_valid = true;  // wtmp = cw(xt): handed to the iterate when this trial is accepted
    return k_w_trial(ctx, wv(), wp(), alpha * sx, eps, gsw->d, gtw->d, wtmp->d, nw, t.wsums);
  };
  {
    // the barrier sums at the trial point share the collective + host sync of the problem's own reductions
    // (f, c) when those go through the internal launchers (built-in problems)
    BatchScope batch(ctx, batchable);
    iterate_flags.trial_cw_valid = false;  // (xt is rewritten: wtmp is no longer cw(xt))
    PO_TRY(k_trial(ctx, bounds(), px->d, alpha * sx, eps, n, xt->d, t.sums, sq));
    s_qn_a = alpha * sx;
    iterate_flags.s_qn_from_trial = sq != nullptr;
    userBegin();
    t.fail_obj = prob->evalObjCon(xt, &fobj, cvals.data());
    userEnd();
    if (with_sparse && batchable && !t.fail_obj) PO_TRY(sparse_part());  // ... rides in the same collective
    PO_TRY(batch.end());
  }
  trial_logs[0] = t.sums[0];  // barrier sums at the point xt holds now
  trial_logs[1] = t.sums[1];
  iterate_flags.trial_logs_valid = true;
  neval++;
  if (with_sparse && !batchable && !t.fail_obj) PO_TRY(sparse_part());
  return PO_OK;
}

// The next trial step length (:4101-4130): half of alpha, or the minimiser of the quadratic through m0, dm0 and the
// merit at alpha (not below alpha / 100); neither below alpha_min, which sets *min_hit
static double nextTrialAlpha(double alpha, double alpha_min, double merit, double m0, double dm0, bool backtrack,
                             bool *min_hit) {
  const double alpha_new = backtrack ? 0.5 * alpha : -0.5 * dm0 * (alpha * alpha) / (merit - m0 - dm0 * alpha);
  *min_hit = alpha_new <= alpha_min;
  if (*min_hit) return alpha_min;
  if (!backtrack && alpha_new < 0.01 * alpha) return 0.01 * alpha;
  return alpha_new;
}

int InteriorPoint::lineSearch(double alpha_min, double *alpha_, double m0, double dm0,
                              int *fail_) {  // :3939-4156
  const int max_it = options.integer("max_line_iters");
  const bool backtrack = options.integer("use_backtracking_alpha");
  const double armijo = options.real("armijo_constant");
  const double fp = options.real("function_precision");
  const double eps = options.real("design_precision");
  double alpha = *alpha_;
  int fail = LS_FAILURE;
  // the quasi-Newton step s = alpha sx px of the trial point is written by the trial pass itself (the accepted
  // trial is the last one): no separate pass in computeStepAndUpdate
  double *sq = (qn && options.integer("use_quasi_newton_update")) ? s_qn->d : nullptr;
  double merit = 0.0, best_merit = 0.0, best_alpha = -1.0;
  std::vector<double> rs(c), rt(c);
  TrialSums t;
  int j = 0;
  for (; j < max_it; j++) {
    PO_TRY(evalTrial(alpha, has_w, eps, sq, t));
    if (t.fail_obj) {
      fprintf(stderr, "ParOpt: Evaluation failed during line search, trying new point\n");
      alpha *= 0.1;
      continue;
    }
    clampStepDense(rs, vars.s, alpha, step.s, eps, true);
    clampStepDense(rt, vars.t, alpha, step.t, eps, true);
    merit = evalMeritFromSums(fobj, cvals.data(), rs.data(), rt.data(), t.sums[0], t.sums[1],
                              has_w ? t.wsums : nullptr);
    if (best_alpha < 0.0 || merit < best_merit) {
      best_alpha = alpha;
      best_merit = merit;
    }
    if (merit - armijo * alpha * dm0 < (m0 + fp)) {
      fail = (fail & LS_MIN_STEP) ? (LS_SUCCESS | LS_MIN_STEP) : LS_SUCCESS;
      if ((merit <= m0 + fp) && (merit + fp >= m0)) fail |= LS_NO_IMPROVEMENT;
      break;
    } else if (fail & LS_MIN_STEP) {
      break;
    }
    if (j < max_it - 1) {
      bool min_hit = false;
      alpha = nextTrialAlpha(alpha, alpha_min, merit, m0, dm0, backtrack, &min_hit);
      if (min_hit) fail |= LS_MIN_STEP;
    }
  }
  if (j == max_it) fail |= LS_MAX_ITERS;
  if (!(fail & LS_SUCCESS)) {
    if (best_merit <= m0 + fp) {
      fail |= LS_SUCCESS;
      fail &= ~LS_FAILURE;
    } else if ((merit <= m0 + fp) && (merit + fp >= m0)) {
      fail |= LS_NO_IMPROVEMENT;
    }
    if (alpha != best_alpha) {  // xt is rebuilt at the best trial, without its sparse constraint values
      PO_TRY(evalTrial(best_alpha, false, eps, sq, t));
      if (t.fail_obj) {
        fprintf(stderr, "ParOpt: Evaluation failed during line search\n");
        fail = LS_FAILURE;
      }
    }
    alpha = best_alpha;
  }
  *alpha_ = alpha;
  *fail_ = fail;
  return PO_OK;
}

// The step of length alpha (:4169-4267) in five parts: the multipliers, the dense variables, the hand-over of the trial
// point, the gradient at the new point and the quasi-Newton update.  form_point: the line search did not form this
// point, so xt, f and c are taken here.
int InteriorPoint::computeStepAndUpdate(double alpha, bool form_point, int *update_type) {
  const double eps = options.real("design_precision");
  *update_type = 0;
  UpdatePlan plan;
  plan.do_qn = qn && options.integer("use_quasi_newton_update");
  PO_TRY(updateMultipliers(alpha, eps, plan));
  updateDenseVariables(alpha, eps);
  if (plan.do_qn && !plan.fast_yqn) {  // y_qn = -g + A^T z  at the old point with the new multipliers
    std::vector<const double *> A;
    for (Vec *a : Ac) A.push_back(a->d);
    PO_TRY(k_panel_axpy(ctx, y_qn->d, -1.0, g->d, 0.0, vars.z.data(), A.data(), c, n));
    if (has_w && prob->addSparseJacobianTranspose(1.0, x, wvar[0], y_qn) != 0) return PO_ERR_USER;
  }
  PO_TRY(acceptTrialPoint(alpha, form_point, eps));
  PO_TRY(evalGradientAtIterate());
  if (plan.do_qn) {
    PO_TRY(quasiNewtonUpdate(alpha, plan, update_type));
  } else if (qn) {  // :4261-4263
    if (qn->updateMult(x, vars.z.data(), has_w ? wvar[0] : nullptr) != 0) return PO_ERR_USER;
  }
  if (plan.fuse_upd_noqn) {
    spec_dt_want = true;  // (the barrier parameter of the next first solve: spec_dt_mu, set by optimize())
    const int rc = computeResidual(barrier_param, true, nullptr, &plan.upd);
    spec_dt_want = false;
    PO_TRY(rc);
    iterate_flags.residual_cached = true;
  }
  return PO_OK;
}

// The sparse and the bound multipliers step by alpha sz.  Decides, in `plan`, which pass carries the bound-multiplier
// step and the first bracket of y_qn, and launches what is not deferred to the residual pass of the new point; sets
// iterate_flags.acz_valid.
int InteriorPoint::updateMultipliers(double alpha, double eps, UpdatePlan &plan) {
  const bool do_qn = plan.do_qn;
  // The gradient difference y_qn = [-g + A^T z+]_old + [g - A^T z+]_new (:4197-4206, 4243-4251)
  // is assembled without streaming the constraint gradients: the first bracket from this
  // iteration's KKT residual rx = [lo]zl - [up]zu - g + A^T z and va = A^T pz (kept by the solves),
  // the second from the NEXT iteration's residual, which is evaluated right after the gradient and
  // reused at the top of the loop.
  // Sparse constraints (round 4): the same identity holds with A^T pz + Aw(x)^T pzw in place of A^T pz -- the first
  // bracket adds Aw(x_old)^T (zw+ - zw) = alpha sz Aw(x_old)^T pzw (:4207-4210 evaluate it at the OLD point), the second
  // is completed by the residual of the new point, whose panel carries Aw(x+)^T zw+ as one more column.  The sum is
  // formed here, from the final step, in one pass over the c constraint gradients: two panel passes, two sparse
  // transposes and the separate multiplier update disappear.  (Not with the linear-constraint recurrence, whose
  // `acz` follows the dense part of this vector alone.)
  const bool fast_w = has_w && do_qn && forms.analytic_panel_dots && !prob->linear_constraints;
  const bool fast_yqn = do_qn && forms.analytic_panel_dots && ((!has_w && step_flags.vA_valid) || fast_w);
  if (fast_w) {
    // vA <- sz Aw^T pzw + sum_j step.z[j] A_j   (step.z already carries sz: scaleKKTStep)
    std::vector<const double *> Aold;
    for (Vec *a : Ac) Aold.push_back(a->d);
    GroupCol gcol;  // (structured problems: the first term is formed by the pass itself)
    if (prob->sparseTransposeColumn(sz, x, wstepv[0], &gcol)) {
      PO_TRY(k_panel_axpy(ctx, vA->d, 0.0, nullptr, 1.0, step.z.data(), Aold.data(), c, n, &gcol));
    } else {
      if (prob->setSparseJacobianTranspose(sz, x, wstepv[0], vA) != 0) return PO_ERR_USER;
      if (c > 0) PO_TRY(k_panel_axpy(ctx, vA->d, 0.0, nullptr, 1.0, step.z.data(), Aold.data(), c, n));
    }
  }
  if (has_w) PO_TRY(k_w_update(ctx, wv(), wp(), alpha * sx, alpha * sz, eps, nw));  // :4177-4183
  // acz = A^T z follows z += alpha*sz*pz through va = A^T pz when the solves kept va; otherwise it is rebuilt
  const bool acz_follow = acz && iterate_flags.acz_valid && step_flags.vA_valid;
  // The bound-multiplier step and the first bracket of y_qn ride in the residual pass of the new point when that
  // pass follows anyway (kkt_res_update_kernel): nothing in between reads zl / zu.
  const bool fuse_upd = fast_yqn && forms.fuse_mult_update;
  // No quasi-Newton update (a fixed approximation: the trust-region subproblem solves): the multiplier step still
  // rides in the residual pass of the new point, which is then taken here, right after the gradient, instead of at
  // the top of the next iteration (round 4: one pass over the bound data and one launch less per inner iteration)
  const bool fuse_upd_noqn = !do_qn && forms.fuse_mult_update && !has_w && step_flags.pz_stored;
  if (!step_flags.pz_stored && !fuse_upd) {
    set_error("internal: lean step without the fused multiplier update");
    return PO_ERR_ARG;
  }
  MultUpdate &upd = plan.upd;
  upd.a = upd.az = alpha * sz;
  if (fast_w) upd.az = alpha;  // vA was built from the scaled step
  upd.eps = eps;
  upd.acz_follow = acz_follow;
  if (fuse_upd || fuse_upd_noqn) {
    // (deferred)
  } else if (fast_yqn) {
    PO_TRY(k_update_mult_yqn(ctx, zl->d, pzl->d, zu->d, pzu->d, alpha * sz, eps, use_lower, use_upper,
                             rx->d, vA->d, upd.az, n, y_qn->d, acz_follow ? acz->d : nullptr));
  } else {
    PO_TRY(k_update_mult(ctx, zl->d, pzl->d, zu->d, pzu->d, alpha * sz, eps, use_lower, use_upper, n));
    if (acz_follow) PO_TRY(k_axpy(ctx, acz->d, alpha * sz, vA->d, n));
  }
  if (!acz_follow) iterate_flags.acz_valid = false;
  plan.fast_yqn = fast_yqn;
  plan.fuse_upd = fuse_upd;
  plan.fuse_upd_noqn = fuse_upd_noqn;
  return PO_OK;
}

// the dense slacks and multipliers step by alpha (step.* carry sx / sz already: scaleKKTStep), clamped at eps
void InteriorPoint::updateDenseVariables(double alpha, double eps) {
  for (int i = 0; i < c; i++) {
    double v = vars.s[i] + alpha * step.s[i];
    vars.s[i] = (v <= eps) ? eps : v;
    v = vars.t[i] + alpha * step.t[i];
    vars.t[i] = (v <= eps) ? eps : v;
    vars.z[i] = vars.z[i] + alpha * step.z[i];
    v = vars.zs[i] + alpha * step.zs[i];
    vars.zs[i] = (v <= eps) ? eps : v;
    v = vars.zt[i] + alpha * step.zt[i];
    vars.zt[i] = (v <= eps) ? eps : v;
  }
}

// The trial point becomes the iterate: x <-> xt, with the sparse constraint values and the barrier sums the last trial
// left (iterate_flags.cwx_valid, iterate_logs_valid; the trial_* flags are consumed).  form_point: xt is formed here
// first and f, c are evaluated at the new x (neval).
int InteriorPoint::acceptTrialPoint(double alpha, bool form_point, double eps) {
  if (form_point) {
    double sums[2];
    PO_TRY(k_trial(ctx, bounds(), px->d, alpha * sx, eps, n, xt->d, sums));  // (not in a batch: sums is local)
    iterate_flags.s_qn_from_trial = false;
    trial_logs[0] = sums[0];
    trial_logs[1] = sums[1];
    iterate_flags.trial_logs_valid = true;
  }
  // the accepted trial point IS the new design point (same clamp, same arithmetic)
  std::swap(x->d, xt->d);
  // ... and so are its sparse constraint values when the line search's last trial left them in wtmp
  iterate_flags.cwx_valid = false;
  if (has_w && iterate_flags.trial_cw_valid && !form_point) {
    std::swap(cwx->d, wtmp->d);
    iterate_flags.cwx_valid = true;
  }
  iterate_flags.trial_cw_valid = false;
  // ... and its barrier sums are those of the new iterate (trial_kernel and the merit pass take them alike)
  iterate_logs[0] = trial_logs[0];
  iterate_logs[1] = trial_logs[1];
  iterate_flags.iterate_logs_valid = iterate_flags.trial_logs_valid;
  iterate_flags.trial_logs_valid = false;
  if (form_point) {
    userBegin();
    int fail = prob->evalObjCon(x, &fobj, cvals.data());
    userEnd();
    neval++;
    if (fail) {
      fprintf(stderr, "ParOpt: Function and constraint evaluation failed\n");
      return PO_ERR_USER;
    }
  }
  return PO_OK;
}

// g and the Jacobian at the new iterate (ngeval); a failure is reported and the run goes on, as in the reference
int InteriorPoint::evalGradientAtIterate() {
  // a problem with linear dense constraints keeps the Jacobian of the first evaluation (Ac == nullptr)
  userBegin();
  // (constantJacobianMask: the library's own model problems may declare single columns constant; those are kept)
  std::vector<Vec *> Acp(Ac);
  const std::vector<char> *cmask = iterate_flags.ac_valid ? prob->constantJacobianMask() : nullptr;
  for (int i = 0; cmask && i < c && i < (int)cmask->size(); i++)
    if ((*cmask)[i]) Acp[i] = nullptr;
  int fail_g =
      prob->evalObjConGradient(x, g, (prob->linear_constraints && iterate_flags.ac_valid) ? nullptr : Acp.data());
  userEnd();
  ngeval++;
  if (fail_g) fprintf(stderr, "ParOpt: Gradient evaluation failed at final line search\n");
  return PO_OK;
}

// s_qn (unless the last trial pass wrote it), the second bracket of y_qn, the problem's correction and the update of the
// approximation.  Where the plan allows, the residual of the NEXT iteration is taken here, in the batch of the update's
// products (iterate_flags.residual_cached).
int InteriorPoint::quasiNewtonUpdate(double alpha, const UpdatePlan &plan, int *update_type) {
  if (!(iterate_flags.s_qn_from_trial && s_qn_a == alpha * sx)) {
    PO_TRY(k_panel_axpy(ctx, s_qn->d, alpha * sx, px->d, 0.0, nullptr, nullptr, 0, n));
  }
  iterate_flags.s_qn_from_trial = false;
  // the next residual's norms and the quasi-Newton products of the update are reduced together: nothing on the
  // host needs the norms before the update has its dots.  Only when no user code runs in between.
  // (user code between the two: only computeQuasiNewtonUpdateCorrection, and only when the problem has one)
  // (sparse constraints: y_qn is assembled by its own passes, the residual of the next iteration is still taken
  // here, early, so that its norms ride with the products of the update -- built-in problems only: their sparse
  // callbacks queue nothing that is read before the flush)
  const bool early_w = has_w && !plan.fast_yqn && prob->reductionsBatchable();
  BatchScope batch(ctx, (plan.fast_yqn || early_w) && qn->reductionsBatchable() &&
                            (prob->reductionsBatchable() || !prob->quasiNewtonCorrectionMayChangeStep()));
  if (plan.fast_yqn) {
    // residual of the next iteration at (x+, z+, zl+, zu+): rx+ = [lo]zl+ - [up]zu+ - g+ + A+^T z+
    // ... and y_qn += [lo]zl+ - [up]zu+ - rx+ in the same pass (the residual kernel has all three in registers)
    // (sequential linear method: the quasi-Newton update that follows does not enter the next KKT diagonal, so this
    // pass can leave Dinv and t of the next first solve behind as the pass without an update does -- spec_dt_*)
    spec_dt_want = plan.fuse_upd && options.integer("sequential_linear_method") != 0;
    const int rcr = computeResidual(barrier_param, true, y_qn, plan.fuse_upd ? &plan.upd : nullptr);
    spec_dt_want = false;
    PO_TRY(rcr);
    iterate_flags.residual_cached = true;
  } else {
    std::vector<const double *> A;
    for (Vec *a : Ac) A.push_back(a->d);
    std::vector<double> mz(c > 0 ? c : 1);
    for (int i = 0; i < c; i++) mz[i] = -vars.z[i];
    PO_TRY(k_panel_axpy(ctx, y_qn->d, 1.0, g->d, 1.0, mz.data(), A.data(), c, n));
    if (has_w && prob->addSparseJacobianTranspose(-1.0, x, wvar[0], y_qn) != 0) return PO_ERR_USER;
    if (early_w) {
      PO_TRY(computeResidual(barrier_param, true));
      iterate_flags.residual_cached = true;
    }
  }
  int rcc = prob->computeQuasiNewtonUpdateCorrection(x, vars.z.data(), s_qn, y_qn);
  if (rcc != 0) return PO_ERR_USER;
  // Z^T s = alpha sx Z^T px is known from the solves (ptpx) when the step came from this very panel
  const int kz = qn->size();
  std::vector<double> zts;
  if (forms.analytic_panel_dots && step_flags.ptpx_valid && kz == kkt.k && kz > 0 && (int)ptpx.size() == c + kz &&
      !inexact_newton_step && !prob->quasiNewtonCorrectionMayChangeStep()) {
    zts.resize(kz);
    for (int j = 0; j < kz; j++) zts[j] = alpha * sx * ptpx[c + j];
  }
  qn->take_buffers = true;  // s_qn / y_qn are rewritten from scratch before their next use
  const int urc = qn->updateAt(x, vars.z.data(), has_w ? wvar[0] : nullptr, s_qn, y_qn,
                               zts.empty() ? nullptr : zts.data(), update_type);
  qn->take_buffers = false;
  PO_TRY(urc);
  return batch.end();
}

// ================================================================================================
// optimize
// ================================================================================================
void InteriorPoint::getOptimizedPoint(Vec **x_, const double **z_, Vec **zl_, Vec **zu_) {
  if (x_) *x_ = x;
  if (z_) *z_ = vars.z.data();
  if (zl_) *zl_ = use_lower ? zl : nullptr;
  if (zu_) *zu_ = use_upper ? zu : nullptr;
}
void InteriorPoint::getOptimizedSlacks(const double **s_, const double **t_, const double **zs_,
                                       const double **zt_) {
  if (s_) *s_ = vars.s.data();
  if (t_) *t_ = vars.t.data();
  if (zs_) *zs_ = vars.zs.data();
  if (zt_) *zt_ = vars.zt.data();
}
void InteriorPoint::getIterationCounters(int *a, int *b, int *d) {
  if (a) *a = niter;
  if (b) *b = neval;
  if (d) *d = ngeval;
}

// ---- the stages of optimize(), in the order it calls them ----

// Host mirrors a caller obtained for the solver's vectors (getOptimizedPoint + getArray) are the vectors' data
// while they are live (the reference's pointers ARE the data, src/ParOptVec.cpp:212-217): what the caller wrote
// through them -- e.g. warm-start multipliers zl / zu for starting_point_strategy = no_start_strategy -- is
// uploaded before the first kernel reads it, as po_vec_release_array(v, 1) would.  The mirrors stop being live
// here (the kernels below do not look at mirrors): views handed out earlier go stale during the solve and are
// refreshed by the next getArray.
int InteriorPoint::uploadLiveMirrors() {
  Vec *mine[] = {x, zl, zu, wvar[0], wvar[1], wvar[2], wvar[3], wvar[4]};
  bool any = false;
  for (Vec *v : mine) {
    any = any || vec_mirror_live(v);
    PO_TRY(vec_mirror_upload(v));
    if (v) v->h_live = 0;
  }
  if (any) PO_HIP(hipStreamSynchronize(ctx->stream));  // the pinned mirrors may be rewritten by the caller at once
  return PO_OK;
}

InteriorPoint::RunOptions InteriorPoint::readRunOptions() const {
  RunOptions o;
  o.abs_res_tol = options.real("abs_res_tol");
  o.rel_func_tol = options.real("rel_func_tol");
  o.function_precision = options.real("function_precision");
  o.design_precision = options.real("design_precision");
  const std::string bname = options.str("barrier_strategy");
  o.barrier_strategy = bname == "monotone" ? Barrier::MONOTONE
                       : bname == "mehrotra" ? Barrier::MEHROTRA
                       : bname == "mehrotra_predictor_corrector" ? Barrier::MPC : Barrier::COMP_FRACTION;
  o.use_hvec_product = options.integer("use_hvec_product");
  o.use_diag_hessian = options.integer("use_diag_hessian");
  o.max_major_iters = options.integer("max_major_iters");
  o.use_quasi_newton_update = options.integer("use_quasi_newton_update");
  o.hessian_reset_freq = options.integer("hessian_reset_freq");
  o.sequential_linear_method = options.integer("sequential_linear_method");
  o.min_fraction_to_boundary = options.real("min_fraction_to_boundary");
  o.use_line_search = options.integer("use_line_search");
  o.write_output_frequency = options.integer("write_output_frequency");
  o.step_verification_frequency = options.integer("step_verification_frequency");
  o.gradient_verification_frequency = options.integer("gradient_verification_frequency");
  o.starting_point_strategy = options.str("starting_point_strategy");
  return o;
}

// Start of a run: the norm, the initial barrier and penalty parameters, the second-order work vectors, every counter
// and carried flag back to its start, then the "init" phase -- bounds, f, c, g, A at the starting point (neval,
// ngeval, iterate_flags.ac_valid) and the starting multipliers.  Returns what the reference returns: 1 without any
// Hessian approximation, the callback's code for a failed first evaluation.
int InteriorPoint::startRun(const RunOptions &opt) {
  {
    const std::string nt = options.str("norm_type");
    norm_type = nt == "infinity" ? 0 : (nt == "l1" ? 1 : 2);
  }
  corrector_active = false;
  if (has_w && opt.use_hvec_product) {
    for (int i = 0; i < 5; i++) {
      if (!wscalev[i]) wscalev[i] = vec_new(ctx, nw);
      if (!wscalev[i]) return PO_ERR_HIP;
    }
  }
  if (opt.use_diag_hessian) PO_TRY(ensureHdiag());
  inexact_newton_step = false;
  barrier_param = options.real("init_barrier_param");
  rho_penalty_search = options.real("init_rho_penalty_search");
  niter = neval = ngeval = nhvec = 0;
  hvec_fd_products = hvec_fd_evals = 0;
  stateReplaced();
  spec_dt_want = false;
  spec_enabled = false;
  history.clear();
  phase_names.clear();
  phase_seconds.clear();
  user_seconds = 0.0;
  user_pending = 0;
  if (!opt.sequential_linear_method && !qn && !opt.use_diag_hessian) {
    if (ctx->rank == 0)
      fprintf(stderr,
              "ParOpt Error: Must use a sequential linear method if no quasi-Newton approximation "
              "is defined\n");
    return 1;
  }
  phaseBegin();
  PO_TRY(initAndCheckDesignAndBounds());
  userBegin();
  int fail_obj = prob->evalObjCon(x, &fobj, cvals.data());
  userEnd();
  neval++;
  if (fail_obj) {
    fprintf(stderr, "ParOpt: Initial function and constraint evaluation failed\n");
    return fail_obj;
  }
  userBegin();
  int fail_g = prob->evalObjConGradient(x, g, Ac.data());
  userEnd();
  ngeval++;
  if (fail_g) {
    fprintf(stderr, "ParOpt: Initial gradient evaluation failed\n");
    return fail_g;
  }
  iterate_flags.ac_valid = true;
  if (opt.starting_point_strategy == "affine_step") {
    PO_TRY(initAffineStepMultipliers());
  } else if (opt.starting_point_strategy == "least_squares_multipliers") {
    PO_TRY(initLeastSquaresMultipliers());
  }
  if (qn && !opt.use_quasi_newton_update) {  // :4569-4573
    if (qn->updateMult(x, vars.z.data(), has_w ? wvar[0] : nullptr) != 0) return PO_ERR_USER;
  }
  phaseEnd("init");
  return PO_OK;
}

// The periodic work at the head of iteration k, in this order: the Hessian reset (qn_hessian_reset), the checkpoint and
// the problem's writeOutput, the iteration callback, the gradient check.  A checkpoint that cannot be written is not
// tried again (*checkpoint).
int InteriorPoint::iterationHead(const RunOptions &opt, int k, const char **checkpoint, IterRecord &it) {
  if (qn && !opt.sequential_linear_method && k > 0 && k % opt.hessian_reset_freq == 0 &&
      opt.use_quasi_newton_update) {
    resetQuasiNewton(it);
  }
  if (opt.write_output_frequency > 0 && k % opt.write_output_frequency == 0) {
    if (*checkpoint) {
      if (writeSolutionFile(*checkpoint) != PO_OK) *checkpoint = nullptr;
    }
    prob->writeOutput(k, x);
  }
  if (iter_cb) iter_cb(iter_cb_user, k);
  // gradient_verification_frequency (:4522-4525, 4635-4639): finite-difference check of the user's gradients
  if (opt.gradient_verification_frequency > 0 && (k % opt.gradient_verification_frequency) == 0) {
    std::string rep;
    PO_TRY(checkGradients(options.real("gradient_check_step_length"), &rep));
    if (ctx->rank == 0) history += rep;
  }
  return PO_OK;
}

void InteriorPoint::resetQuasiNewton(IterRecord &it) {
  qn->reset();
  it.qn_hessian_reset = true;
}

// the dense part of the residual for `mu` (in res) and the four norms of the whole residual, as the last
// computeResidual left its vector part
void InteriorPoint::residualNorms(double mu, IterRecord &it) {
  denseResidual(mu, res);
  resNorms(res, &it.max_prime, &it.max_dual, &it.max_infeas, &it.res_norm);
}

// Complementarity + KKT residual + norms in ONE pass (:4656-4671), unless the last step update took it already, and
// the barrier parameter of this iteration by the strategy in force (:4673-4762).  Owns barrier_param, the restart of
// rho_penalty_search at a monotone reduction, spec_enabled, st.line_search_test, and sets it.rel_function_test,
// it.comp, the four norms and it.monotone_barrier_converged.
int InteriorPoint::updateBarrierAndNorms(const RunOptions &opt, int k, MajorState &st, IterRecord &it) {
  it.rel_function_test = (st.alpha_xprev == 1.0 && st.alpha_zprev == 1.0 &&
                          (fabs(fobj - st.fobj_prev) < opt.rel_func_tol * fabs(st.fobj_prev)));
  if (st.no_merit_function_improvement) {
    st.line_search_test += 1;
  } else {
    st.line_search_test = 0;
  }
  // (the inexact Newton step reads the 2-norms of the bound residuals, computeKKTGMRESStep: no shortcut there)
  spec_enabled = st.barrier_strategy == Barrier::MONOTONE && norm_type == 0 && !has_w && !opt.use_hvec_product;
  if (!iterate_flags.residual_cached) PO_TRY(computeResidual(barrier_param, true));
  iterate_flags.residual_cached = false;
  it.comp = compFromSums(comp_prod, comp_count, vars, w_sums[0]);
  if (st.barrier_strategy == Barrier::COMP_FRACTION) {  // :4747-4762
    barrier_param = options.real("monotone_barrier_fraction") * it.comp;
    if (barrier_param < 0.1 * opt.abs_res_tol) barrier_param = 0.1 * opt.abs_res_tol;
    PO_TRY(computeResidual(barrier_param, false));
  }
  residualNorms(barrier_param, it);
  if (st.barrier_strategy == Barrier::MONOTONE && k > 0 &&
      ((it.res_norm < 10.0 * barrier_param) || it.rel_function_test || (st.line_search_test >= 2))) {
    it.monotone_barrier_converged = true;
    if (barrier_param > 0.1 * opt.abs_res_tol) st.line_search_test = 0;
    const double new_mu = nextMonotoneMu();
    if (iterate_flags.spec_valid && spec_mu == new_mu && norm_type == 0) {
      // the residual pass of this iterate took the two maxima for new_mu as well (the complementarity product
      // and the bound count do not depend on mu): what computeResidual(new_mu, false) would produce
      max_rzl = spec_max[0];
      max_rzu = spec_max[1];
      iterate_flags.spec_valid = false;
    } else {
      PO_TRY(computeResidual(new_mu, false));  // rx does not depend on mu
    }
    residualNorms(new_mu, it);
    rho_penalty_search = options.real("min_rho_penalty_search");
    barrier_param = new_mu;
  }
  phaseEnd("residual");
  return PO_OK;
}

// the row of iteration k in the table (:4777-4801), with the header every ten rows and the problem's factor report
void InteriorPoint::appendTableRow(int k, const MajorState &st, const IterRecord &it) {
  if (ctx->rank != 0) return;
  char line[512];
  if (k == 0 || options.integer("output_level") > 0) {  // :4767-4774
    const char *inform = prob->sparseFactorInfo();
    if (inform) history += std::string("MatInfo: ") + inform + "\n";
  }
  if (k % 10 == 0) {
    snprintf(line, sizeof(line),
             "\n%4s %4s %4s %4s %7s %7s %7s %12s %7s %7s %7s %7s %7s %8s %7s info\n", "iter",
             "nobj", "ngrd", "nhvc", "alpha", "alphx", "alphz", "fobj", "|opt|", "|infes|",
             "|dual|", "mu", "comp", "dmerit", "rho");
    history += line;
  }
  if (k == 0) {
    snprintf(line, sizeof(line),
             "%4d %4d %4d %4d %7s %7s %7s %12.5e %7.1e %7.1e %7.1e %7.1e %7.1e %8s %7s %s\n", k,
             neval, ngeval, nhvec, "--", "--", "--", fobj, it.max_prime, it.max_infeas, it.max_dual,
             barrier_param, it.comp, "--", "--", st.info.c_str());
  } else {
    snprintf(line, sizeof(line),
             "%4d %4d %4d %4d %7.1e %7.1e %7.1e %12.5e %7.1e %7.1e %7.1e %7.1e %7.1e %8.1e %7.1e %s\n",
             k, neval, ngeval, nhvec, st.alpha_prev, st.alpha_xprev, st.alpha_zprev, fobj, it.max_prime,
             it.max_infeas, it.max_dual, barrier_param, it.comp, st.dm0_prev, rho_penalty_search, st.info.c_str());
  }
  history += line;
}

// true when the run ends at iteration k (:4803-4818); the reason goes into the history
bool InteriorPoint::stopTest(const RunOptions &opt, int k, const MajorState &st, const IterRecord &it) {
  if (!(k > 0 && (barrier_param <= 0.1 * opt.abs_res_tol) &&
        (it.res_norm < opt.abs_res_tol || it.rel_function_test || (st.line_search_test >= 2)))) {
    return false;
  }
  if (ctx->rank == 0) {
    if (it.rel_function_test) {
      history += "\nParOpt: Successfully converged on relative function test\n";
    } else if (st.line_search_test >= 2) {
      history +=
          "\nParOpt Warning: Current design point could not be improved. No barrier function "
          "decrease in previous two iterations\n";
    } else {
      history += "\nParOpt: Successfully converged to requested tolerance\n";
    }
  }
  return true;
}

// Inexact Newton-Krylov step with exact Hessian-vector products (:4853-4900), tried once the three norms are below
// nk_switch_tol and the Eisenstat-Walker tolerance below max_gmres_rtol.  Owns inexact_newton_step (true: the step is
// in px, pzl, pzu, step) and it.gmres_iters (negative: no descent direction, the quasi-Newton step follows).
int InteriorPoint::newtonKrylovAttempt(const RunOptions &opt, const MajorState &st, IterRecord &it) {
  inexact_newton_step = false;
  if (!opt.use_hvec_product) return PO_OK;
  const double gmres_rtol =
      st.res_norm_prev == 0.0 ? 1e300
                              : options.real("eisenstat_walker_gamma") *
                                    pow(it.res_norm / st.res_norm_prev, options.real("eisenstat_walker_alpha"));
  const double nk = options.real("nk_switch_tol");
  if (it.max_prime < nk && it.max_dual < nk && it.max_infeas < nk && gmres_rtol < options.real("max_gmres_rtol")) {
    const bool precon_qn = !(opt.sequential_linear_method || !options.integer("use_qn_gmres_precon"));
    PO_TRY(setUpKKTSystem(precon_qn));
    PO_TRY(computeKKTGMRESStep(gmres_rtol, options.real("gmres_atol"), precon_qn, it.tau, &it.gmres_iters));
    phaseEnd("gmres_step");
    // negative: GMRES did not produce a descent direction (:4883-4894), fall back to the quasi-Newton step
    if (it.gmres_iters > 0) inexact_newton_step = true;
  }
  return PO_OK;
}

// The kind of step this iteration takes (:4920-4949); the diagonal Hessian is evaluated here when that is the kind.
int InteriorPoint::chooseStepKind(const RunOptions &opt, const MajorState &st, IterRecord &it) {
  const bool seq_lin = opt.sequential_linear_method;
  if (inexact_newton_step) {
    it.kind = StepKind::INEXACT_NEWTON;  // the step is already in place
  } else if (!seq_lin && st.line_search_failed && !opt.use_quasi_newton_update) {
    // a fixed quasi-Newton approximation whose line search failed (:4923-4939): sequential linear
    // step, or only the diagonal b0 of the approximation when that is positive
    it.kind = (qn && qn->diag() > 0.0) ? StepKind::DIAG_QUASI_NEWTON : StepKind::SEQ_LINEAR;
  } else if (opt.use_diag_hessian && !seq_lin) {  // :4940-4948
    // (an else-if chain in the reference, :4920-4949: under the sequential linear method the diagonal is never
    // evaluated -- hdiag keeps its initial zeros, which setUpKKTDiagSystem and addKKTResStep then use)
    it.kind = StepKind::DIAG_HESSIAN;
    if (prob->evalHessianDiag(x, vars.z.data(), has_w ? wvar[0] : nullptr, hdiag) != 0) {
      fprintf(stderr, "ParOpt: Hessian diagonal evaluation failed\n");
      return PO_ERR_USER;
    }
  } else {
    it.kind = seq_lin ? StepKind::SEQ_LINEAR : StepKind::QUASI_NEWTON;
  }
  return PO_OK;
}

// The step of the chosen kind (an inexact Newton step is in place already), the step check, and the step lengths:
// it.tau (Mehrotra's rule replaces it), it.alpha_x, it.alpha_z, it.ceq_step; lean_step_allowed around the solve.
int InteriorPoint::computeStep(const RunOptions &opt, int k, const MajorState &st, IterRecord &it) {
  if (it.kind != StepKind::INEXACT_NEWTON) {
    const bool use_qn = it.kind == StepKind::QUASI_NEWTON;
    const double rhs_mu = mehrotra(st) ? 0.0 : barrier_param;  // of the solve that follows
    PO_TRY(setUpKKTSystem(use_qn, it.kind == StepKind::DIAG_QUASI_NEWTON, &rhs_mu));
    phaseEnd("setup_kkt");
    if (!mehrotra(st)) {
      // every consumer of (pzl, pzu) after this solve is the fused multiplier update of computeStepAndUpdate
      lean_step_allowed = qn && opt.use_quasi_newton_update && use_qn && forms.analytic_panel_dots &&
                          forms.fuse_mult_update && !opt.use_hvec_product && !opt.use_diag_hessian;
      const int step_rc = computeKKTStepWithRefinement(barrier_param, use_qn, it.tau);
      lean_step_allowed = false;
      PO_TRY(step_rc);
    } else {
      PO_TRY(mehrotraStep(use_qn, it.comp, st.barrier_strategy == Barrier::MPC, opt.min_fraction_to_boundary,
                          opt.abs_res_tol, &it.tau));
    }
  }
  phaseEnd("kkt_step");
  // step_verification_frequency (:5056-5073): block maxima of the linearised KKT residual at the step
  if (opt.step_verification_frequency > 0 && (k % opt.step_verification_frequency) == 0 && !inexact_newton_step) {
    if (st.barrier_strategy == Barrier::MPC && ctx->rank == 0)
      history += "Note: the step check is inconsistent with the predictor-corrector step (corrector terms)\n";
    PO_TRY(checkKKTStep(k, barrier_param));
  }
  PO_TRY(scaleKKTStep(it.tau, it.comp, &it.alpha_x, &it.alpha_z, &it.ceq_step, inexact_newton_step));
  phaseEnd("scale_step");
  return PO_OK;
}

// merit function and its derivative along the scaled step; the derivative is what the next table row prints
int InteriorPoint::meritDerivative(MajorState &st, const IterRecord &it, double *m0, double *dm0) {
  PO_TRY(evalMeritInitDeriv(it.alpha_x, m0, dm0));
  st.dm0_prev = *dm0;
  return PO_OK;
}

// Globalisation, first form: the merit derivative is inside the function precision, the full step is taken without a
// line search (line_search_skipped; line_fail says whether the objective moved).
int InteriorPoint::stepWithLineSearchSkipped(const RunOptions &opt, const MajorState &st, IterRecord &it) {
  const double fprec = opt.function_precision;
  it.line_search_skipped = true;
  PO_TRY(computeStepAndUpdate(it.alpha, true, &it.update_type));
  phaseEnd("step_update");
  if ((st.fobj_prev + fprec <= fobj) && (fobj + fprec <= st.fobj_prev)) it.line_fail = LS_NO_IMPROVEMENT;
  return PO_OK;
}

// The step is no descent direction of the merit function (:5130-5173): the quasi-Newton approximation is reset and the
// step, its lengths and the merit derivative are taken again (qn_hessian_reset, retried_after_reset, the norms).
int InteriorPoint::retryAfterReset(MajorState &st, IterRecord &it, double *m0, double *dm0) {
  if (qn) resetQuasiNewton(it);
  it.retried_after_reset = true;
  PO_TRY(computeResidual(barrier_param, true));
  residualNorms(barrier_param, it);
  PO_TRY(setUpKKTSystem(true, false, &barrier_param));
  PO_TRY(computeKKTStepWithRefinement(barrier_param, true, it.tau));
  PO_TRY(scaleKKTStep(it.tau, it.comp, &it.alpha_x, &it.alpha_z, &it.ceq_step));
  PO_TRY(meritDerivative(st, it, m0, dm0));
  phaseEnd("qn_reset_step");
  return PO_OK;
}

// Globalisation, second form: the line search, after retryAfterReset where the step is no descent direction, and the
// step update unless the search failed (it.alpha, it.line_fail, it.update_type).
int InteriorPoint::stepByLineSearch(const RunOptions &opt, MajorState &st, IterRecord &it, double m0, double dm0) {
  if (dm0 >= 0.0) PO_TRY(retryAfterReset(st, it, &m0, &dm0));
  if (dm0 >= 0.0) {
    it.line_fail = LS_FAILURE;
    return PO_OK;
  }
  double px_norm = 0.0;
  if (step_flags.merit_cache_valid) {
    px_norm = merit_cache.px_amax;
  } else if (step_flags.px_amax_valid) {
    px_norm = px_amax_w;
  } else {
    PO_TRY(k_reduce1(ctx, RED_AMAX, px->d, nullptr, n, &px_norm));
  }
  px_norm *= fabs(sx);
  double alpha_min = 1.0;
  if (px_norm != 0.0) alpha_min = opt.function_precision / px_norm;
  if (alpha_min > 0.5) alpha_min = 0.5;
  PO_TRY(lineSearch(alpha_min, &it.alpha, m0, dm0, &it.line_fail));
  phaseEnd("line_search");
  if (px_norm < opt.design_precision) it.line_fail |= LS_SHORT_STEP;
  if (!(it.line_fail & LS_FAILURE)) {
    PO_TRY(computeStepAndUpdate(it.alpha, false, &it.update_type));
    phaseEnd("step_update");
  }
  return PO_OK;
}

// Globalisation, third form (use_line_search = 0): the full step, then the merit function at the new point to say
// whether it improved (it.line_fail).
int InteriorPoint::stepWithoutLineSearch(const RunOptions &opt, IterRecord &it, double m0, double dm0) {
  const double fprec = opt.function_precision;
  it.line_fail = LS_SUCCESS;
  PO_TRY(computeStepAndUpdate(it.alpha, true, &it.update_type));
  // merit at the new point (:5236-5237): barrier sums of x itself (a zero step from x)
  double bs[2];
  PO_TRY(k_trial(ctx, bounds(), px->d, 0.0, opt.design_precision, n, xt->d, bs));
  double wsums[5];
  if (has_w) {
    const double *cw = nullptr;
    PO_TRY(sparseConAtIterate(&cw));
    PO_TRY(k_w_trial(ctx, wv(), wp(), 0.0, opt.design_precision, gsw->d, gtw->d, cw, nw, wsums));
  }
  const double m1 = evalMeritFromSums(fobj, cvals.data(), vars.s.data(), vars.t.data(), bs[0], bs[1],
                                      has_w ? wsums : nullptr);
  if ((m1 <= m0 + fprec) && (m1 + fprec >= m0)) {
    it.line_fail |= LS_NO_IMPROVEMENT;
  } else if (fabs(dm0) <= fprec) {
    it.line_fail = LS_NO_IMPROVEMENT;
  }
  phaseEnd("step_update");
  return PO_OK;
}

// What the next iteration inherits: the merit-improvement and line-search flags, the step lengths, the reset of the
// approximation after a failed line search (qn_hessian_reset), the info column (:5272-5322) and, at the first monotone
// reduction of the barrier parameter, the strategy of the input.
void InteriorPoint::closeIteration(const RunOptions &opt, MajorState &st, IterRecord &it) {
  st.no_merit_function_improvement =
      ((it.line_fail & LS_NO_IMPROVEMENT) || (it.line_fail & LS_MIN_STEP) ||
       (it.line_fail & LS_SHORT_STEP) || (it.line_fail & LS_FAILURE));
  st.line_search_failed = (it.line_fail & LS_FAILURE) ? 1 : 0;
  st.alpha_prev = it.alpha;
  st.alpha_xprev = it.alpha_x;
  st.alpha_zprev = it.alpha_z;
  if (qn && opt.use_quasi_newton_update && (it.line_fail & LS_FAILURE)) resetQuasiNewton(it);
  std::string &s = st.info;
  s.clear();
  if (it.gmres_iters != 0) s += "iNK" + std::to_string(it.gmres_iters) + " ";
  if (it.update_type == 1) s += "dampH ";
  else if (it.update_type == 2) s += "skipH ";
  if (it.qn_hessian_reset) s += "resetH ";
  if (it.line_fail & LS_FAILURE) s += "LFail ";
  if (it.line_fail & LS_MIN_STEP) s += "LMnStp ";
  if (it.line_fail & LS_MAX_ITERS) s += "LMxItr ";
  if (it.line_fail & LS_NO_IMPROVEMENT) s += "LNoImprv ";
  // (SLP marks the fall-back of a fixed approximation, not the method the options chose)
  if (it.kind == StepKind::SEQ_LINEAR && !opt.sequential_linear_method) s += "SLP ";
  if (it.kind == StepKind::DIAG_QUASI_NEWTON || it.retried_after_reset) s += "DQN ";
  if (it.line_search_skipped) s += "LSkip ";
  if (it.ceq_step) s += "cmpEq ";
  if (s.size() > 63) s.resize(63);  // the column is 63 characters wide
  if (it.monotone_barrier_converged) st.barrier_strategy = opt.barrier_strategy;
}

int InteriorPoint::optimize(const char *checkpoint) {
  PO_TRY(uploadLiveMirrors());
  PO_TRY(createQuasiNewton());
  PO_TRY(refreshQuasiNewton());
  const RunOptions opt = readRunOptions();
  PO_TRY(startRun(opt));
  MajorState st;
  for (int k = 0; k < opt.max_major_iters; k++, niter++) {
    IterRecord it;
    PO_TRY(iterationHead(opt, k, &checkpoint, it));
    PO_TRY(updateBarrierAndNorms(opt, k, st, it));
    appendTableRow(k, st, it);
    if (stopTest(opt, k, st, it)) break;
    // (what the first solve of the NEXT iteration will most likely take as its barrier parameter: see spec_dt_valid)
    spec_dt_mu = mehrotra(st) ? 0.0 : barrier_param;
    it.tau = fractionToBoundary(barrier_param, opt.min_fraction_to_boundary);
    PO_TRY(newtonKrylovAttempt(opt, st, it));
    st.fobj_prev = fobj;
    st.res_norm_prev = it.res_norm;
    PO_TRY(chooseStepKind(opt, st, it));
    PO_TRY(computeStep(opt, k, st, it));
    double m0 = 0.0, dm0 = 0.0;
    PO_TRY(meritDerivative(st, it, &m0, &dm0));
    if (!opt.use_line_search) {
      PO_TRY(stepWithoutLineSearch(opt, it, m0, dm0));
    } else {
      phaseEnd("merit_deriv");
      if (dm0 >= 0.0 && dm0 <= opt.function_precision) {
        PO_TRY(stepWithLineSearchSkipped(opt, st, it));
      } else {
        PO_TRY(stepByLineSearch(opt, st, it, m0, dm0));
      }
    }
    closeIteration(opt, st, it);
  }
  flushHistory();
  return 0;
}

// The reference streams the iteration table to `output_file` on the root rank (setOutputFile
// :1297-1309, :4777-4805); here it is accumulated in `history` and written when optimize returns.
void InteriorPoint::flushHistory() {
  userHarvest();
  phase_names.push_back("user_eval");
  phase_seconds.push_back(user_seconds);
  const std::string fname = options.str("output_file");
  // debugging aid: PAROPT_AMD_DUMP_LONG_SOLVES=<N> prints the head and tail of the iteration table of
  // every solve that took at least N major iterations (e.g. a stalled trust-region subproblem)
  if (ctx->rank == 0) {
    const int dump_from = dbg_switch(SW_DUMP_LONG_SOLVES);
    if (dump_from >= 0 && niter >= dump_from) {
      const size_t len = history.size();
      fprintf(stderr, "---- paropt_amd: solve with %d iterations ----\n%s\n   [...]\n%s\n", niter,
              history.substr(0, std::min<size_t>(len, 6000)).c_str(),
              history.substr(len > 4000 ? len - 4000 : 0).c_str());
    }
  }
  write_history_file(ctx, fname, "ParOptInteriorPoint", history);
}
void write_history_file(Ctx *ctx, const std::string &fname, const char *solver, const std::string &history) {
  if (ctx->rank != 0 || fname.empty()) return;
  FILE *fp = fopen(fname.c_str(), "w");
  if (!fp) return;
  fprintf(fp, "%s (paropt_amd, MI355X)\n", solver);
  fputs(history.c_str(), fp);
  fclose(fp);
}

// writeSolutionFile (:883-972): ONE file in the reference's layout whatever the number of ranks -
//   int32 {total nvars, total nwcon, ncon}, mu, s, t, z, zs, zt (ncon each, written by rank 0), then x, zl, zu
//   as global arrays (each rank writes its block at its offset, as MPI_File_write_at_all does there), then zw
//   and sw likewise when there are sparse constraints.
// A file written by N ranks is byte-for-byte the file of the concatenated problem and can be read by any
// number of ranks (shared file system, like MPI-IO).
int InteriorPoint::gatherCounts(int64_t mine, std::vector<int64_t> *all) {
  // all[r] = the count of rank r, through the one collective the context has: a dot product of the
  // 1-vector [mine] with unit vectors that are 1 only on their own rank
  all->assign(ctx->size, mine);
  if (ctx->size == 1) return PO_OK;
  if (ctx->size > kMaxPanel) {
    set_error("solution files support at most %d ranks", kMaxPanel);
    return PO_ERR_ARG;
  }
  Vec *v = vec_new(ctx, 1), *one = vec_new(ctx, 1), *zero = vec_new(ctx, 1);
  if (!v || !one || !zero) return PO_ERR_HIP;
  int rc = k_fill(ctx, v->d, 1, (double)mine);
  if (rc == PO_OK) rc = k_fill(ctx, one->d, 1, 1.0);
  if (rc == PO_OK) rc = k_fill(ctx, zero->d, 1, 0.0);
  std::vector<const double *> V(ctx->size, zero->d);
  V[ctx->rank] = one->d;
  std::vector<double> out(ctx->size, 0.0);
  if (rc == PO_OK) rc = k_mdot(ctx, v->d, V.data(), ctx->size, 1, out.data());
  for (int r = 0; r < ctx->size; r++) (*all)[r] = (int64_t)(out[r] + 0.5);
  vec_decref(v);
  vec_decref(one);
  vec_decref(zero);
  return rc;
}

int InteriorPoint::solutionFileOffsets(int64_t *nvars_total, int64_t *var_off, int64_t *nw_total, int64_t *w_off) {
  std::vector<int64_t> nv, nwv;
  PO_TRY(gatherCounts(n, &nv));
  PO_TRY(gatherCounts(nw, &nwv));
  *nvars_total = *nw_total = *var_off = *w_off = 0;
  for (int r = 0; r < ctx->size; r++) {
    if (r < ctx->rank) {
      *var_off += nv[r];
      *w_off += nwv[r];
    }
    *nvars_total += nv[r];
    *nw_total += nwv[r];
  }
  return PO_OK;
}

static bool file_block(FILE *fp, bool writing, int64_t byte_offset, double *host, size_t count) {
  if (fseeko(fp, (off_t)byte_offset, SEEK_SET) != 0) return false;
  if (count == 0) return true;
  return (writing ? fwrite(host, sizeof(double), count, fp) : fread(host, sizeof(double), count, fp)) == count;
}

int InteriorPoint::writeSolutionFile(const char *filename) {
  int64_t N = 0, off = 0, Wt = 0, woff = 0;
  PO_TRY(solutionFileOffsets(&N, &off, &Wt, &woff));  // collective
  int ok = 1;
  if (ctx->rank == 0) {
    FILE *fp = fopen(filename, "wb");
    if (fp) {
      int sizes[3] = {(int)N, (int)Wt, c};
      ok = fwrite(sizes, sizeof(int), 3, fp) == 3 && fwrite(&barrier_param, sizeof(double), 1, fp) == 1;
      const std::vector<double> *blocks[5] = {&vars.s, &vars.t, &vars.z, &vars.zs, &vars.zt};
      for (auto *b : blocks) ok = ok && fwrite(b->data(), sizeof(double), c, fp) == (size_t)c;
      fclose(fp);
    } else {
      ok = 0;
    }
  }
  // every rank learns whether the header is there (and waits for it)
  std::vector<int64_t> flags;
  PO_TRY(gatherCounts(ok, &flags));
  if (flags[0] == 0) {
    set_error("cannot open checkpoint file %s", filename);
    return PO_ERR_ARG;
  }
  FILE *fp = fopen(filename, "r+b");
  if (!fp) {
    ok = 0;
  } else {
    const int64_t base = 3 * (int64_t)sizeof(int) + (5 * (int64_t)c + 1) * (int64_t)sizeof(double);
    std::vector<double> host((size_t)std::max<int64_t>(std::max(n, nw), 1));
    Vec *vs[3] = {x, zl, zu};
    for (int b = 0; b < 3 && ok; b++) {
      ok = hipMemcpyAsync(host.data(), vs[b]->d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) ==
               hipSuccess &&
           hipStreamSynchronize(ctx->stream) == hipSuccess &&
           file_block(fp, true, base + 8 * (b * N + off), host.data(), (size_t)n);
    }
    if (Wt > 0) {  // zw then sw, as the reference (:951-968)
      for (int b = 0; b < 2 && ok; b++) {
        ok = (nw == 0 || (hipMemcpyAsync(host.data(), wvar[b]->d, sizeof(double) * (size_t)nw,
                                         hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                          hipStreamSynchronize(ctx->stream) == hipSuccess)) &&
             file_block(fp, true, base + 8 * (3 * N + b * Wt + woff), host.data(), (size_t)nw);
      }
    }
    fclose(fp);
  }
  PO_TRY(gatherCounts(ok, &flags));  // completion barrier + agreement on the outcome
  for (int r = 0; r < ctx->size; r++) {
    if (flags[r] == 0) {
      set_error("writing the checkpoint file %s failed on rank %d", filename, r);
      return PO_ERR_ARG;
    }
  }
  return PO_OK;
}

// readSolutionFile (:983-1104): restart state written by writeSolutionFile (same layout, any rank count)
int InteriorPoint::readSolutionFile(const char *filename) {
  stateReplaced();
  int64_t N = 0, off = 0, Wt = 0, woff = 0;
  PO_TRY(solutionFileOffsets(&N, &off, &Wt, &woff));  // collective
  FILE *fp = fopen(filename, "rb");
  int ok = fp != nullptr;
  int sizes[3] = {0, 0, 0};
  bool size_ok = true;
  if (ok) {
    ok = fread(sizes, sizeof(int), 3, fp) == 3;
    size_ok = ok && sizes[0] == (int)N && sizes[1] == (int)Wt && sizes[2] == c;
    ok = ok && size_ok && fread(&barrier_param, sizeof(double), 1, fp) == 1;
    std::vector<double> *blocks[5] = {&vars.s, &vars.t, &vars.z, &vars.zs, &vars.zt};
    for (auto *b : blocks) ok = ok && fread(b->data(), sizeof(double), c, fp) == (size_t)c;
    const int64_t base = 3 * (int64_t)sizeof(int) + (5 * (int64_t)c + 1) * (int64_t)sizeof(double);
    std::vector<double> host((size_t)std::max<int64_t>(std::max(n, nw), 1));
    Vec *vs[3] = {x, zl, zu};
    for (int b = 0; b < 3 && ok; b++) {
      ok = file_block(fp, false, base + 8 * (b * N + off), host.data(), (size_t)n) &&
           hipMemcpyAsync(vs[b]->d, host.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream) ==
               hipSuccess &&
           hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    if (Wt > 0) {
      for (int b = 0; b < 2 && ok; b++) {
        ok = file_block(fp, false, base + 8 * (3 * N + b * Wt + woff), host.data(), (size_t)nw) &&
             (nw == 0 || (hipMemcpyAsync(wvar[b]->d, host.data(), sizeof(double) * (size_t)nw,
                                         hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                          hipStreamSynchronize(ctx->stream) == hipSuccess));
      }
    }
    fclose(fp);
  }
  std::vector<int64_t> flags;
  PO_TRY(gatherCounts(ok, &flags));  // every rank takes the same decision
  for (int r = 0; r < ctx->size; r++) {
    if (flags[r] == 0) {
      if (!fp) {
        set_error("cannot open solution file %s", filename);
      } else if (!size_ok) {
        set_error("ParOpt: Problem size incompatible with solution file");
      } else {
        set_error("short read or upload failure on solution file %s (rank %d)", filename, r);
      }
      return PO_ERR_ARG;
    }
  }
  Vec *written[5] = {x, zl, zu, has_w ? wvar[0] : nullptr, has_w ? wvar[1] : nullptr};
  for (Vec *v : written) PO_TRY(vec_mirror_refresh(v));
  return PO_OK;
}

}  // namespace po
