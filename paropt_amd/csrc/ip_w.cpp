// The sparse ("weighting") constraint path of the interior-point mirror: nwcon > 0 with nwblock = 1,
// i.e. a diagonal Cw = (Cdiag + Aw D^-1 Aw^T)^-1 (reference src/ParOptSparseMat.cpp:41-229 and the
// `nwcon > 0` branches of src/ParOptInteriorPoint.cpp cited per function).
//
// The design-space operator of K0 changes from diag(Dinv) to
//     D0x^-1 = Dinv - Dinv Aw^T Cw Aw Dinv                      (ParOptQuasiDefBlockMat::apply :122-190)
// and everything the dense path does with the weighted Gram  W = P^T Dinv P  carries over with
//     W = P^T Dinv P - U^T Cw U,   U_j = Aw (Dinv o P_j)        (one extra w-sized Gram)
// so the Schur complements G, Ce and the analytic P^T px bookkeeping are unchanged (ip.cpp).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ip.hpp"

namespace po {

int comm_allreduce_host(Ctx *c, double *values, int count, int op);  // context.cpp

WVars InteriorPoint::wv() const { return WVars{wvar[0]->d, wvar[1]->d, wvar[2]->d, wvar[3]->d, wvar[4]->d}; }
WVars InteriorPoint::wr() const {
  return WVars{wresv[0]->d, wresv[1]->d, wresv[2]->d, wresv[3]->d, wresv[4]->d};
}
WVars InteriorPoint::wp() const {
  return WVars{wstepv[0]->d, wstepv[1]->d, wstepv[2]->d, wstepv[3]->d, wstepv[4]->d};
}

void InteriorPoint::getOptimizedSparse(Vec *v[5]) {
  for (int i = 0; i < 5; i++) v[i] = has_w ? wvar[i] : nullptr;
}

int InteriorPoint::allocateW() {
  // path selection must be uniform across ranks (every reduction is collective)
  Vec *cnt = vec_new(ctx, 1);
  if (!cnt) return PO_ERR_HIP;
  PO_TRY(k_fill(ctx, cnt->d, 1, (double)nw));
  double total = 0.0;
  PO_TRY(k_reduce1(ctx, RED_ASUM, cnt->d, nullptr, 1, &total));
  vec_decref(cnt);
  nw_global = total;
  has_w = total > 0.0;
  if (!has_w) return PO_OK;
  // ... and so must be whether the problem brings its own quasi-definite solver (the two Gram corrections issue
  // different reductions): checked once, collectively
  if (ctx->size > 1) {
    double mm[2] = {prob->sparseUserSolver() ? 1.0 : 0.0, prob->sparseUserSolver() ? -1.0 : 0.0};
    PO_TRY(comm_allreduce_host(ctx, mm, 2, 1));  // {min of the flag, -max of the flag}
    if (mm[0] != -mm[1]) {
      set_error("a quasi-definite solver (po_problem_set_quasidef_callbacks) is attached on some ranks only");
      return PO_ERR_ARG;
    }
  }
  Vec **all[] = {&gsw, &gtw, &Cw, &wd2, &wyw, &wtmp, &wtmp2, &cwx};
  for (Vec **v : all) {
    *v = vec_new(ctx, nw);
    if (!*v) return PO_ERR_HIP;
  }
  for (int i = 0; i < 5; i++) {
    wvar[i] = vec_new(ctx, nw);
    wresv[i] = vec_new(ctx, nw);
    wstepv[i] = vec_new(ctx, nw);
    if (!wvar[i] || !wresv[i] || !wstepv[i]) return PO_ERR_HIP;
    PO_TRY(k_fill(ctx, wvar[i]->d, nw, 1.0));  // constructor state (:439-446)
  }
  d1v = vec_new(ctx, n);
  if (!d1v) return PO_ERR_HIP;
  PO_TRY(k_w_gamma(ctx, gsw->d, gtw->d, options.real("penalty_gamma"), prob->nwinequality, nw));
  return PO_OK;
}

// (yx, yw) <- K0^-1 (bx, bw), ParOptQuasiDefBlockMat::apply (src/ParOptSparseMat.cpp:122-190);
// bw == nullptr stands for a zero block.  bx must not alias yx->d.
int InteriorPoint::applyK0(const double *bx, const double *bw, Vec *yx, Vec *yw) {
  return prob->sparseApplyK0(x, Dinv, Cw, bx, bw, yx, yw, wtmp);
}

// the w blocks of computeKKTRes (:1358-1398) and their norms
// (norms = false: the blocks only -- the caller knows that the sums of this mu and iterate are already in place)
int InteriorPoint::sparseConAtIterate(const double **cw) {
  if (!iterate_flags.cwx_valid) {
    if (prob->evalSparseCon(x, cwx) != 0) return PO_ERR_USER;
    iterate_flags.cwx_valid = true;
  }
  *cw = cwx->d;
  return PO_OK;
}

int InteriorPoint::computeResidualW(double mu, bool norms, bool with_d2) {
  const double *cw = nullptr;
  PO_TRY(sparseConAtIterate(&cw));
  scratch_flags.wd2_ready = false;
  PO_TRY(k_w_res(ctx, wv(), wr(), gsw->d, gtw->d, mu, nw, norms ? wres_out : nullptr, cw, with_d2 ? wd2->d : nullptr));
  if (!norms) return PO_OK;
  after_reduce(ctx, [this] {
    for (int i = 0; i < 7; i++) w_sums[i] = wres_out[i];
    for (int i = 0; i < 5; i++) w_maxs[i] = wres_out[7 + i];
  });
  return PO_OK;
}

int InteriorPoint::wCompStep(double ax, double az, double *prod) {
  return k_w_comp_step(ctx, wv(), wp(), ax, az, nw, prod);
}

// W -= U^T S^-1 U with U_j = Aw (Dinv o P_j), S = C + Aw Dinv Aw^T (diagonal for the block form: Cw = S^-1)
int InteriorPoint::panelImageVectors(int m, std::vector<double *> &U) {
  while ((int)Uw.size() < m) {
    Vec *u = vec_new(ctx, nw);
    if (!u) return PO_ERR_HIP;
    Uw.push_back(u);
  }
  U.resize(m);
  for (int j = 0; j < m; j++) U[j] = Uw[j]->d;
  return PO_OK;
}
std::vector<const double *> InteriorPoint::correctionPanel(int m) const {
  std::vector<const double *> C(m);
  for (int j = 0; j < m; j++) C[j] = (panel_form.solved ? Yw[j] : Uw[j])->d;
  return C;
}
// panel_done: the Gram pass over P has already written U (Problem::sparseGramGroups)
int InteriorPoint::sparseGramCorrection(const std::vector<const double *> &P, int m, Vec *work, bool may_defer,
                                        bool panel_done) {
  if (m <= 0) return PO_OK;
  std::vector<double *> U;
  PO_TRY(panelImageVectors(m, U));
  // What the problem's solver makes of the panel (quasidef.hpp): a half solve in place -- scalar forms: nothing, the
  // weights are Cw; packed blocks and CSR: U <- L^-1 U with S = L L^T, unit weights -- or, where the user exposes no
  // factor, a second panel Yw_j = -S^-1 U_j from one three-argument apply per column (the reference makes c for G,
  // :1937, and two inside each of the k diagonal solves, :2398, 2427).
  const GramForm form = panel_form = prob->sparseGramForm();
  std::vector<double *> Y;
  while (form.solved && (int)Yw.size() < m) {
    Vec *y = vec_new(ctx, nw);
    if (!y) return PO_ERR_HIP;
    Yw.push_back(y);
  }
  for (int j = 0; form.solved && j < m; j++) Y.push_back(Yw[j]->d);
  if (form.solved && kkt.W.size() != (size_t)m * m) {
    // (the caller sized W for this panel: a Schur-complement term is never dropped)
    set_error("internal: the Gram matrix holds %zu entries for a panel of %d columns", kkt.W.size(), m);
    return PO_ERR_ARG;
  }
  W2_buf.assign((size_t)m * m, 0.0);
  // panel, gramSolve and the w-sized product (Problem::sparseGramProduct, shared with po_quasidef_gram).  may_defer:
  // inside setUpKKTSystem's batch the product arrives at the flush: a member holds it, the update of W follows it there
  bool cross = false;
  PO_TRY(prob->sparseGramProduct(x, Dinv, P.data(), m, U.data(), Y.data(), Cw, work ? work : tvec, panel_done, may_defer,
                                 W2_buf.data(), &cross));
  if (cross) {
    // the cross product W += U^T Yw of two different w-sized panels, symmetric up to rounding: both halves are averaged
    after_reduce(ctx, [this, m] {
      for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++)
          kkt.W[i + (size_t)m * j] += 0.5 * (W2_buf[i + (size_t)m * j] + W2_buf[j + (size_t)m * i]);
    });
  } else {
    after_reduce(ctx, [this] {
      for (size_t i = 0; i < W2_buf.size() && i < kkt.W.size(); i++) kkt.W[i] -= W2_buf[i];
    });
  }
  scratch_flags.panel_valid = true;  // Uw (and Yw) hold the panel of the CURRENT Dinv, factor and panel columns
  return PO_OK;
}

// computeKKTStep (:2700-2737) with both solveKKTDiagSystem overloads folded together, sparse blocks
// included.  first pass: rhs = (rx, wres, b); refine pass: d1v already holds the raw d1' and wres r'.
int InteriorPoint::solveKKTW(const Dense &b, double mu, bool use_qn, bool refine_pass, double tau,
                             Dense &out, bool fuse_residual) {
  const double beta_mu = options.real("rel_bound_barrier") * mu;
  int k = 0;
  std::vector<const double *> P = panel(use_qn, &k);
  PO_TRY(kkt.checkWidth(k));
  const int m = c + k;
  const double *cl = (corrector_active && !refine_pass) ? s_qn->d : nullptr;
  const double *cu = (corrector_active && !refine_pass) ? y_qn->d : nullptr;
  // t = [K0^-1 (d1, d2)]_x, wyw and P^T t were produced by setUpKKTSystem when the right-hand side was known then
  const bool have_t0 = !refine_pass && scratch_flags.t0_valid && t0_mu == mu && !cl && (int)t0dots.size() == m && m > 0;
  std::vector<double> dots(m > 0 ? m : 1, 0.0);
  if (have_t0) {
    for (int i = 0; i < m; i++) dots[i] = t0dots[i];
  } else {
    if (!refine_pass) PO_TRY(k_d1(ctx, bounds(), rx->d, nullptr, beta_mu, n, d1v->d, cl, cu));
    // (wd2_ready: formed by the pass that wrote the blocks)
    if (!scratch_flags.wd2_ready) PO_TRY(k_w_d2(ctx, wv(), wr(), nw, wd2->d));
    scratch_flags.wd2_ready = false;
    PO_TRY(applyK0(d1v->d, wd2->d, tvec, wyw));
    if (refine_pass && step_flags.tdots_valid && (int)tdots.size() == m && m > 0 && scratch_flags.panel_valid &&
        panel_form.plain && (int)Uw.size() >= m) {
      // tvec = Dinv o (d1' + Aw^T yw): P^T tvec = P^T (Dinv o d1') + U^T yw with U = Aw (Dinv o P) -- the first
      // term came out of the fused first pass, the second is a w-sized product with the panel image
      std::vector<const double *> Uc(m);
      for (int j = 0; j < m; j++) Uc[j] = Uw[j]->d;
      PO_TRY(k_mdot(ctx, wyw->d, Uc.data(), m, nw, dots.data()));
      for (int i = 0; i < m; i++) dots[i] += tdots[i];
    } else if (m > 0) {
      PO_TRY(k_mdot(ctx, tvec->d, P.data(), m, n, dots.data()));
    }
  }
  if (!refine_pass) scratch_flags.t0_valid = false;  // tvec is overwritten below
  bool first_px_only = refine_pass && step_flags.px_first_only;  // px holds the first step, pzl / pzu were not stored
  const Bordered::Sol sol = solveBordered(b, dots.data(), refine_pass);
  const bool have_corr_panel = m > 0 && (int)Uw.size() >= m && scratch_flags.panel_valid;
  if (first_px_only && !have_corr_panel) {
    // (not reached with the flags as they are set: the fused first pass implies a valid panel) the stored-step forms
    // below need the first bound-multiplier steps as vectors
    PO_TRY(k_form_pz(ctx, bounds(), px->d, beta_mu, n, pzl->d, pzu->d));
    first_px_only = false;
  }
  // (dx, dzw) = K0^-1 (d1 + P alpha, d2) = K0^-1 (d1, d2) + K0^-1 (P alpha, 0), and the second term comes from
  // the panel the Gram correction already holds: dzw += -S^-1 (U alpha), dx += Dinv (P alpha + Aw^T of that) -
  // no second quasi-definite apply, and P alpha rides in the same pass that forms the bound multipliers
  const bool seq_lin = options.integer("sequential_linear_method");
  const int kq = (qn && !seq_lin) ? qn->size() : 0;
  // Fused refinement residual (as on the dense path, ip.cpp solveKKT): the coefficients of addKKTResStep are known
  // before the axpy pass starts, and so is the sparse multiplier step pzw (it depends on wyw only), so ONE pass
  // over P writes the step, the RAW right-hand side d1' of the refinement solve (its design rows, :1451-1483, with
  // the extra column Aw^T pzw) and the panel products of Dinv o d1'.
  const bool fuse = fuse_residual && !refine_pass && forms.analytic_panel_dots && kq == k && have_corr_panel &&
                    panel_form.plain && !cl && !(options.integer("use_diag_hessian") && hdiag) && m + 2 <= kMaxPanel;
  // the fraction-to-boundary minima of the design and of the sparse blocks: one collective + sync in every form
  double mins_x[2], mins_w[2];
  const SolvePass sp{P, sol.coef, m, beta_mu, tau};
  if (fuse) {
    PO_TRY(fusedFirstPassW(sp, k, mins_x, mins_w));
  } else if (have_corr_panel) {
    PO_TRY(correctionPanelSolve(sp, refine_pass, first_px_only, cl, cu, mins_x, mins_w));
  } else {
    PO_TRY(blockSolveFallback(sp, refine_pass, cl, cu, mins_x, mins_w));
  }
  step_mins[0] = std::min(mins_x[0], mins_w[0]);
  step_mins[1] = std::min(mins_x[1], mins_w[1]);
  kkt.backSubstitute(1.0, b, vars, sol, true, out);
  return PO_OK;
}

// Fused first pass, sparse constraints -- taken for the first solve when the correction panel is the plain image of the
// current system and the refinement residual can be written as panel coefficients (`fuse` in solveKKTW).  Of the step
// only px is stored.  Sets px_first_only, tdots_valid and residual_fused.
int InteriorPoint::fusedFirstPassW(const SolvePass &sp, int k, double mins_x[2], double mins_w[2]) {
  const int m = sp.m;
  const bool seq_lin = options.integer("sequential_linear_method");
  BatchScope minbatch(ctx, false);  // (opened right before the first of the two launches: no user code runs between them)
  std::vector<const double *> Uc = correctionPanel(m);
  PO_TRY(prob->sparseCorrection(Uc.data(), m, sp.alpha.data(), Cw, wtmp2, wyw));  // ... and wyw += wtmp2
  // the two extra columns Aw^T wtmp2 (coefficient 1 in the step's row sum) and Aw^T pzw (1 in the residual's): n-sized
  // vectors from Problem::setSparseJacobianTranspose, or -- structured problems -- described and formed by the pass
  GroupCols2 gcs;
  const bool grouped = prob->sparseTransposeColumn(1.0, x, wtmp2, &gcs.g[0]);
  if (!grouped && prob->setSparseJacobianTranspose(1.0, x, wtmp2, d1v) != 0) return PO_ERR_USER;
  // sparse blocks of the step first: pzw = wstepv[0] feeds the residual column Aw^T pzw (its minima wait for
  // those of the design blocks unless user code runs in between)
  if (prob->reductionsBatchable()) minbatch.begin();
  PO_TRY(k_w_step(ctx, wv(), wr(), wyw->d, 0, sp.tau, wp(), nw, mins_w));
  if (grouped) {
    if (!prob->sparseTransposeColumn(1.0, x, wstepv[0], &gcs.g[1])) {
      set_error("internal: the problem describes one sparse transpose column but not the other");
      return PO_ERR_ARG;
    }
    gcs.count = 2;
    gcs.ca[0] = 1.0;
    gcs.cb[1] = 1.0;
  } else if (prob->setSparseJacobianTranspose(1.0, x, wstepv[0], xt) != 0) {
    return PO_ERR_USER;
  }
  std::vector<const double *> P1(sp.P);
  std::vector<double> a1(sp.alpha.begin(), sp.alpha.begin() + m), c2(m + 2, 0.0);
  if (!grouped) {
    P1.push_back(d1v->d);
    a1.push_back(1.0);
    P1.push_back(xt->d);
    a1.push_back(0.0);
  }
  const int np1 = (int)P1.size();
  double diag = 0.0;  // (alpha[0..c) = step.z)
  PO_TRY(residualCoefs(qn && !seq_lin ? RES_QN : RES_SIGMA, sp.alpha.data(), ptpx.data() + c, k, c2, &diag));
  c2[m + 1] = 1.0;
  std::vector<double> so(m + 4, 0.0);
  // the raw right-hand side lands in y_qn (free while no corrector is active: y_qn is rebuilt from scratch by
  // computeStepAndUpdate) -- d1v is one of the columns being read -- and the two exchange buffers afterwards.
  // Of the step only px is stored (store_step 2): the refinement's sparse rows need Aw px as a vector, the bound-
  // multiplier steps are re-formed from px by the refinement pass (two output streams less)
  PO_TRY(k_solve2_dots(ctx, {.b = bounds(), .t = tvec->d, .dinv = Dinv->d, .alpha = a1.data(), .coef2 = c2.data(),
                             .P = P1.data(), .nv = np1, .beta_mu = sp.beta_mu, .tau = sp.tau, .rx = rx->d,
                             .diag = diag, .n = n, .px = px->d, .pzl = pzl->d, .pzu = pzu->d, .out = so.data(),
                             .traw = y_qn->d, .store_step = 2, .gcols = grouped ? &gcs : nullptr}));
  step_flags.px_first_only = true;
  std::swap(d1v->d, y_qn->d);
  PO_TRY(minbatch.end());
  tdots.assign(so.begin(), so.begin() + m);
  step_flags.tdots_valid = true;
  step_flags.residual_fused = true;
  mins_x[0] = so[np1];  // out = {dots[np1], max_x, max_z}
  mins_x[1] = so[np1 + 1];
  return PO_OK;
}

// Correction-panel solve -- taken whenever the panel image of the current system is at hand and the fused first pass is
// not: K0^-1 (P alpha, 0) comes from the panel, one more column Aw^T wtmp2 rides in the design pass.  first_px_only:
// the refinement on top of a fused first pass, which re-forms the first bound-multiplier steps from px; when it takes
// the merit sums it sets fused_merit_valid, w_comp_valid and w_merit_cache_valid, and a lean step clears pz_stored
// (with step_beta_mu).  Otherwise the stored-step kernel, which sets no flag.
int InteriorPoint::correctionPanelSolve(const SolvePass &sp, bool refine_pass, bool first_px_only, const double *cl,
                                        const double *cu, double mins_x[2], double mins_w[2]) {
  const int m = sp.m;
  BatchScope minbatch(ctx, false);
  std::vector<const double *> Uc = correctionPanel(m);
  PO_TRY(prob->sparseCorrection(Uc.data(), m, sp.alpha.data(), Cw, wtmp2, wyw));  // ... and wyw += wtmp2
  // the extra column Aw^T wtmp2 (coefficient 1): stored, or (structured problems, refinement of a px-only first
  // step) described and formed by the pass itself
  GroupCol gcol;
  const bool grouped = first_px_only && prob->sparseTransposeColumn(1.0, x, wtmp2, &gcol);
  if (!grouped && prob->setSparseJacobianTranspose(1.0, x, wtmp2, d1v) != 0) return PO_ERR_USER;
  std::vector<const double *> P1(sp.P);
  std::vector<double> a1(sp.alpha.begin(), sp.alpha.begin() + m);
  if (!grouped) {
    P1.push_back(d1v->d);
    a1.push_back(1.0);
  }
  minbatch.begin();
  if (!first_px_only) {
    PO_TRY(k_solve2(ctx, {.b = bounds(), .t = tvec->d, .dinv = Dinv->d, .alpha = a1.data(), .P = P1.data(),
                          .nv = m + 1, .beta_mu = sp.beta_mu, .refine = refine_pass ? 1 : 0, .tau = sp.tau, .n = n,
                          .px = px->d, .pzl = pzl->d, .pzu = pzu->d, .out = mins_x, .rx = rx->d, .cl = cl, .cu = cu}));
  } else {
    // Refinement on top of a first step of which only px was stored: solve2r_kernel in its stored right-hand side
    // form with a ZERO first coefficient set and t1 = px -- it re-forms (pzl, pzu) of the first step from px
    // (the very expressions the first pass evaluated: same bits), applies the refinement (t2 = tvec, a2) and takes
    // the complementarity / merit sums of the FINAL step (fused_merit); the final px goes to xt (free during the
    // solves) and the two buffers are exchanged.  Lean step: (pzl, pzu) are not stored either -- their only
    // consumer left is the multiplier update of computeStepAndUpdate, which re-forms them (kkt_res_update_kernel)
    const bool take_merit = forms.fuse_merit && !cl;
    const bool lean = take_merit && forms.lean_step && lean_step_allowed && iterate_flags.iterate_logs_valid &&
                      !prob->linear_constraints && options.integer("iterative_refinement_steps") == 1;
    std::vector<double> azero(m + 1, 0.0);
    PO_TRY(k_solve2r(ctx, {.b = bounds(), .t1 = px->d, .t2 = tvec->d, .dinv = Dinv->d, .a1 = azero.data(),
                           .a2 = a1.data(), .P = P1.data(), .nv = (int)P1.size(), .beta_mu = sp.beta_mu,
                           .tau = sp.tau, .n = n, .px = xt->d, .pzl = lean ? nullptr : pzl->d,
                           .pzu = lean ? nullptr : pzu->d, .out = mins_x, .g = take_merit ? g->d : nullptr,
                           .merit_out = take_merit ? fused_merit.as_array() : nullptr,
                           .gcol = grouped ? &gcol : nullptr, .gc2 = 1.0}));
    std::swap(px->d, xt->d);
    if (lean) {
      step_flags.pz_stored = false;
      step_beta_mu = sp.beta_mu;
    }
    if (take_merit) {
      // the sparse blocks of the final step, their share of the complementarity polynomial and the sparse merit
      // sums (at sx = 1) in the same batch: scaleKKTStep and evalMeritInitDeriv then launch nothing
      PO_TRY(k_w_step(ctx, wv(), wr(), wyw->d, 1, sp.tau, wp(), nw, w_step_out, 1));
      const double *cw = nullptr;
      PO_TRY(sparseConAtIterate(&cw));
      PO_TRY(prob->setSparseJacobian(1.0, x, px, wtmp2));
      PO_TRY(k_w_merit(ctx, wv(), wp(), 1.0, gsw->d, gtw->d, cw, wtmp2->d, nw, w_merit_cache));
      PO_TRY(minbatch.end());
      mins_x[0] = fused_merit.max_x;
      mins_x[1] = fused_merit.max_z;
      mins_w[0] = w_step_out[3];
      mins_w[1] = w_step_out[4];
      for (int i = 0; i < 3; i++) w_comp_poly[i] = w_step_out[i];
      step_flags.fused_merit_valid = true;
      step_flags.w_comp_valid = true;
      step_flags.w_merit_cache_valid = true;
      return PO_OK;  // (the sparse step was taken above, with its other sums)
    }
  }
  PO_TRY(k_w_step(ctx, wv(), wr(), wyw->d, refine_pass ? 1 : 0, sp.tau, wp(), nw, mins_w));
  return minbatch.end();
}

// Block-solve fallback -- no panel image at hand (no panel columns, or a problem-supplied solver that keeps none):
// P alpha is formed as a vector and goes through a second quasi-definite apply.  Sets no flag.
int InteriorPoint::blockSolveFallback(const SolvePass &sp, bool refine_pass, const double *cl, const double *cu,
                                      double mins_x[2], double mins_w[2]) {
  BatchScope minbatch(ctx, false);
  if (sp.m > 0) PO_TRY(k_panel_axpy(ctx, d1v->d, 0.0, nullptr, 1.0, sp.alpha.data(), sp.P.data(), sp.m, n));
  PO_TRY(applyK0(d1v->d, wd2->d, tvec, wyw));
  minbatch.begin();
  PO_TRY(k_solve2(ctx, {.b = bounds(), .t = tvec->d, .dinv = Dinv->d, .beta_mu = sp.beta_mu,
                        .refine = refine_pass ? 1 : 0, .tau = sp.tau, .n = n, .px = px->d, .pzl = pzl->d,
                        .pzu = pzu->d, .out = mins_x, .rx = rx->d, .cl = cl, .cu = cu}));
  PO_TRY(k_w_step(ctx, wv(), wr(), wyw->d, refine_pass ? 1 : 0, sp.tau, wp(), nw, mins_w));
  return minbatch.end();
}

// initLeastSquaresMultipliers (:5366-5534) with the sparse blocks
int InteriorPoint::initLeastSquaresMultipliersW() {
  const double mu0 = options.real("init_barrier_param");
  for (int i = 0; i < 5; i++) PO_TRY(k_fill(ctx, wvar[i]->d, nw, mu0));
  const double small = 1e-4;
  PO_TRY(k_fill(ctx, Dinv->d, n, 1.0));
  PO_TRY(k_fill(ctx, Cw->d, nw, small));
  PO_TRY(prob->sparseFactor(x, Dinv, Cw));  // mat->factor (:5429)
  int k = 0;
  std::vector<const double *> A = panel(false, &k);
  kkt.W.assign((size_t)c * c, 0.0);
  std::vector<int> piv(c > 0 ? c : 1);
  if (c > 0) {
    PO_TRY(k_wgram(ctx, Dinv->d, A.data(), c, n, kkt.W.data()));
    PO_TRY(sparseGramCorrection(A, c, nullptr));
    for (int i = 0; i < c; i++) kkt.W[(size_t)i * (c + 1)] += small;
    lu_factor(c, kkt.W.data(), c, piv.data());
  }
  // rx = -(g - zl + zu)
  const double al[2] = {1.0, -1.0};
  const double *vv[2] = {zl->d, zu->d};
  PO_TRY(k_panel_axpy(ctx, d1v->d, -1.0, g->d, 0.0, al, vv, 2, n));
  PO_TRY(applyK0(d1v->d, nullptr, tvec, wyw));
  std::vector<double> z(c > 0 ? c : 1, 0.0);
  if (c > 0) {
    PO_TRY(k_mdot(ctx, tvec->d, A.data(), c, n, z.data()));
    for (int i = 0; i < c; i++) z[i] = -z[i];
    lu_solve(c, kkt.W.data(), c, piv.data(), z.data());
    PO_TRY(k_panel_axpy(ctx, d1v->d, 0.0, nullptr, 1.0, z.data(), A.data(), c, n));
  }
  PO_TRY(applyK0(d1v->d, nullptr, tvec, wyw));
  for (int i = 0; i < c; i++) {
    const double gam = 10.0 * std::max(gamma_s[i], gamma_t[i]);
    vars.z[i] = (z[i] < -gam || z[i] > gam) ? 0.0 : z[i];
  }
  PO_TRY(k_w_clip(ctx, wvar[0]->d, wyw->d, gsw->d, gtw->d, nw));
  scratch_flags.panel_valid = false;  // Uw was built with Dinv = 1 and the constraint columns only
  return PO_OK;
}

}  // namespace po
