// Hessian-vector products of the Lagrangian f - z^T c - zw^T cw for problems that provide none: the Jacobian-free
// Newton-Krylov construction, H p ~ [grad L(x + h p) - grad L(x)] / h (forward) or [grad L(x + h p) - grad L(x - h p)]
// / 2h (central), with the multipliers held fixed.  An extension without a reference counterpart, switched on per solver
// (po_ip_set_hvec_finite_difference); both users of a product -- the Krylov loop of computeKKTGMRESStep and the RES_HVEC
// term of the refinement residual -- go through hvecProduct() below.
//
// What a product costs: one pass for the step size (k_hvec_fd_prepare), one for each perturbed point (k_panel_axpy),
// the problem's evalObjCon + evalObjConGradient at each point -- in that order: the reference never asks for a gradient
// at a point whose values it has not just asked for, and problems cache on that -- and one pass that combines the
// gradients pair by pair (k_hvec_fd_combine).  Everything is written into vectors owned by the solver; what the solver
// holds for the current iterate is the same bits afterwards.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "ip.hpp"

namespace po {

int InteriorPoint::setHvecFiniteDifference(int mode, int central, double rel_step) {
  if (mode != PO_HVEC_EXACT && mode != PO_HVEC_FD_WHEN_MISSING && mode != PO_HVEC_FD_ALWAYS) {
    set_error("po_ip_set_hvec_finite_difference: unknown mode %d", mode);
    return PO_ERR_ARG;
  }
  if (mode != PO_HVEC_EXACT && prob->isSubproblem()) {
    set_error("po_ip_set_hvec_finite_difference: differenced Hessian-vector products are not available for the solver "
              "of a trust-region or MMA subproblem");
    return PO_ERR_ARG;
  }
  if (rel_step != rel_step || rel_step > 0.1) {
    set_error("po_ip_set_hvec_finite_difference: relative step %g is not in (0, 0.1] (<= 0 selects the default)",
              rel_step);
    return PO_ERR_ARG;
  }
  hvec_mode = mode;
  hvec_central = central ? 1 : 0;
  hvec_rel = rel_step > 0.0 ? rel_step : 0.0;
  hvec_fd_active = false;
  return PO_OK;
}

void InteriorPoint::getHvecFiniteDifferenceCount(int *products, int *evaluations) const {
  if (products) *products = hvec_fd_products;
  if (evaluations) *evaluations = hvec_fd_evals;
}

int InteriorPoint::hvecProduct(const double *z, Vec *zw, Vec *p, Vec *hvec) {
  if (hvec_mode != PO_HVEC_FD_ALWAYS && !hvec_fd_active) {
    if (prob->evalHvecProduct(x, z, zw, p, hvec) == 0) return PO_OK;
    if (hvec_mode == PO_HVEC_EXACT) {
      set_error("evalHvecProduct failed or is not provided by the problem");
      return PO_ERR_USER;
    }
    hvec_fd_active = true;  // PO_HVEC_FD_WHEN_MISSING: differences for the rest of this solver's life
  }
  return hvecFiniteDifference(z, zw, p, hvec);
}

int InteriorPoint::evalHvec(const double *z, Vec *zw, Vec *p, Vec *hvec) {
  if (!p || !hvec || p->n != n || hvec->n != n || (c > 0 && !z) || (has_w && (!zw || zw->n != nw)) || p == hvec) {
    set_error("po_ip_eval_hvec: px and hvec must be two design-sized vectors, z has one entry per dense constraint and "
              "zw is sized like the sparse constraints");
    return PO_ERR_ARG;
  }
  const int rc = hvecProduct(z, has_w ? zw : nullptr, p, hvec);
  if (user_timing && user_pending > 0) {
    // outside optimize() nothing else reads the callbacks' event pairs: their stream time goes to a phase of its own
    const double before = user_seconds;
    userHarvest();
    size_t i = 0;
    while (i < phase_names.size() && phase_names[i] != "hvec_user_eval") i++;
    if (i == phase_names.size()) {
      phase_names.push_back("hvec_user_eval");
      phase_seconds.push_back(0.0);
    }
    phase_seconds[i] += user_seconds - before;
  }
  return rc;
}

// The scratch of the differenced products: the perturbed point and `sides` sets of (g, A_1 .. A_nc), allocated on
// first use and never otherwise.
int InteriorPoint::hvecScratch(int sides, int nc) {
  if (!hvec_xp) {
    hvec_xp = vec_new(ctx, n);
    if (!hvec_xp) return PO_ERR_HIP;
  }
  for (int s = 0; s < sides; s++) {
    while ((int)hvec_work[s].size() < nc + 1) {
      Vec *v = vec_new(ctx, n);
      if (!v) return PO_ERR_HIP;
      hvec_work[s].push_back(v);
    }
  }
  return PO_OK;
}

// values, then gradient, at xp = x + a p into scratch set `side`; with_jac: the dense Jacobian as well
int InteriorPoint::hvecEvalAt(double a, Vec *p, int side, bool with_jac) {
  // xp = x + (a p): the product is rounded before the sum, so that the point is the one plain arithmetic gives
  PO_TRY(k_panel_axpy(ctx, hvec_xp->d, a, p->d, 0.0, nullptr, nullptr, 0, n));
  PO_TRY(k_axpy(ctx, hvec_xp->d, 1.0, x->d, n));
  double f_unused = 0.0;
  std::vector<double> c_unused(c > 0 ? c : 1, 0.0);
  std::vector<Vec *> &W = hvec_work[side];
  userBegin();
  int fail = prob->evalObjCon(hvec_xp, &f_unused, c_unused.data());
  if (!fail) fail = prob->evalObjConGradient(hvec_xp, W[0], with_jac ? W.data() + 1 : nullptr);
  userEnd();
  hvec_fd_evals++;
  // (the values go nowhere: a problem with deferred reductions must not find their landing area gone at a later flush)
  if (ctx->batch_depth > 0) PO_TRY(batch_flush(ctx));
  if (fail) {
    set_error("Hessian-vector product by differences: the evaluation at the perturbed point failed");
    return PO_ERR_USER;
  }
  return PO_OK;
}

int InteriorPoint::hvecFiniteDifference(const double *z, Vec *zw, Vec *p, Vec *hvec) {
  if (prob->isSubproblem()) {
    set_error("differenced Hessian-vector products are not available for a trust-region or MMA subproblem");
    return PO_ERR_ARG;
  }
  if (!hvec_central && !iterate_flags.ac_valid) {
    set_error("Hessian-vector product by forward differences: the solver holds no gradient at its current point "
              "(call optimize() first)");
    return PO_ERR_ARG;
  }
  hvec_fd_products++;
  // the step size: identical on every rank, since both sums and both minima come out of one reduction
  double red[4] = {0.0, 0.0, 0.0, 0.0};
  PO_TRY(k_hvec_fd_prepare(ctx, bounds(), p->d, n, red));
  const double pnorm = sqrt(red[1]);
  if (!(pnorm > 0.0)) {  // no direction: no callback
    hvec_fd_h = 0.0;
    return k_fill(ctx, hvec->d, n, 0.0);
  }
  const double rel = hvec_rel > 0.0 ? hvec_rel : (hvec_central ? cbrt(DBL_EPSILON) : sqrt(DBL_EPSILON));
  const double to_bound = hvec_central ? std::min(red[2], red[3]) : red[2];
  const double h = std::min(rel * (1.0 + sqrt(red[0])) / pnorm, 0.5 * to_bound);
  if (!(h > 0.0)) {
    set_error("Hessian-vector product by differences: no room for a step inside the bounds (step %g)", h);
    return PO_ERR_ARG;
  }
  hvec_fd_h = h;
  // a problem with linear dense constraints keeps its Jacobian: the constraint terms drop out of the difference
  const bool with_jac = c > 0 && !(prob->linear_constraints && iterate_flags.ac_valid);
  const int nc = with_jac ? c : 0, sides = hvec_central ? 2 : 1;
  PO_TRY(hvecScratch(sides, nc));
  // CSR form: the evaluations at the perturbed points overwrite the library's value array and constraint values
  CsrSparse *csr = has_w ? prob->csr : nullptr;
  if (csr) {
    if (!hvec_csr_data || hvec_csr_nnz < csr->nnz) {
      vec_decref(hvec_csr_data);
      hvec_csr_data = vec_new(ctx, csr->nnz > 0 ? csr->nnz : 1);
      hvec_csr_nnz = csr->nnz;
      if (!hvec_csr_data) return PO_ERR_HIP;
    }
    if (!hvec_csr_cw) {
      hvec_csr_cw = vec_new(ctx, nw > 0 ? nw : 1);
      if (!hvec_csr_cw) return PO_ERR_HIP;
    }
    PO_TRY(k_copy(ctx, hvec_csr_data->d, csr->data, csr->nnz));
    PO_TRY(k_copy(ctx, hvec_csr_cw->d, csr->cw->d, nw));
  }
  const double s = hvec_central ? 0.5 / h : 1.0 / h;
  int rc = PO_OK;
  auto body = [&]() -> int {
    // the sparse constraints enter as -s Aw(x+)^T zw + s Aw(x-)^T zw, accumulated in hvec ahead of the dense terms
    if (has_w) PO_TRY(k_fill(ctx, hvec->d, n, 0.0));
    PO_TRY(hvecEvalAt(h, p, 0, with_jac));
    if (has_w && prob->addSparseJacobianTranspose(-s, hvec_xp, zw, hvec) != 0) return PO_ERR_USER;
    if (hvec_central) {
      PO_TRY(hvecEvalAt(-h, p, 1, with_jac));
      if (has_w && prob->addSparseJacobianTranspose(s, hvec_xp, zw, hvec) != 0) return PO_ERR_USER;
    }
    return PO_OK;
  };
  rc = body();
  if (csr) {  // back to the iterate's values, also when an evaluation failed
    int rc2 = k_copy(ctx, csr->data, hvec_csr_data->d, csr->nnz);
    if (rc2 == PO_OK) rc2 = k_copy(ctx, csr->cw->d, hvec_csr_cw->d, nw);
    if (rc2 == PO_OK) rc2 = prob->csrValuesChanged();
    if (rc == PO_OK) rc = rc2;
  }
  PO_TRY(rc);
  if (has_w && !hvec_central && prob->addSparseJacobianTranspose(s, x, zw, hvec) != 0) return PO_ERR_USER;
  // the minus side of the forward form is the live gradient and Jacobian of the iterate
  std::vector<const double *> Ap(nc > 0 ? nc : 1, nullptr), Am(nc > 0 ? nc : 1, nullptr);
  for (int j = 0; j < nc; j++) {
    Ap[j] = hvec_work[0][1 + j]->d;
    Am[j] = hvec_central ? hvec_work[1][1 + j]->d : Ac[j]->d;
  }
  return k_hvec_fd_combine(ctx, hvec->d, s, hvec_work[0][0]->d, hvec_central ? hvec_work[1][0]->d : g->d, z, Ap.data(),
                           Am.data(), nc, n, has_w ? 1 : 0);
}

}  // namespace po
