// Problem implementations: the C-callback problem and the device-resident separable workloads.
#include <math.h>
#include <stdio.h>

#include <string>

#include "problem.hpp"

namespace po {

static void shard(int64_t n, int rank, int size, int64_t *nlocal, int64_t *offset) {
  const int64_t base = n / size, rem = n % size;
  *nlocal = base + (rank < rem ? 1 : 0);
  *offset = rank * base + (rank < rem ? rank : rem);
}

// ---- CSR form (ParOptSparseProblem) and the generic fallbacks ------------------------------------
int comm_allreduce_host(Ctx *c, double *values, int count, int op);  // context.cpp

// Rows of equal length nw with consecutive columns at equal spacing: the grouped pattern of problem.hpp
static bool recognise_groups(int64_t n, int64_t w, const int *rowp, const int *cols, GroupMap *gm) {
  if (w <= 0 || rowp[0] != 0) return false;
  const int64_t nw = rowp[1] - rowp[0];
  if (nw <= 0 || nw > (1 << 20)) return false;
  const int64_t start = cols[0];
  int64_t period = nw;
  if (w > 1) {
    if (rowp[2] - rowp[1] != nw) return false;
    period = (int64_t)cols[rowp[1]] - start;
  }
  if (start < 0 || period < nw || start + (w - 1) * period + nw > n) return false;
  for (int64_t i = 0; i < w; i++) {
    if (rowp[i + 1] - rowp[i] != nw) return false;
    const int *cr = cols + rowp[i];
    const int64_t c0 = start + i * period;
    for (int64_t k = 0; k < nw; k++)
      if (cr[k] != c0 + k) return false;
  }
  gm->nwcon = w;
  gm->start = start;
  gm->nw = (int)nw;
  gm->skip = (int)(period - nw);
  return true;
}

int Problem::setSparseJacobianData(int64_t nwcon_, int64_t nwineq_, const int *rowp, const int *cols) {
  if (nwcon_ < 0 || nwineq_ < 0 || nwineq_ > nwcon_ || !rowp || (rowp[nwcon_] > 0 && !cols)) {
    set_error("setSparseJacobianData: bad arguments");
    return PO_ERR_ARG;
  }
  static const bool no_groups = dbg_switch(SW_NO_CSR_GROUPS) != 0;
  GroupMap gm;
  bool rec = !no_groups && nwblock == 1 && ((nwcon_ == 0 && ctx->size > 1) || recognise_groups(nlocal, nwcon_, rowp, cols, &gm));
  if (ctx->size > 1) {  // all ranks or none (the two paths issue different reductions): collective
    double flag = rec ? 1.0 : 0.0;
    PO_TRY(comm_allreduce_host(ctx, &flag, 1, 1));
    rec = flag != 0.0;
  }
  CsrSparse *m = new CsrSparse(ctx, nlocal, nwcon_);
  m->dense_min_rows = dense_min_rows;
  m->factor_kind = sparse_factor_kind;
  int rc = rec ? m->setPatternLight(rowp, cols) : m->setPattern(rowp, cols);
  if (rc != PO_OK) {
    delete m;
    return rc;
  }
  delete csr;
  csr = m;
  PO_TRY(agreeDenseForm());
  nwcon = nwcon_;
  nwinequality = nwineq_;
  grouped = rec;
  gmap = rec ? gm : GroupMap();
  group_alpha = 0.0;  // known after the first gradient evaluation (csrValuesChanged)
  return chooseSolver(userSolverTable(), nwblock);
}

int Problem::csrValuesChanged() {
  if (!csr) return PO_OK;
  if (!grouped) return csr->valuesChanged();
  // every entry the same value?  {min, max} over the nnz values the user just wrote (one pass + host result)
  double mm[2] = {0.0, 0.0};
  PO_TRY(k_minmax(ctx, csr->data, csr->nnz, mm));  // over all ranks: every rank takes the same decision
  if (mm[0] > mm[1]) {  // no entries anywhere
    group_alpha = 0.0;
    return PO_OK;
  }
  if (mm[0] == mm[1]) {
    group_alpha = mm[0];
    return PO_OK;
  }
  // not the uniform weighting pattern after all: the general path from here on (analysis of the pattern once, device
  // sparse Cholesky), with the values already written
  if (ctx->rank == 0 && csr_group_fallbacks == 0)
    fprintf(stderr, "paropt_amd: the sparse Jacobian has the grouped pattern but entries in [%g, %g]: general CSR path\n",
            mm[0], mm[1]);
  csr_group_fallbacks++;
  grouped = false;
  gmap = GroupMap();
  // (mid-run, inside a gradient evaluation: whatever the interior point built with the grouped solver stands until
  // its next setUpKKTSystem rebuilds it)
  PO_TRY(csr->upgradeFromLight());
  PO_TRY(agreeDenseForm());
  PO_TRY(chooseSolver(userSolverTable(), nwblock));
  return csr->valuesChanged();
}

int Problem::agreeDenseForm() {
  double flag = csr && csr->ndense() > 0 ? 1.0 : 0.0;
  if (ctx->size > 1) PO_TRY(comm_allreduce_host(ctx, &flag, 1, 2));  // any rank
  csr_dense_form = flag != 0.0;
  return PO_OK;
}
Problem::Problem(Ctx *c, int64_t nlocal_, int ncon_, int nineq_)
    : ctx(c), nlocal(nlocal_), offset(0), nglobal(nlocal_), ncon(ncon_), ninequality(nineq_) {
  (void)chooseSolver(nullptr, 1);  // (the generic scalar form allocates nothing)
}
Problem::Problem(const Problem *like) : Problem(like->ctx, like->nlocal, like->ncon, like->ninequality) {
  offset = like->offset;
  nglobal = like->nglobal;
  nwcon = like->nwcon;
  nwinequality = like->nwinequality;
}
Problem::~Problem() {
  delete solver;
  delete csr;
}

int Problem::setSparseBlockSize(int nwblock_) {
  if (nwblock_ < 1 || nwblock_ > 16 || (nwcon % nwblock_) != 0 || csr) {
    set_error("sparse block size %d: must be 1..16, divide the %lld local sparse constraints, and the problem must "
              "not be in the CSR form", nwblock_, (long long)nwcon);
    return PO_ERR_ARG;
  }
  // (the packed-block solver allocates first and is committed on success: a failure leaves the problem in its
  // previous, consistent, state)
  return chooseSolver(userSolverTable(), nwblock_);
}
int Problem::sparseFactorFromSlacks(Vec *x, Vec *d, const WVars &v, Vec *cw) {
  if (sparseFusedForms()) return sparseSolver(&x)->factorFromSlacks(x, d, v, cw);
  PO_TRY(k_w_cdiag(ctx, v, nwcon, cw->d));
  return sparseFactor(x, d, cw);
}
int Problem::sparseFactorChecked(Vec *x, Vec *d, Vec *cw) {
  QuasiDefSolver *s = sparseSolver(&x);
  const long before = s->breakdowns();
  PO_TRY(s->factor(x, d, cw));
  if (s->breakdowns() == before) return PO_OK;
  s->describeBreakdown();
  return PO_ERR_NUMERIC;
}
// ParOptSparseProblem::evalSparseCon copies the values the last evaluation stored (.cpp:750-760)
int Problem::evalSparseCon(Vec *, Vec *out) {
  if (!csr) return 0;
  return k_copy(ctx, out->d, csr->cw->d, nwcon) != PO_OK;
}
int Problem::addSparseJacobian(double alpha, Vec *, Vec *px, Vec *out) {  // .cpp:762-788
  if (grouped) return k_group_sum(ctx, gmap, out->d, 1, 0.0, alpha * group_alpha, px->d);
  if (!csr) return 0;
  return csr->spmv(alpha, px->d, out->d) != PO_OK;
}
int Problem::setSparseJacobianTranspose(double alpha, Vec *x, Vec *pzw, Vec *out) {
  if (grouped) return k_group_scatter_set(ctx, gmap, out->d, alpha * group_alpha, pzw->d, nlocal);
  PO_TRY(k_fill(ctx, out->d, out->n, 0.0));
  return addSparseJacobianTranspose(alpha, x, pzw, out) != 0 ? PO_ERR_USER : PO_OK;
}
int Problem::addSparseJacobianTranspose(double alpha, Vec *, Vec *pzw, Vec *out) {  // .cpp:790-816
  if (grouped) return k_group_scatter(ctx, gmap, out->d, alpha * group_alpha, pzw->d, nlocal);
  if (!csr) return 0;
  return csr->spmvT(alpha, pzw->d, out->d) != PO_OK;
}
int Problem::setSparseJacobian(double alpha, Vec *x, Vec *px, Vec *out) {
  // out = alpha Aw px = alpha group_alpha (group sums of px), every entry written
  if (grouped) return k_group_sum(ctx, gmap, out->d, 0, 0.0, alpha * group_alpha, px->d);
  PO_TRY(k_fill(ctx, out->d, nwcon, 0.0));
  return addSparseJacobian(alpha, x, px, out) != 0 ? PO_ERR_USER : PO_OK;
}
int Problem::addSparseInnerProduct(double alpha, Vec *, Vec *cvec, Vec *A) {
  if (grouped) return k_group_sum(ctx, gmap, A->d, 1, 0.0, alpha * (group_alpha * group_alpha), cvec->d);
  if (!csr) return 0;
  return csr->innerProduct(alpha, cvec->d, A->d) != PO_OK;
}
int Problem::sparseGramProduct(Vec *x, Vec *d, const double *const *P, int m, double *const *U, double *const *Yw,
                               Vec *cw, Vec *work, bool panel_done, bool may_defer, double *W2, bool *cross) {
  if (!panel_done) PO_TRY(sparseJacobianPanel(x, d, P, m, U, work));
  const double *weights = nullptr;
  PO_TRY(sparseGramSolve(P, m, U, Yw, cw, work, &weights));
  *cross = weights == nullptr;
  std::vector<const double *> Uc(U, U + m);
  if (*cross) {
    std::vector<const double *> Yc(Yw, Yw + m);
    return k_xgram(ctx, Uc.data(), Yc.data(), m, nwcon, W2, may_defer);
  }
  return k_wgram(ctx, weights, Uc.data(), m, nwcon, W2, nullptr, nullptr, 0, 0.0, 0, may_defer);
}

int Problem::sparsePanelImage(Vec *x, Vec *d, const double *const *P, int nv, double *const *U, Vec *work) {
  if (grouped) return k_group_panel(ctx, gmap, P, nv, d->d, group_alpha, U);
  for (int j = 0; j < nv; j++) {
    PO_TRY(k_mul(ctx, work->d, 1.0, d->d, P[j], nlocal));
    PO_TRY(k_fill(ctx, U[j], nwcon, 0.0));
    BorrowedVec u(ctx, nwcon, U[j]);
    if (addSparseJacobian(1.0, x, work, &u) != 0) return PO_ERR_USER;
  }
  return PO_OK;
}

int Problem::checkGradients(double dh, Vec *x, bool check_hvec, Vec *xt, Vec *px, std::string *report) {
  const int64_t n = nlocal;
  Vec *g = vec_new(ctx, n), *gt = vec_new(ctx, n);
  std::vector<Vec *> A, At;
  bool ok = g && gt;
  for (int j = 0; ok && j < ncon; j++) {
    A.push_back(vec_new(ctx, n));
    At.push_back(vec_new(ctx, n));
    ok = A.back() && At.back();
  }
  int rc = ok ? PO_OK : PO_ERR_HIP;
  auto run = [&]() -> int {
    double f0 = 0.0, f1 = 0.0;
    std::vector<double> c0(ncon > 0 ? ncon : 1, 0.0), c1(c0), Ap(c0);
    if (evalObjCon(x, &f0, c0.data()) != 0 || evalObjConGradient(x, g, A.data()) != 0) return PO_ERR_USER;
    PO_TRY(k_sign(ctx, px->d, g->d, n));  // p_i = +1 where g_i >= 0, else -1
    double gp = 0.0;
    PO_TRY(k_reduce1(ctx, RED_DOT, g->d, px->d, n, &gp));
    std::vector<const double *> ap;
    for (Vec *v : A) ap.push_back(v->d);
    if (ncon > 0) PO_TRY(k_mdot(ctx, px->d, ap.data(), ncon, n, Ap.data()));
    const double one[1] = {dh};
    const double *pv[1] = {px->d};
    PO_TRY(k_panel_axpy(ctx, xt->d, 1.0, x->d, 0.0, one, pv, 1, n));
    if (evalObjCon(xt, &f1, c1.data()) != 0) return PO_ERR_USER;
    char line[256];
    auto row = [&](const char *what, int idx, double actual, double fd) {
      const double err = fabs(actual - fd), rel = err / (fabs(actual) > 1e-300 ? fabs(actual) : 1.0);
      if (idx < 0) {
        snprintf(line, sizeof(line), "%s\n%15s %15s %15s %15s\n%15.6e %15.6e %15.4e %15.4e\n", what, "Actual", "FD",
                 "Err", "Rel err", actual, fd, err, rel);
      } else {
        snprintf(line, sizeof(line), "%s[%d]\n%15.6e %15.6e %15.4e %15.4e\n", what, idx, actual, fd, err, rel);
      }
      *report += line;
    };
    *report += "\nGradient check (forward differences along sign(g))\n";
    row("Objective gradient test", -1, gp, (f1 - f0) / dh);
    for (int j = 0; j < ncon; j++) row("Constraint gradient test", j, Ap[j], (c1[j] - c0[j]) / dh);
    if (check_hvec) {
      std::vector<double> z(ncon > 0 ? ncon : 1, 0.0), mz(z);
      for (int j = 0; j < ncon; j++) {
        z[j] = 2.3 - 0.15 * (j % 5);
        mz[j] = -z[j];
      }
      if (evalObjConGradient(xt, gt, At.data()) != 0) return PO_ERR_USER;
      std::vector<const double *> atp;
      for (Vec *v : At) atp.push_back(v->d);
      // Lagrangian gradients g - sum z_j A_j (the sparse constraints of the built-in problems are linear or
      // enter through zw = 0 here)
      PO_TRY(k_panel_axpy(ctx, g->d, 0.0, nullptr, 1.0, mz.data(), ap.data(), ncon, n));
      PO_TRY(k_panel_axpy(ctx, gt->d, 0.0, nullptr, 1.0, mz.data(), atp.data(), ncon, n));
      if (evalHvecProduct(x, z.data(), nullptr, px, xt) == 0) {
        PO_TRY(k_axpy(ctx, gt->d, -1.0, g->d, n));
        PO_TRY(k_scale(ctx, gt->d, n, 1.0 / dh));
        double hp = 0.0, fp = 0.0;
        PO_TRY(k_reduce1(ctx, RED_DOT, xt->d, px->d, n, &hp));
        PO_TRY(k_reduce1(ctx, RED_DOT, gt->d, px->d, n, &fp));
        row("Hessian-vector product test (p^T H p)", -1, hp, fp);
      } else {
        *report += "Hessian-vector products are not implemented by this problem\n";
      }
    }
    return PO_OK;
  };
  if (rc == PO_OK) rc = run();
  vec_decref(g);
  vec_decref(gt);
  for (Vec *v : A) vec_decref(v);
  for (Vec *v : At) vec_decref(v);
  return rc;
}

bool Problem::sparseTransposeColumn(double alpha, Vec *x, Vec *pzw, GroupCol *col) {
  if (sparseUserSolver() || !grouped || nwcon <= 0 || gmap.start != 0 || nlocal >= 2000000000LL) return false;
  col->w = pzw->d;
  col->scale = alpha * group_alpha;  // the value k_group_scatter_set(..., alpha * group_alpha, ...) stores
  col->period = (unsigned)(gmap.nw + gmap.skip);
  col->nw = (unsigned)gmap.nw;
  col->nwcon = gmap.nwcon;
  return true;
}
bool Problem::sparseGramGroups(Vec *x, GramGroups *g) {
  if (sparseUserSolver() || !grouped || nwcon <= 0) return false;
  g->nwcon = gmap.nwcon;
  g->start = gmap.start;
  g->nw = gmap.nw;
  g->skip = gmap.skip;
  g->alpha = group_alpha;  // as in sparseJacobianPanel
  return true;
}

// ---- callbacks --------------------------------------------------------------------------------
int CallbackProblem::getVarsAndBounds(Vec *x, Vec *lb, Vec *ub) {
  if (!cb.get_vars_and_bounds) {
    set_error("problem callbacks lack get_vars_and_bounds");
    return PO_ERR_ARG;
  }
  int rc = cb.get_vars_and_bounds(cb.user, static_cast<po_vec>(x), static_cast<po_vec>(lb),
                                  static_cast<po_vec>(ub));
  return rc;
}
int CallbackProblem::evalObjCon(Vec *x, double *fobj, double *cons) {
  if (csr) {  // ParOptSparseProblem::evalObjCon (.cpp:724-727)
    if (!csr_obj_con) return 1;
    return csr_obj_con(cb.user, static_cast<po_vec>(x), fobj, cons, static_cast<po_vec>(csr->cw));
  }
  return cb.eval_obj_con(cb.user, static_cast<po_vec>(x), fobj, cons);
}
int CallbackProblem::evalObjConGradient(Vec *x, Vec *g, Vec **Ac) {
  std::vector<po_vec> h(ncon > 0 ? ncon : 1);
  // Ac == nullptr with ncon > 0: objective gradient only (linear_constraints); with ncon == 0 the callback still
  // receives a valid (empty) array
  const bool only_g = (Ac == nullptr && ncon > 0);
  for (int j = 0; j < ncon; j++) h[j] = Ac ? static_cast<po_vec>(Ac[j]) : nullptr;
  if (csr) {  // ParOptSparseProblem::evalObjConGradient (.cpp:739-742)
    if (!csr_gradient) return 1;
    int rc = csr_gradient(cb.user, static_cast<po_vec>(x), static_cast<po_vec>(g), only_g ? nullptr : h.data(),
                          csr->data, csr->nnz);
    if (rc != 0) return rc;
    return csrValuesChanged() != PO_OK;
  }
  return cb.eval_obj_con_gradient(cb.user, static_cast<po_vec>(x), static_cast<po_vec>(g),
                                  only_g ? nullptr : h.data());
}
int CallbackProblem::computeQuasiNewtonUpdateCorrection(Vec *x, const double *z, Vec *s, Vec *y) {
  if (!cb.qn_update_correction) return 0;
  return cb.qn_update_correction(cb.user, static_cast<po_vec>(x), z, static_cast<po_vec>(s),
                                 static_cast<po_vec>(y));
}
int CallbackProblem::writeOutput(int iter, Vec *x) {
  if (!cb.write_output) return 0;
  return cb.write_output(cb.user, iter, static_cast<po_vec>(x));
}

int CallbackProblem::evalSparseCon(Vec *x, Vec *out) {
  if (csr) return Problem::evalSparseCon(x, out);
  if (!sparse.set || !sparse.cb.eval_sparse_con) return nwcon > 0 ? 1 : 0;
  return sparse.cb.eval_sparse_con(cb.user, static_cast<po_vec>(x), static_cast<po_vec>(out));
}
int CallbackProblem::addSparseJacobian(double alpha, Vec *x, Vec *px, Vec *out) {
  if (csr) return Problem::addSparseJacobian(alpha, x, px, out);
  if (!sparse.set || !sparse.cb.add_sparse_jacobian) return nwcon > 0 ? 1 : 0;
  return sparse.cb.add_sparse_jacobian(cb.user, alpha, static_cast<po_vec>(x),
                                       static_cast<po_vec>(px), static_cast<po_vec>(out));
}
int CallbackProblem::addSparseJacobianTranspose(double alpha, Vec *x, Vec *pzw, Vec *out) {
  if (csr) return Problem::addSparseJacobianTranspose(alpha, x, pzw, out);
  if (!sparse.set || !sparse.cb.add_sparse_jacobian_transpose) return nwcon > 0 ? 1 : 0;
  return sparse.cb.add_sparse_jacobian_transpose(cb.user, alpha, static_cast<po_vec>(x),
                                                 static_cast<po_vec>(pzw), static_cast<po_vec>(out));
}
int CallbackProblem::addSparseInnerProduct(double alpha, Vec *x, Vec *cvec, Vec *A) {
  if (csr) return Problem::addSparseInnerProduct(alpha, x, cvec, A);
  if (!sparse.set || !sparse.cb.add_sparse_inner_product) return nwcon > 0 ? 1 : 0;
  return sparse.cb.add_sparse_inner_product(cb.user, alpha, static_cast<po_vec>(x),
                                            static_cast<po_vec>(cvec), static_cast<po_vec>(A));
}

int CallbackProblem::evalHvecProduct(Vec *x, const double *z, Vec *zw, Vec *px, Vec *hvec) {
  if (!hvec_fn) return 1;
  return hvec_fn(cb.user, static_cast<po_vec>(x), z, static_cast<po_vec>(zw), static_cast<po_vec>(px),
                 static_cast<po_vec>(hvec));
}
int CallbackProblem::evalHessianDiag(Vec *x, const double *z, Vec *zw, Vec *hdiag) {
  if (!hdiag_fn) return 1;
  return hdiag_fn(cb.user, static_cast<po_vec>(x), z, static_cast<po_vec>(zw), static_cast<po_vec>(hdiag));
}

// ---- separable workloads ----------------------------------------------------------------------
SeparableProblem::SeparableProblem(Ctx *c, int kind_, int64_t nglobal_, int ncon_, uint64_t seed_,
                                   double eig_min_, double eig_max_)
    : Problem(c, 0, kind_ == PO_PROBLEM_ROSENBROCK ? 2 : ncon_,
              kind_ == PO_PROBLEM_ROSENBROCK ? 2 : ncon_),
      kind(kind_), seed(seed_), eig_min(eig_min_), eig_max(eig_max_), q(nullptr), b(nullptr) {
  nglobal = nglobal_;
  shard(nglobal_, c->rank, c->size, &nlocal, &offset);
}

SeparableProblem::~SeparableProblem() {
  vec_decref(chain_tmp);
  vec_decref(q);
  vec_decref(b);
  for (Vec *v : A) vec_decref(v);
}

int SeparableProblem::init() {
  const int64_t n = nlocal;
  beta.assign(ncon, 0.0);
  if (kind == PO_PROBLEM_ROSENBROCK) return PO_OK;
  b = vec_new(ctx, n);
  if (!b) return PO_ERR_HIP;
  PO_TRY(k_fill_hash(ctx, b->d, n, seed, 2, offset, 1.0, 0.0));
  if (kind == PO_PROBLEM_QUADRATIC) {
    q = vec_new(ctx, n);
    if (!q) return PO_ERR_HIP;
    PO_TRY(k_fill_hash(ctx, q->d, n, seed, 1, offset, eig_max - eig_min, eig_min));
  }
  for (int j = 0; j < ncon; j++) {
    Vec *a = vec_new(ctx, n);
    if (!a) return PO_ERR_HIP;
    PO_TRY(k_fill_hash(ctx, a->d, n, seed, 100 + j, offset, 1.0, 0.0));
    A.push_back(a);
  }
  if (kind == PO_PROBLEM_QUADRATIC) {
    // beta_j = u01(seed, 4, j): same hash on the host
    for (int j = 0; j < ncon; j++) {
      uint64_t z = seed * 0x9E3779B97F4A7C15ULL + 4 * 0xD1B54A32D192ED03ULL + (uint64_t)j;
      z += 0x9E3779B97F4A7C15ULL;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
      z = z ^ (z >> 31);
      beta[j] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
  } else {
    // beta_j = 0.25 * sum_i a_j[i]  (examples/random_convex/random_convex.py:110-111): the sums of
    // all rows in one pass, as dot products with a vector of ones
    Vec *ones = vec_new(ctx, n);
    if (!ones) return PO_ERR_HIP;
    PO_TRY(k_fill(ctx, ones->d, n, 1.0));
    std::vector<const double *> ap;
    for (Vec *v : A) ap.push_back(v->d);
    if (ncon > 0) PO_TRY(k_mdot(ctx, ones->d, ap.data(), ncon, n, beta.data()));
    for (int j = 0; j < ncon; j++) beta[j] *= 0.25;
    vec_decref(ones);
  }
  return PO_OK;
}

int SeparableProblem::setWeighting(int64_t nwg, int nw, int64_t nwstart, int nwskip, int64_t nwineq) {
  if (nwg < 0 || nw <= 0 || nwstart < 0 || nwskip < 0 || nwineq < 0 || nwineq > nwg) {
    set_error("setWeighting: bad arguments");
    return PO_ERR_ARG;
  }
  const int64_t period = (int64_t)nw + nwskip;
  if (nwstart + (nwg - 1) * period + nw > nglobal && nwg > 0) {
    set_error("setWeighting: groups reach past the last variable");
    return PO_ERR_ARG;
  }
  int64_t first = 0, count = nwg;  // global index of this rank's first group, number of local groups
  int64_t lstart = nwstart;
  if (ctx->size > 1) {
    // group i lives where its first variable lives; it must end on the same rank
    if (nwstart + nw > period || nlocal % period != 0 || offset % period != 0) {
      set_error("setWeighting: with %d ranks the shard size (%lld) must be a multiple of nw+nwskip",
                ctx->size, (long long)nlocal);
      return PO_ERR_ARG;
    }
    first = offset / period;
    count = nlocal / period;
    if (first > nwg) first = nwg;
    if (first + count > nwg) count = nwg - first;
  }
  gmap.nwcon = count;
  gmap.start = lstart;
  gmap.nw = nw;
  gmap.skip = nwskip;
  grouped = true;
  group_alpha = -1.0;  // Aw = -(group indicator)
  nwcon = count;
  nwinequality = nwineq - first;
  if (nwinequality < 0) nwinequality = 0;
  if (nwinequality > count) nwinequality = count;
  return chooseSolver(userSolverTable(), nwblock);
}
int SeparableProblem::setChain(int span, int stride, int reverse_cols, int dense_vars) {
  if (span < 1 || stride < 1 || dense_vars < 0 || dense_vars > nlocal) {
    set_error("setChain: span and stride must be positive, the dense variables between 0 and the local size");
    return PO_ERR_ARG;
  }
  const int64_t nchain = nlocal - dense_vars, len = span + dense_vars;
  const int64_t rows = nchain >= span ? (nchain - span) / stride + 1 : 0;
  if (rows * len > 2000000000LL) {
    set_error("setChain: more than 2e9 Jacobian entries on one rank");
    return PO_ERR_ARG;
  }
  std::vector<int> rowp(rows + 1), cols((size_t)rows * len);
  for (int64_t i = 0; i < rows; i++) {
    rowp[i] = (int)(i * len);
    for (int k = 0; k < span; k++) {
      cols[i * len + (reverse_cols ? span - 1 - k : k)] = (int)(i * stride + k);
    }
    for (int j = 0; j < dense_vars; j++) cols[i * len + span + j] = (int)(nchain + j);
  }
  rowp[rows] = (int)(rows * len);
  PO_TRY(setSparseJacobianData(rows, rows, rowp.data(), cols.data()));
  chain_span = span;
  chain_stride = stride;
  chain_reverse = reverse_cols;
  chain_dense = dense_vars;
  // (gmap is setSparseJacobianData's: a chain with stride >= span has row-disjoint groups, is recognised as the grouped
  // pattern and runs the group kernels for as long as its Jacobian entries -2 x are uniform -- a start at x = -1, say.
  // Until round 5's random campaign this function reset gmap behind the recognition: `grouped` with an empty map.)
  return PO_OK;
}
int SeparableProblem::evalSparseCon(Vec *x, Vec *out) {
  if (csr) return Problem::evalSparseCon(x, out);
  return k_group_sum(ctx, gmap, out->d, 0, 1.0, -1.0, x->d);  // cw_i = 1 - sum of the group
}
// Hessian of the Lagrangian f - z^T c - zw^T cw.  The weighting constraints are linear; a chain constraint
// cw_i = 1 - sum x^2 adds 2 zw_i on the diagonal entries of its variables.
int SeparableProblem::chainHessian(Vec *zw, Vec *px, Vec *h) {
  if (!csr || !zw) return PO_OK;
  if (!chain_tmp) chain_tmp = vec_new(ctx, nlocal);
  if (!chain_tmp) return PO_ERR_HIP;
  // a recognised chain (stride >= span, uniform entries) keeps the light pattern: no transposed index on the device.
  // Its rows are the groups of gmap, so the column sums are the group scatter (same value per entry: 2 zw_g).
  if (grouped || csr->light)
    PO_TRY(k_group_scatter_set(ctx, gmap, chain_tmp->d, 2.0, zw->d, nlocal));
  else
    PO_TRY(csr->colSum(2.0, zw->d, chain_tmp->d));
  if (px) PO_TRY(k_mul(ctx, chain_tmp->d, 1.0, chain_tmp->d, px->d, nlocal));
  return k_axpy(ctx, h->d, 1.0, chain_tmp->d, nlocal);
}
int SeparableProblem::evalHvecProduct(Vec *x, const double *z, Vec *zw, Vec *px, Vec *hvec) {
  if (kind == PO_PROBLEM_ROSENBROCK) {
    if (k_rosen_hess(ctx, x->d, z[0], px->d, nlocal, hvec->d) != PO_OK) return 1;
  } else if (k_sep_hess(ctx, kind == PO_PROBLEM_QUADRATIC ? 0 : 1, q ? q->d : nullptr, b->d, x->d, px->d, nlocal,
                        hvec->d) != PO_OK) {
    return 1;
  }
  return chainHessian(zw, px, hvec) != PO_OK;
}
int SeparableProblem::evalHessianDiag(Vec *x, const double *z, Vec *zw, Vec *hdiag) {
  if (kind == PO_PROBLEM_ROSENBROCK) {
    if (k_rosen_hess(ctx, x->d, z[0], nullptr, nlocal, hdiag->d) != PO_OK) return 1;
  } else if (k_sep_hess(ctx, kind == PO_PROBLEM_QUADRATIC ? 0 : 1, q ? q->d : nullptr, b->d, x->d, nullptr,
                        nlocal, hdiag->d) != PO_OK) {
    return 1;
  }
  return chainHessian(zw, nullptr, hdiag) != PO_OK;
}

int SeparableProblem::getVarsAndBounds(Vec *x, Vec *lb, Vec *ub) {
  const int64_t n = nlocal;
  if (kind == PO_PROBLEM_QUADRATIC) {
    PO_TRY(k_fill_hash(ctx, x->d, n, seed, 3, offset, 1.0, -2.0));
    PO_TRY(k_fill(ctx, lb->d, n, -5.0));
    PO_TRY(k_fill(ctx, ub->d, n, 5.0));
  } else if (kind == PO_PROBLEM_CONVEX) {
    PO_TRY(k_fill_hash(ctx, x->d, n, seed, 3, offset, 0.9, 0.05));
    PO_TRY(k_fill(ctx, lb->d, n, 0.0));
    PO_TRY(k_fill(ctx, ub->d, n, 1.0));
  } else {
    PO_TRY(k_fill(ctx, x->d, n, -1.0));
    PO_TRY(k_fill(ctx, lb->d, n, -2.0));
    PO_TRY(k_fill(ctx, ub->d, n, 1.0));
  }
  return k_bounds_mode(ctx, x->d, lb->d, ub->d, bounds_mode, offset, n);
}

int SeparableProblem::evalObjCon(Vec *x, double *fobj, double *cons) {
  const int64_t n = nlocal;
  if (csr && chain_dense > 0) {
    PO_TRY(k_chain_dense_con(ctx, x->d, nwcon, chain_span, chain_stride, x->d + (nlocal - chain_dense), chain_dense,
                             csr->cw->d));
  } else if (csr) {
    PO_TRY(k_chain_con(ctx, x->d, nwcon, chain_span, chain_stride, csr->cw->d));
  }
  if (kind == PO_PROBLEM_ROSENBROCK) {
    BatchScope batch(ctx);
    PO_TRY(k_rosen_f(ctx, x->d, n, rosen_out));
    return batch.end_then([this, fobj, cons] {
      *fobj = rosen_out[0];
      cons[0] = rosen_out[1] + 0.25;
      cons[1] = rosen_out[2] + 10.0;
    });
  }
  // objective sum and constraint products share one collective + host sync (and the caller's, if it has
  // reductions queued: the line search's barrier sums at the trial point)
  BatchScope batch(ctx);
  if (kind == PO_PROBLEM_QUADRATIC) {
    PO_TRY(k_quadratic_f(ctx, q->d, b->d, x->d, n, fobj));
  } else {
    PO_TRY(k_convex_f(ctx, b->d, x->d, n, fobj));
  }
  std::vector<const double *> ap;
  for (Vec *v : A) ap.push_back(v->d);
  if (ncon > 0) PO_TRY(k_mdot(ctx, x->d, ap.data(), ncon, n, cons));
  return batch.end_then([this, cons] {
    for (int j = 0; j < ncon; j++) {
      cons[j] = (kind == PO_PROBLEM_QUADRATIC) ? cons[j] + beta[j] : -cons[j] + beta[j];
    }
  });
}

int SeparableProblem::evalObjConGradient(Vec *x, Vec *g, Vec **Ac) {
  const int64_t n = nlocal;
  if (csr) {
    if (chain_dense > 0) {
      PO_TRY(k_chain_dense_jac(ctx, x->d, nwcon, chain_span, chain_stride, chain_reverse,
                               x->d + (nlocal - chain_dense), chain_dense, csr->data));
    } else {
      PO_TRY(k_chain_jac(ctx, x->d, nwcon, chain_span, chain_stride, chain_reverse, csr->data));
    }
    PO_TRY(csrValuesChanged());
  }
  if (kind == PO_PROBLEM_ROSENBROCK) {
    if (!Ac) return 1;  // nonlinear constraints: the flag must not be set
    return k_rosen_g(ctx, x->d, n, g->d, Ac[0]->d, Ac[1]->d);
  }
  if (kind == PO_PROBLEM_QUADRATIC) {
    PO_TRY(k_quadratic_g(ctx, q->d, b->d, x->d, n, g->d));
  } else {
    PO_TRY(k_convex_g(ctx, b->d, x->d, n, g->d));
  }
  // the constraint Jacobian is rewritten at every gradient evaluation, as the reference's example
  // problems do (examples/random_convex/random_convex.py:67-71): Ac_j = +-a_j, one launch
  std::vector<double *> dst;
  std::vector<const double *> src;
  for (int j = 0; j < ncon && Ac; j++) {
    dst.push_back(Ac[j]->d);
    src.push_back(A[j]->d);
  }
  if (ncon > 0 && Ac) {
    PO_TRY(k_panel_lincomb(ctx, dst.data(), kind == PO_PROBLEM_QUADRATIC ? 1.0 : -1.0, src.data(), 0.0,
                           nullptr, ncon, n));
  }
  return PO_OK;
}

}  // namespace po
