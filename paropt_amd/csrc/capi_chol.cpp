// C ABI of the multifrontal sparse Cholesky (include/paropt_amd.h, "ParOptSparseCholesky"); each entry names the line
// of the reference's src/ParOptSparseCholesky.h it stands for.
#include "sparse_chol.hpp"

using namespace po;

#define PO_CHECK_PTR(p)                         \
  do {                                          \
    if (!(p)) {                                 \
      po::set_error("null argument: %s", #p);   \
      return PO_ERR_ARG;                        \
    }                                           \
  } while (0)

struct po_sparse_chol_s {
  po::SparseChol *c;
  int form_counts[po::CHF_COUNT + po::CHF_SCHUR_COUNT];
};

#define PO_CHECK_NUMERIC(h)                                                                         \
  do {                                                                                              \
    PO_CHECK_PTR(h);                                                                                \
    if (!(h)->c->ctx) {                                                                             \
      po::set_error("sparse Cholesky: an analysis-only handle (created with ctx == NULL) has no numeric part"); \
      return PO_ERR_ARG;                                                                            \
    }                                                                                               \
  } while (0)

extern "C" {

// ParOptSparseCholesky::ParOptSparseCholesky, ParOptSparseCholesky.h:31-33
int po_sparse_chol_create(po_ctx ctx, int64_t size, const int *colp, const int *rows, int order, const int *perm,
                          po_sparse_chol *out) {
  PO_CHECK_PTR(out);
  *out = nullptr;
  PO_CHECK_PTR(colp);
  po::SparseChol *c = new po::SparseChol(ctx);
  int rc = po::chol_analyse(size, colp, rows, order, perm, &c->sym);
  if (rc == PO_OK && ctx) rc = c->upload();
  if (rc != PO_OK) {
    delete c;
    return rc;
  }
  *out = new po_sparse_chol_s{c, {}};
  return PO_OK;
}
// no counterpart in the reference: partial factorization with a Schur complement (paropt_amd.h, "SCHUR COMPLEMENT")
int po_sparse_chol_create_schur(po_ctx ctx, int64_t size, const int *colp, const int *rows, int order, const int *perm,
                                int64_t nschur, const int *schur, po_sparse_chol *out) {
  PO_CHECK_PTR(out);
  *out = nullptr;
  PO_CHECK_PTR(colp);
  if (nschur > 0) PO_CHECK_PTR(schur);
  po::SparseChol *c = new po::SparseChol(ctx);
  int rc = po::chol_analyse(size, colp, rows, order, perm, nschur, schur, &c->sym);
  if (rc == PO_OK && ctx) rc = c->upload();
  if (rc != PO_OK) {
    delete c;
    return rc;
  }
  *out = new po_sparse_chol_s{c, {}};
  return PO_OK;
}
int po_sparse_chol_schur_info(po_sparse_chol h, int64_t info[4]) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(info);
  const po::CholSymbolic &s = h->c->sym;
  info[0] = s.ns;
  info[1] = s.schur_sn;
  info[2] = s.schur_sn >= 0 ? s.child_ptr[s.schur_sn + 1] - s.child_ptr[s.schur_sn] : 0;
  info[3] = (int64_t)s.schur_src.size();
  return PO_OK;
}
int po_sparse_chol_schur_indices(po_sparse_chol h, const int **schur) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(schur);
  *schur = h->c->sym.schur.data();
  return PO_OK;
}
int po_sparse_chol_get_schur(po_sparse_chol h, double *S, int64_t lds) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.ns > 0) PO_CHECK_PTR(S);
  return h->c->getSchurHost(S, lds);
}
int po_sparse_chol_get_schur_device(po_sparse_chol h, double *dS, int64_t lds) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.ns > 0) PO_CHECK_PTR(dS);
  return h->c->getSchurDevice(dS, lds);
}
int po_sparse_chol_solve_condense(po_sparse_chol h, double *x, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(x);
  return h->c->condenseHost(x, nrhs, ldx);
}
int po_sparse_chol_solve_condense_device(po_sparse_chol h, double *dx, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(dx);
  return h->c->condenseDevice(dx, nrhs, ldx);
}
int po_sparse_chol_solve_expand(po_sparse_chol h, double *x, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(x);
  return h->c->expandHost(x, nrhs, ldx);
}
int po_sparse_chol_solve_expand_device(po_sparse_chol h, double *dx, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(dx);
  return h->c->expandDevice(dx, nrhs, ldx);
}
int po_sparse_chol_schur_assembly_probe(po_sparse_chol h, int chunked, int reps) {
  PO_CHECK_NUMERIC(h);
  return h->c->schurAssemblyProbe(chunked != 0, reps);
}
// no counterpart in the reference: factoring and solving with S on the device (paropt_amd.h, "FACTORED SCHUR COMPLEMENT")
int po_sparse_chol_schur_factor(po_sparse_chol h, const double *add, int64_t ldadd, int *info) {
  PO_CHECK_NUMERIC(h);
  return h->c->schurFactorHost(add, ldadd, info);
}
int po_sparse_chol_schur_factor_device(po_sparse_chol h, const double *dadd, int64_t ldadd, int *info) {
  PO_CHECK_NUMERIC(h);
  return h->c->schurFactorDevice(dadd, ldadd, info);
}
int po_sparse_chol_schur_solve(po_sparse_chol h, double *x2, int nrhs, int64_t ldx2) {
  PO_CHECK_NUMERIC(h);
  if (h->c->schurFactored() && nrhs > 0) PO_CHECK_PTR(x2);
  return h->c->schurSolveHost(x2, nrhs, ldx2);
}
int po_sparse_chol_schur_solve_device(po_sparse_chol h, double *dx2, int nrhs, int64_t ldx2) {
  PO_CHECK_NUMERIC(h);
  if (h->c->schurFactored() && nrhs > 0) PO_CHECK_PTR(dx2);
  return h->c->schurSolveDevice(dx2, nrhs, ldx2);
}
int po_sparse_chol_schur_inertia(po_sparse_chol h, int64_t inertia[3]) {
  PO_CHECK_NUMERIC(h);
  PO_CHECK_PTR(inertia);
  return h->c->schurInertia(inertia);
}
int po_sparse_chol_schur_solve_info(po_sparse_chol h, int64_t info[4]) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(info);
  info[0] = h->c->sym.schur_w;
  info[1] = po::chol_schur_solve_launches(h->c->sym);
  info[2] = h->c->schurFactorBytes();
  info[3] = h->c->schurFactored() ? 1 : 0;
  return PO_OK;
}
// setValues, ParOptSparseCholesky.h:37-38
int po_sparse_chol_set_values(po_sparse_chol h, int64_t n, const int *colp, const int *rows, const double *vals) {
  PO_CHECK_NUMERIC(h);
  PO_CHECK_PTR(colp);
  if (n == h->c->sym.n && n >= 0 && colp[n] > 0) {
    PO_CHECK_PTR(rows);
    PO_CHECK_PTR(vals);
  }
  return h->c->setValuesHost(n, colp, rows, vals);
}
int po_sparse_chol_set_values_device(po_sparse_chol h, const double *dvals) {
  PO_CHECK_NUMERIC(h);
  if (!h->c->sym.rows.empty()) PO_CHECK_PTR(dvals);
  return h->c->setValuesDevice(dvals);
}
// factor, ParOptSparseCholesky.h:41
int po_sparse_chol_factor(po_sparse_chol h, int *info) {
  PO_CHECK_NUMERIC(h);
  return h->c->factor(info);
}
// no counterpart in the reference: L S L^T for quasi-definite matrices (paropt_amd.h, "FACTORIZATION KIND")
int po_sparse_chol_set_factorization(po_sparse_chol h, int kind) {
  PO_CHECK_PTR(h);
  return h->c->setFactorization(kind);
}
int po_sparse_chol_get_factorization(po_sparse_chol h, int *kind) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(kind);
  *kind = h->c->factorization();
  return PO_OK;
}
int po_sparse_chol_inertia(po_sparse_chol h, int64_t inertia[3]) {
  PO_CHECK_NUMERIC(h);
  PO_CHECK_PTR(inertia);
  return h->c->inertia(inertia);
}
int po_sparse_chol_solve(po_sparse_chol h, double *x, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(x);
  return h->c->solveHost(x, nrhs, ldx);
}
int po_sparse_chol_solve_device(po_sparse_chol h, double *dx, int nrhs, int64_t ldx) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(dx);
  return h->c->solveDevice(dx, nrhs, ldx);
}
// no counterpart in the reference: the retained matrix, the diagonal shift and the refined solve (paropt_amd.h,
// "RETAINED MATRIX AND REFINED SOLVE")
int po_sparse_chol_set_keep_matrix(po_sparse_chol h, int on) {
  PO_CHECK_PTR(h);
  return h->c->setKeepMatrix(on != 0);
}
int po_sparse_chol_get_keep_matrix(po_sparse_chol h, int *on) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(on);
  *on = h->c->keepMatrix() ? 1 : 0;
  return PO_OK;
}
int po_sparse_chol_matrix_arrays(po_sparse_chol h, const int **rowp, const int **col, const int **vidx, int64_t *nd) {
  PO_CHECK_PTR(h);
  if (!h->c->keepMatrix()) {
    po::set_error("po_sparse_chol_matrix_arrays: keep_matrix is off, there is no table");
    return PO_ERR_ARG;
  }
  const po::CholSymbolic &s = h->c->sym;
  if (rowp) *rowp = s.mat_rowp.data();
  if (col) *col = s.mat_col.data();
  if (vidx) *vidx = s.mat_vidx.data();
  if (nd) *nd = (int64_t)s.asm_dst.size();
  return PO_OK;
}
int po_sparse_chol_set_diagonal_shift(po_sparse_chol h, const double *shift) {
  PO_CHECK_NUMERIC(h);
  return h->c->setDiagonalShift(shift);
}
int po_sparse_chol_matvec(po_sparse_chol h, const double *x, int64_t ldx, double *y, int64_t ldy, int nrhs) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) {
    PO_CHECK_PTR(x);
    PO_CHECK_PTR(y);
  }
  return h->c->matvecHost(x, ldx, y, ldy, nrhs);
}
int po_sparse_chol_matvec_device(po_sparse_chol h, const double *dx, int64_t ldx, double *dy, int64_t ldy, int nrhs) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) {
    PO_CHECK_PTR(dx);
    PO_CHECK_PTR(dy);
  }
  return h->c->matvecDevice(dx, ldx, dy, ldy, nrhs);
}
int po_sparse_chol_solve_refined(po_sparse_chol h, double *x, int nrhs, int64_t ldx, int max_steps, double tol,
                                 int *steps, double *eta0, double *eta) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(x);
  return h->c->solveRefinedHost(x, nrhs, ldx, max_steps, tol, steps, eta0, eta);
}
int po_sparse_chol_solve_refined_device(po_sparse_chol h, double *dx, int nrhs, int64_t ldx, int max_steps, double tol,
                                        int *steps, double *eta0, double *eta) {
  PO_CHECK_NUMERIC(h);
  if (h->c->sym.n > 0 && nrhs > 0) PO_CHECK_PTR(dx);
  return h->c->solveRefinedDevice(dx, nrhs, ldx, max_steps, tol, steps, eta0, eta);
}
// getInfo, ParOptSparseCholesky.h:47
int po_sparse_chol_info(po_sparse_chol h, int64_t info[8]) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(info);
  const po::CholSymbolic &s = h->c->sym;
  info[0] = s.n;
  info[1] = s.nsn;
  info[2] = s.nnzL;
  info[3] = s.nlev;
  info[4] = s.max_s;
  info[5] = s.max_front;
  info[6] = s.work_bytes;
  info[7] = po::kCholNB;
  return PO_OK;
}
int po_sparse_chol_arrays(po_sparse_chol h, const int **perm, const int **snode_first, const int **snode_parent,
                          const int **snode_level) {
  PO_CHECK_PTR(h);
  const po::CholSymbolic &s = h->c->sym;
  if (perm) *perm = s.perm.data();
  if (snode_first) *snode_first = s.sn_first.data();
  if (snode_parent) *snode_parent = s.sn_parent.data();
  if (snode_level) *snode_level = s.sn_level.data();
  return PO_OK;
}
int po_sparse_chol_packing(po_sparse_chol h, int64_t info[4], const int **group_first, const int **group_root,
                           const int **group_level, const int **front_order, const int64_t **upd_off) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(info);
  po::chol_packing(h->c->sym, info, group_first, group_root, group_level, front_order, upd_off);
  return PO_OK;
}
int po_sparse_chol_kernel_forms(po_sparse_chol h, int nv, int *count, const char *const **names, const int **levels) {
  PO_CHECK_PTR(h);
  PO_CHECK_PTR(count);
  if (nv < 1) {
    po::set_error("po_sparse_chol_kernel_forms: nv must be at least 1");
    return PO_ERR_ARG;
  }
  static const char *form_names[po::CHF_COUNT + po::CHF_SCHUR_COUNT];
  for (int f = 0; f < po::CHF_COUNT + po::CHF_SCHUR_COUNT; f++) form_names[f] = po::chol_form_name(f);
  po::chol_kernel_forms(h->c->sym, nv, h->form_counts);
  *count = po::CHF_COUNT;
  if (h->c->sym.ns > 0) {  // a handle with a Schur set: its two gather launches on top
    po::chol_schur_forms(h->c->sym, nv, h->form_counts + po::CHF_COUNT);
    *count += po::CHF_SCHUR_COUNT;
  }
  if (names) *names = form_names;
  if (levels) *levels = h->form_counts;
  return PO_OK;
}
// ~ParOptSparseCholesky, ParOptSparseCholesky.h:34
int po_sparse_chol_destroy(po_sparse_chol h) {
  if (!h) return PO_OK;
  delete h->c;
  delete h;
  return PO_OK;
}

}  // extern "C"
