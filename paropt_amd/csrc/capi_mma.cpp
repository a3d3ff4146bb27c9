// C ABI of the method of moving asymptotes (include/paropt_amd.h, "ParOptMMA"): the driver object, the views of its
// current subproblem, and the dual passes on caller vectors.
#include <initializer_list>
#include <utility>
#include <vector>

#include "mma.hpp"

using namespace po;

#define PO_CHECK_PTR(p)                         \
  do {                                          \
    if (!(p)) {                                 \
      po::set_error("null argument: %s", #p);   \
      return PO_ERR_ARG;                        \
    }                                           \
  } while (0)

struct po_mma_s {
  po::MMA *mma;
  std::vector<po_vec> p, q;  // the handle arrays po_mma_get_subproblem hands out
  std::vector<po_vec> a;     // ... and po_mma_get_linear_subproblem
};

extern "C" {

int po_mma_create(po_problem prob, po_mma *out) {
  PO_CHECK_PTR(prob);
  PO_CHECK_PTR(out);
  po_mma_s *h = new po_mma_s();
  h->mma = new MMA(prob->p);
  *out = h;
  return PO_OK;
}
int po_mma_destroy(po_mma mma) {
  if (!mma) return PO_OK;
  delete mma->mma;
  delete mma;
  return PO_OK;
}
int po_mma_set_option_str(po_mma mma, const char *name, const char *value) {
  PO_CHECK_PTR(mma);
  PO_CHECK_PTR(name);
  return mma->mma->options().set(name, value);
}
int po_mma_set_option_int(po_mma mma, const char *name, int value) {
  PO_CHECK_PTR(mma);
  PO_CHECK_PTR(name);
  return mma->mma->options().set(name, value);
}
int po_mma_set_option_float(po_mma mma, const char *name, double value) {
  PO_CHECK_PTR(mma);
  PO_CHECK_PTR(name);
  return mma->mma->options().set(name, value);
}
int po_mma_optimize(po_mma mma) {
  PO_CHECK_PTR(mma);
  return mma->mma->optimize();
}
int po_mma_get_optimized_point(po_mma mma, po_vec *x, const double **z, po_vec *zw, po_vec *zl, po_vec *zu) {
  PO_CHECK_PTR(mma);
  MMA *m = mma->mma;
  PO_TRY(m->build());
  if (x) *x = static_cast<po_vec>(m->xvec);
  if (z) *z = m->z.data();
  if (zw) *zw = static_cast<po_vec>(m->zwvec);
  if (zl) *zl = static_cast<po_vec>(m->zlvec);
  if (zu) *zu = static_cast<po_vec>(m->zuvec);
  return PO_OK;
}
int po_mma_get_asymptotes(po_mma mma, po_vec *L, po_vec *U) {
  PO_CHECK_PTR(mma);
  PO_TRY(mma->mma->build());
  if (L) *L = static_cast<po_vec>(mma->mma->Lvec);
  if (U) *U = static_cast<po_vec>(mma->mma->Uvec);
  return PO_OK;
}
int po_mma_get_state(po_mma mma, int *mma_iter, int *subproblem_iter, double *fobj, const double **cons) {
  PO_CHECK_PTR(mma);
  MMA *m = mma->mma;
  if (mma_iter) *mma_iter = m->mma_iter;
  if (subproblem_iter) *subproblem_iter = m->subproblem_iter;
  if (fobj) *fobj = m->fobj;
  if (cons) *cons = m->cons.data();
  return PO_OK;
}
int po_mma_get_last_row(po_mma mma, const double **row5) {
  PO_CHECK_PTR(mma);
  PO_CHECK_PTR(row5);
  *row5 = mma->mma->last_row;
  return PO_OK;
}
int po_mma_get_history(po_mma mma, const char **text) {
  PO_CHECK_PTR(mma);
  PO_CHECK_PTR(text);
  *text = mma->mma->history.c_str();
  return PO_OK;
}
int po_mma_set_iteration_callback(po_mma mma, po_mma_iteration_fn fn, void *user) {
  PO_CHECK_PTR(mma);
  mma->mma->iter_cb = fn;
  mma->mma->iter_cb_user = user;
  return PO_OK;
}
int po_mma_get_dual_stats(po_mma mma, int *solves, int *iterations, int *evaluations, int *last_status,
                          double *last_pg) {
  PO_CHECK_PTR(mma);
  const MmaDualStats &s = mma->mma->dual;
  if (solves) *solves = s.solves;
  if (iterations) *iterations = s.iterations;
  if (evaluations) *evaluations = s.evaluations;
  if (last_status) *last_status = s.last_status;
  if (last_pg) *last_pg = s.last_pg;
  return PO_OK;
}
int po_mma_get_subproblem(po_mma mma, po_vec *alpha, po_vec *beta, po_vec *p0, po_vec *q0, const po_vec **p,
                          const po_vec **q, const double **b) {
  PO_CHECK_PTR(mma);
  MMA *m = mma->mma;
  PO_TRY(m->build());
  if (m->linearDual()) {
    po::set_error("po_mma_get_subproblem: with mma_dual_linearized_constraints = newton the solver holds no p_i, q_i; "
                  "po_mma_get_linear_subproblem hands out the linearised subproblem");
    return PO_ERR_ARG;
  }
  if (alpha) *alpha = static_cast<po_vec>(m->alphavec);
  if (beta) *beta = static_cast<po_vec>(m->betavec);
  if (p0) *p0 = static_cast<po_vec>(m->p0vec);
  if (q0) *q0 = static_cast<po_vec>(m->q0vec);
  if (mma->p.empty()) {  // the vectors stay from build() to the destructor
    for (Vec *v : m->pivecs) mma->p.push_back(static_cast<po_vec>(v));
    for (Vec *v : m->qivecs) mma->q.push_back(static_cast<po_vec>(v));
  }
  if (p) *p = mma->p.data();
  if (q) *q = mma->q.data();
  if (b) *b = m->b.data();
  return PO_OK;
}
// the linearised subproblem of src/ParOptMMA.cpp:804-866 (use_true_mma = 0): cons + A (x - xk)
int po_mma_get_linear_subproblem(po_mma mma, po_vec *alpha, po_vec *beta, po_vec *p0, po_vec *q0, const po_vec **A,
                                 const double **cons, po_vec *xk) {
  PO_CHECK_PTR(mma);
  MMA *m = mma->mma;
  PO_TRY(m->build());
  if (alpha) *alpha = static_cast<po_vec>(m->alphavec);
  if (beta) *beta = static_cast<po_vec>(m->betavec);
  if (p0) *p0 = static_cast<po_vec>(m->p0vec);
  if (q0) *q0 = static_cast<po_vec>(m->q0vec);
  if (mma->a.empty())  // the vectors stay from build() to the destructor
    for (Vec *v : m->constraintGradients()) mma->a.push_back(static_cast<po_vec>(v));
  if (A) *A = mma->a.data();
  if (cons) *cons = m->cons.data();
  if (xk) *xk = static_cast<po_vec>(m->xvec);
  return PO_OK;
}
int po_mma_get_dual_linear_stats(po_mma mma, long *cap_hits, int *max_steps) {
  PO_CHECK_PTR(mma);
  const MmaLinearStats &s = mma->mma->linear;
  if (cap_hits) *cap_hits = s.cap_hits;
  if (max_steps) *max_steps = s.max_steps;
  return PO_OK;
}
// ---- the dual passes on caller vectors --------------------------------------------------------------------------------
namespace {
struct Columns {  // m caller vectors, the name a null entry is reported under, and the table of their device pointers
  const po_vec *v;
  const char *name;
  std::vector<const double *> *table;
};
// The argument checks of the entries below.  Each entry calls them in the order it has always checked in, so a call
// with several faults is refused for the same one as before.
struct ArgCheck {
  const char *who;
  po_ctx ctx;
  int m;
  po_vec L;  // every other vector has its layout

  static int null(const char *name) {
    po::set_error("null argument: %s", name);
    return PO_ERR_ARG;
  }
  int head(bool outputs, const double *W, const double *grad) const {  // ctx, L and the outputs of an evaluation
    if (!ctx) return null("ctx");
    if (!L) return null("L");
    if (outputs && !W) return null("W");
    if (outputs && !grad) return null("grad");
    return PO_OK;
  }
  int range(int form) const {
    if (m < 0 || m > kMmaDualMax || form < 0 || form > 2 || (form == 1 && m > kMmaDualFused)) {
      po::set_error("%s: m = %d, form = %d: m is 0..%d, form 1 covers m <= %d", who, m, form, kMmaDualMax,
                    kMmaDualFused);
      return PO_ERR_ARG;
    }
    return PO_OK;
  }
  int range() const {
    if (m < 0 || m > kMmaDualMax) {
      po::set_error("%s: m = %d outside 0..%d", who, m, kMmaDualMax);
      return PO_ERR_ARG;
    }
    return PO_OK;
  }
  int arrays(std::initializer_list<std::pair<const void *, const char *>> given) const {  // of m entries: read if m > 0
    for (const auto &a : given)
      if (m > 0 && !a.first) return null(a.second);
    return PO_OK;
  }
  int vec(po_vec v, const char *name = "v") const {  // given, on ctx, of the length of L
    if (!v) return null(name);
    if (v->ctx != ctx || v->n != L->n) {
      po::set_error("%s: vectors of different layouts", who);
      return PO_ERR_ARG;
    }
    return PO_OK;
  }
  int vectors(std::initializer_list<po_vec> vs) const {
    for (po_vec v : vs) PO_TRY(vec(v));
    return PO_OK;
  }
  int point(po_vec x, po_vec zl, po_vec zu) const {  // the optional outputs: all or none
    for (po_vec v : {x, zl, zu}) {
      if ((v != nullptr) != (x != nullptr) || (v && (v->ctx != ctx || v->n != L->n))) {
        po::set_error("%s: x, zl and zu are given together, in the layout of L", who);
        return PO_ERR_ARG;
      }
    }
    return PO_OK;
  }
  // column by column; nulls_first: the entries of one index are all checked for null before any layout of that index
  int columns(std::initializer_list<Columns> arrays, bool nulls_first) const {
    for (int i = 0; i < m; i++) {
      for (const Columns &a : arrays)
        if (nulls_first && !a.v[i]) return null(a.name);
      for (const Columns &a : arrays) PO_TRY(vec(a.v[i], a.name));
    }
    for (const Columns &a : arrays)
      for (int i = 0; i < m; i++) a.table->push_back(a.v[i]->d);
    return PO_OK;
  }
};
// form 0 is the library's choice; without a Hessian every form is the value and the gradient alone
int entry_form(int form, int m, const double *hess) {
  if (form == 0) form = m <= kMmaDualFused ? 1 : 2;
  return hess ? form : 0;
}
}  // namespace

// the dual of the linearised subproblem (gradients of :871-924 with use_true_mma = 0: the A_i themselves)
int po_mma_dual_linear_eval(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                            const po_vec *A, const double *cons, po_vec xk, const double *lambda, int form,
                            po_vec xstart_inout, double *W, double *grad, double *hess, po_vec x, po_vec zl,
                            po_vec zu, double *stats) {
  const ArgCheck ck{"po_mma_dual_linear_eval", ctx, m, L};
  std::vector<const double *> cols;
  PO_TRY(ck.head(true, W, grad));
  PO_TRY(ck.range(form));
  PO_TRY(ck.arrays({{A, "A"}, {cons, "cons"}, {lambda, "lambda"}}));
  PO_TRY(ck.vectors({L, U, alpha, beta, p0, q0, xk, xstart_inout}));
  PO_TRY(ck.columns({{A, "v", &cols}}, false));
  PO_TRY(ck.point(x, zl, zu));
  const MmaDualLinear s{L->d, U->d, alpha->d, beta->d, p0->d, q0->d, xk->d, cols.data(), cons, m, L->n};
  form = entry_form(form, m, hess);
  WorkVecs work(ctx);  // the panel form's weights
  if (form == 2) PO_TRY(work.add(1, L->n));
  MmaLinearStats st;
  int rc = k_mma_dual_linear(ctx, s, lambda, form, xstart_inout->d, xstart_inout->d, W, grad, hess,
                             form == 2 ? work.d(0) : nullptr, &st);
  if (rc == PO_OK && x) rc = k_mma_dual_linear_point(ctx, s, lambda, xstart_inout->d, x->d, zl->d, zu->d, &st);
  rc = work.release(rc);
  if (rc == PO_OK && stats) {
    stats[0] = (double)st.cap_hits;
    stats[1] = (double)st.max_steps;
  }
  return rc;
}
// ---- the dual of a subproblem given by caller vectors ---------------------------------------------------------------
namespace {
struct DualVectors {  // the subproblem: six vectors of one layout and the m column pairs
  po_vec L, U, alpha, beta, p0, q0;
  const po_vec *p, *q;
};
enum DualPass { EVAL, EVAL_RHO, POINT };
struct DualCall {
  const char *who;
  DualPass pass;
  po_ctx ctx;
  int m;
  DualVectors v;
  const double *b, *lambda;
  po_vec xk;          // EVAL_RHO, POINT
  const double *rho;  // EVAL_RHO, POINT
  int form;
  double *W, *grad, *hess, *D;  // EVAL, EVAL_RHO (D: EVAL_RHO only)
  po_vec x, zl, zu;             // EVAL (optional), POINT
  double *sums;                 // POINT
};
}  // namespace
// the shared body of po_mma_dual_eval / po_mma_dual_eval_rho / po_mma_gcmma_point: argument checks, the tables and the
// panel form's work vectors
static int mma_dual_entry(const DualCall &a) {
  const DualVectors &v = a.v;
  const int m = a.m;
  const bool with_rho = a.pass != EVAL;
  const ArgCheck ck{a.who, a.ctx, m, v.L};
  std::vector<const double *> pp, qq;
  PO_TRY(ck.head(a.pass != POINT, a.W, a.grad));
  PO_TRY(ck.range(a.form));
  PO_TRY(ck.arrays({{v.p, "p"}, {v.q, "q"}, {a.b, "b"}, {a.lambda, "lambda"}}));
  PO_TRY(ck.vectors({v.L, v.U, v.alpha, v.beta, v.p0, v.q0, with_rho ? a.xk : v.U}));
  PO_TRY(ck.point(a.x, a.zl, a.zu));
  PO_TRY(ck.columns({{v.p, "p[i]", &pp}, {v.q, "q[i]", &qq}}, true));
  const int64_t n = v.L->n;
  const MmaDualData s = mma_dual_data(v.L->d, v.U->d, v.alpha->d, v.beta->d, v.p0->d, v.q0->d, pp.data(), qq.data(),
                                      a.b, m, n);
  const MmaDualRho r{with_rho ? a.xk->d : nullptr, a.rho};
  if (a.pass == POINT) return k_mma_gcmma_point(a.ctx, s, r, a.lambda, a.x->d, a.zl->d, a.zu->d, a.sums);
  const int form = entry_form(a.form, m, a.hess);
  WorkVecs work(a.ctx);  // the panel form's columns and weights
  int rc = form == 2 ? work.add(m + 1, n) : PO_OK;
  if (rc == PO_OK) {
    const std::vector<double *> G = work.pointers(0, form == 2 ? m : 0);
    rc = k_mma_dual(a.ctx, s, a.lambda, form, a.W, a.grad, a.hess, form == 2 ? G.data() : nullptr,
                    form == 2 ? work.d(m) : nullptr, with_rho ? &r : nullptr, a.D);
  }
  if (rc == PO_OK && a.x) rc = k_mma_dual_point(a.ctx, s, a.lambda, a.x->d, a.zl->d, a.zu->d);
  return work.release(rc);
}
int po_mma_dual_eval(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                     const po_vec *p, const po_vec *q, const double *b, const double *lambda, int form, double *W,
                     double *grad, double *hess, po_vec x, po_vec zl, po_vec zu) {
  return mma_dual_entry({.who = "po_mma_dual_eval", .pass = EVAL, .ctx = ctx, .m = m,
                         .v = {L, U, alpha, beta, p0, q0, p, q}, .b = b, .lambda = lambda, .form = form, .W = W,
                         .grad = grad, .hess = hess, .x = x, .zl = zl, .zu = zu});
}
int po_mma_dual_eval_rho(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                         const po_vec *p, const po_vec *q, const double *b, const double *lambda, po_vec xk,
                         const double *rho, int form, double *W, double *grad, double *hess, double *D) {
  PO_CHECK_PTR(xk);
  PO_CHECK_PTR(rho);
  return mma_dual_entry({.who = "po_mma_dual_eval_rho", .pass = EVAL_RHO, .ctx = ctx, .m = m,
                         .v = {L, U, alpha, beta, p0, q0, p, q}, .b = b, .lambda = lambda, .xk = xk, .rho = rho,
                         .form = form, .W = W, .grad = grad, .hess = hess, .D = D});
}
int po_mma_gcmma_point(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                       const po_vec *p, const po_vec *q, const double *lambda, po_vec xk, const double *rho, po_vec x,
                       po_vec zl, po_vec zu, double *sums) {
  PO_CHECK_PTR(xk);
  PO_CHECK_PTR(rho);
  PO_CHECK_PTR(x);
  PO_CHECK_PTR(sums);
  const double none = 0.0;  // (the point pass does not read b)
  return mma_dual_entry({.who = "po_mma_gcmma_point", .pass = POINT, .ctx = ctx, .m = m,
                         .v = {L, U, alpha, beta, p0, q0, p, q}, .b = &none, .lambda = lambda, .xk = xk, .rho = rho,
                         .x = x, .zl = zl, .zu = zu, .sums = sums});
}
int po_mma_gcmma_rho_sums(po_ctx ctx, int m, po_vec L, po_vec U, po_vec g, const po_vec *A, double *sums) {
  const ArgCheck ck{"po_mma_gcmma_rho_sums", ctx, m, L};
  std::vector<const double *> cols;
  PO_TRY(ck.head(false, nullptr, nullptr));
  PO_CHECK_PTR(U);
  PO_CHECK_PTR(g);
  PO_CHECK_PTR(sums);
  PO_TRY(ck.range());
  PO_TRY(ck.arrays({{A, "A"}}));
  for (int i = 0; i < m; i++) PO_CHECK_PTR(A[i]);  // (every null column is reported before any layout)
  PO_TRY(ck.vectors({L, U, g}));
  PO_TRY(ck.columns({{A, "A[i]", &cols}}, true));
  return k_mma_gcmma_rho_sums(ctx, L->d, U->d, g->d, cols.data(), m, L->n, sums);
}
namespace {
struct GroupCall {  // po_mma_dual_group_eval / _rho (W != NULL) and po_mma_gcmma_group_point (sums != NULL)
  const char *who;
  po_ctx ctx;
  int m;
  DualVectors v;
  const double *b, *lambda;
  int64_t nwcon;
  int nw;
  int64_t start;
  int skip;
  double a;
  po_vec c;
  int64_t nwinequality;
  double gamma;
  double *W, *grad, *hess;
  po_vec x, zl, zu, zw;
  double *stats;
  po_vec xk;          // the rho form (with rho) and the point
  const double *rho;
  double *D, *sums;
};
}  // namespace
static int mma_group_entry(const GroupCall &k) {
  const DualVectors &v = k.v;
  const int m = k.m;
  const int64_t nwcon = k.nwcon;
  const bool point = k.sums != nullptr;
  const ArgCheck ck{k.who, k.ctx, m, v.L};
  const char *who = k.who;
  std::vector<const double *> pp, qq;
  PO_TRY(ck.head(!point, k.W, k.grad));
  PO_TRY(ck.range());
  PO_TRY(ck.arrays({{v.p, "p"}, {v.q, "q"}, {k.b, "b"}, {k.lambda, "lambda"}}));
  PO_TRY(ck.vectors({v.L, v.U, v.alpha, v.beta, v.p0, v.q0, k.x, k.zl, k.zu}));
  if (k.rho) PO_TRY(ck.vec(k.xk));
  PO_TRY(ck.columns({{v.p, "v", &pp}, {v.q, "v", &qq}}, false));
  const int64_t n = v.L->n;
  MmaDualGroups g;
  g.map.nwcon = nwcon;
  g.map.nw = k.nw;
  g.map.start = k.start;
  g.map.skip = k.skip;
  g.a = k.a;
  g.nwinequality = k.nwinequality;
  g.gamma = k.gamma;
  if (nwcon < 0 || (nwcon > 0 && (k.nw <= 0 || k.skip < 0 || !mma_dual_groups_tile(g.map, n))) || !(k.gamma > 0.0) ||
      k.nwinequality < 0) {
    po::set_error("%s: groups (nwcon %lld, nw %d, skip %d, start %lld) must lie inside the %lld variables with "
                  "nw + skip <= 512, and gamma > 0", who, (long long)nwcon, k.nw, k.skip, (long long)k.start,
                  (long long)n);
    return PO_ERR_ARG;
  }
  if (nwcon > 0) {
    if (!k.c) return ArgCheck::null("c");
    if (!k.zw) return ArgCheck::null("zw");
    if (k.c->ctx != k.ctx || k.zw->ctx != k.ctx || k.c->n != nwcon || k.zw->n != nwcon) {
      po::set_error("%s: c and zw hold nwcon = %lld values", who, (long long)nwcon);
      return PO_ERR_ARG;
    }
    g.c = k.c->d;
  }
  double *const zw = nwcon > 0 ? k.zw->d : nullptr;
  const MmaDualData s = mma_dual_data(v.L->d, v.U->d, v.alpha->d, v.beta->d, v.p0->d, v.q0->d, pp.data(), qq.data(),
                                      k.b, m, n);
  const MmaDualRho r{k.rho ? k.xk->d : nullptr, k.rho};
  MmaGroupStats st;
  auto put_stats = [&]() {
    const double out[8] = {(double)st.strict,    (double)st.at_lower, (double)st.at_gamma, (double)st.cap_hits,
                           (double)st.steps,     (double)st.max_inner, st.max_psi,         st.zw_psi};
    for (int i = 0; i < 8 && k.stats; i++) k.stats[i] = out[i];
  };
  if (point) {
    PO_TRY(k_mma_group_solve(k.ctx, s, g, k.lambda, k.x->d, zw, k.zl->d, k.zu->d, &st, &r));
    PO_TRY(k_mma_gcmma_group_sums(k.ctx, s, r.xk, k.x->d, k.sums));
    put_stats();
    return PO_OK;
  }
  WorkVecs work(k.ctx);  // G (m of n), d (n), and with groups Uw (m of nwcon), sw (nwcon)
  int rc = work.add(m + 1, n);
  if (rc == PO_OK && nwcon > 0) rc = work.add(m + 1, nwcon);
  if (rc == PO_OK) {
    const std::vector<double *> G = work.pointers(0, m), Uw = work.pointers(m + 1, nwcon > 0 ? m : 0);
    rc = k_mma_dual_groups(k.ctx, s, g, k.lambda, k.W, k.grad, k.hess, G.data(), work.d(m), k.x->d, zw,
                           nwcon > 0 ? Uw.data() : nullptr, nwcon > 0 ? work.d(2 * m + 1) : nullptr, k.zl->d, k.zu->d,
                           &st, k.rho ? &r : nullptr, k.D);
  }
  rc = work.release(rc);
  if (rc == PO_OK) put_stats();
  return rc;
}
int po_mma_dual_group_eval(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                           const po_vec *p, const po_vec *q, const double *b, const double *lambda, int64_t nwcon,
                           int nw, int64_t start, int skip, double a, po_vec c, int64_t nwinequality, double gamma,
                           double *W, double *grad, double *hess, po_vec x, po_vec zl, po_vec zu, po_vec zw,
                           double *stats) {
  return mma_group_entry({.who = "po_mma_dual_group_eval", .ctx = ctx, .m = m, .v = {L, U, alpha, beta, p0, q0, p, q},
                          .b = b, .lambda = lambda, .nwcon = nwcon, .nw = nw, .start = start, .skip = skip, .a = a,
                          .c = c, .nwinequality = nwinequality, .gamma = gamma, .W = W, .grad = grad, .hess = hess,
                          .x = x, .zl = zl, .zu = zu, .zw = zw, .stats = stats});
}
int po_mma_dual_group_eval_rho(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                               const po_vec *p, const po_vec *q, const double *b, const double *lambda, int64_t nwcon,
                               int nw, int64_t start, int skip, double a, po_vec c, int64_t nwinequality, double gamma,
                               double *W, double *grad, double *hess, po_vec x, po_vec zl, po_vec zu, po_vec zw,
                               double *stats, po_vec xk, const double *rho, double *D) {
  PO_CHECK_PTR(xk);
  PO_CHECK_PTR(rho);
  return mma_group_entry({.who = "po_mma_dual_group_eval_rho", .ctx = ctx, .m = m,
                          .v = {L, U, alpha, beta, p0, q0, p, q}, .b = b, .lambda = lambda, .nwcon = nwcon, .nw = nw,
                          .start = start, .skip = skip, .a = a, .c = c, .nwinequality = nwinequality, .gamma = gamma,
                          .W = W, .grad = grad, .hess = hess, .x = x, .zl = zl, .zu = zu, .zw = zw, .stats = stats,
                          .xk = xk, .rho = rho, .D = D});
}
int po_mma_gcmma_group_point(po_ctx ctx, int m, po_vec L, po_vec U, po_vec alpha, po_vec beta, po_vec p0, po_vec q0,
                             const po_vec *p, const po_vec *q, const double *lambda, int64_t nwcon, int nw,
                             int64_t start, int skip, double a, po_vec c, int64_t nwinequality, double gamma,
                             po_vec xk, const double *rho, po_vec x, po_vec zl, po_vec zu, po_vec zw, double *sums,
                             double *stats) {
  PO_CHECK_PTR(xk);
  PO_CHECK_PTR(rho);
  PO_CHECK_PTR(sums);
  const double none = 0.0;  // (the point does not read b)
  return mma_group_entry({.who = "po_mma_gcmma_group_point", .ctx = ctx, .m = m,
                          .v = {L, U, alpha, beta, p0, q0, p, q}, .b = &none, .lambda = lambda, .nwcon = nwcon,
                          .nw = nw, .start = start, .skip = skip, .a = a, .c = c, .nwinequality = nwinequality,
                          .gamma = gamma, .x = x, .zl = zl, .zu = zu, .zw = zw, .stats = stats, .xk = xk, .rho = rho,
                          .sums = sums});
}
int po_mma_get_dual_group_stats(po_mma mma, long *strict, long *at_lower, long *at_gamma, int *max_inner,
                                long *cap_hits, double *max_psi) {
  PO_CHECK_PTR(mma);
  const MmaGroupStats &s = mma->mma->groups;
  if (strict) *strict = s.strict;
  if (at_lower) *at_lower = s.at_lower;
  if (at_gamma) *at_gamma = s.at_gamma;
  if (max_inner) *max_inner = s.max_inner;
  if (cap_hits) *cap_hits = s.cap_hits;
  if (max_psi) *max_psi = s.max_psi;
  return PO_OK;
}
int po_mma_get_globalization_stats(po_mma mma, int *inner_total, int *inner_last, int *inner_max, int *cap_hits,
                                   const double **rho) {
  PO_CHECK_PTR(mma);
  const MmaGcmmaStats &s = mma->mma->gcmma;
  if (inner_total) *inner_total = s.inner_total;
  if (inner_last) *inner_last = s.inner_last;
  if (inner_max) *inner_max = s.inner_max;
  if (cap_hits) *cap_hits = s.cap_hits;
  if (rho) *rho = s.rho.data();
  return PO_OK;
}

}  // extern "C"
