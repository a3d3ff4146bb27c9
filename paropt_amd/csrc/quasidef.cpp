// The five forms of the quasi-definite solver (quasidef.hpp) and the one place that chooses among them.
#include <stdio.h>

#include <string>

#include "problem.hpp"

namespace po {

int QuasiDefSolver::factorFromSlacks(Vec *x, Vec *d, const WVars &v, Vec *cw) {
  PO_TRY(k_w_cdiag(prob->ctx, v, prob->nwcon, cw->d));
  return factor(x, d, cw);
}
int QuasiDefSolver::panel(Vec *x, Vec *d, const double *const *P, int nv, double *const *U, Vec *work) {
  return prob->sparsePanelImage(x, d, P, nv, U, work);
}
int QuasiDefSolver::combine(const double *const *U, int nv, const double *alpha, Vec *out) {
  return k_panel_axpy(prob->ctx, out->d, 0.0, nullptr, 0.0, alpha, U, nv, prob->nwcon);
}
int QuasiDefSolver::accumulate(Vec *out, Vec *acc) {
  return acc ? k_axpy(prob->ctx, acc->d, 1.0, out->d, prob->nwcon) : PO_OK;
}

namespace {

// yx = d o bx; yw = S^-1 (bw - Aw yx) with `solve` for S^-1 in place; yx = d o (bx + Aw^T yw): the sequence of
// ParOptQuasiDefBlockMat::apply through the Jacobian callbacks (11 n-sized passes)
template <class Solve>
int apply_through_jacobian(Problem *p, Vec *x, Vec *d, const double *bx, const double *bw, Vec *yx, Vec *yw,
                           Solve solve) {
  Ctx *ctx = p->ctx;
  const int64_t n = p->nlocal, w = p->nwcon;
  PO_TRY(k_mul(ctx, yx->d, 1.0, d->d, bx, n));
  if (bw) {
    PO_TRY(k_copy(ctx, yw->d, bw, w));
  } else {
    PO_TRY(k_fill(ctx, yw->d, w, 0.0));
  }
  if (p->addSparseJacobian(-1.0, x, yx, yw) != 0) return PO_ERR_USER;
  PO_TRY(solve());
  PO_TRY(k_copy(ctx, yx->d, bx, n));
  if (p->addSparseJacobianTranspose(1.0, x, yw, yx) != 0) return PO_ERR_USER;
  return k_mul(ctx, yx->d, 1.0, d->d, yx->d, n);
}

// nwblock = 1 through the Jacobian callbacks: S is diagonal and cw = S^-1 is the whole factor
class ScalarSolver : public QuasiDefSolver {
 public:
  using QuasiDefSolver::QuasiDefSolver;
  int factor(Vec *x, Vec *d, Vec *cw) override {
    if (prob->addSparseInnerProduct(1.0, x, d, cw) != 0) return PO_ERR_USER;
    return k_recip(prob->ctx, cw->d, prob->nwcon);
  }
  int applyK0(Vec *x, Vec *d, Vec *cw, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *) override {
    return apply_through_jacobian(prob, x, d, bx, bw, yx, yw,
                                  [&] { return k_mul(prob->ctx, yw->d, 1.0, cw->d, yw->d, prob->nwcon); });
  }
  GramForm gramForm() const override { return {false, true}; }
  int gramSolve(const double *const *, int, double *const *, double *const *, Vec *cw, Vec *,
                const double **weights) override {
    *weights = cw->d;  // Y = U
    return PO_OK;
  }
  int correction(const double *const *U, int nv, const double *alpha, Vec *cw, Vec *out, Vec *acc) override {
    // sum, scale by -cw and the caller's accumulation in ONE w-sized launch (round 4; the same operations in the same
    // order as the three launches below) for as wide a panel as the kernel takes
    if (nv <= kMaxPanel) return k_w_correction(prob->ctx, U, nv, alpha, cw->d, prob->nwcon, out->d, acc ? acc->d : nullptr);
    PO_TRY(combine(U, nv, alpha, out));
    PO_TRY(k_mul(prob->ctx, out->d, -1.0, cw->d, out->d, prob->nwcon));
    return accumulate(out, acc);
  }
  const char *info() override { return "nblock: 1"; }  // ParOptQuasiDefBlockMat::getFactorInfo (:218-221)
};

// The grouped pattern (Problem::grouped): the same scalar form with the group kernels of wcon.hip in place of the
// Jacobian callbacks.  Reads the problem's gmap and group_alpha at every call (the entries of a recognised CSR pattern
// are known after each gradient evaluation).
class GroupedSolver : public ScalarSolver {
 public:
  using ScalarSolver::ScalarSolver;
  int factor(Vec *, Vec *d, Vec *cw) override {
    // Cw = 1 / (Cdiag + alpha^2 (sum of d over the group)): the group sum and the reciprocal in one launch
    const double a = prob->group_alpha;
    return k_group_sum(prob->ctx, prob->gmap, cw->d, 1, 0.0, a * a, d->d, 1);
  }
  int factorFromSlacks(Vec *x, Vec *d, const WVars &v, Vec *cw) override {
    // entries +-1: Cdiag from the slack blocks, the group sums of d and the reciprocal in ONE launch
    if (prob->group_alpha * prob->group_alpha == 1.0) return k_group_factor(prob->ctx, prob->gmap, v, d->d, cw->d);
    return QuasiDefSolver::factorFromSlacks(x, d, v, cw);
  }
  int applyK0(Vec *, Vec *d, Vec *cw, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *wwork) override {
    // u = Aw (d o bx) in one tiled pass, yw = cw (bw - u), yx = d (bx + alpha yw[group]); one launch where the map tiles
    Ctx *ctx = prob->ctx;
    const GroupMap &gmap = prob->gmap;
    const double a = prob->group_alpha;
    bool done = false;
    PO_TRY(k_group_k0(ctx, gmap, d->d, bx, cw->d, bw, a, prob->nlocal, yx->d, yw->d, &done));
    if (done) return PO_OK;
    const double *P[1] = {bx};
    double *U[1] = {wwork->d};
    PO_TRY(k_group_panel(ctx, gmap, P, 1, d->d, a, U));
    PO_TRY(k_w_apply_mid(ctx, cw->d, bw, wwork->d, prob->nwcon, yw->d));
    return k_group_apply(ctx, gmap, d->d, bx, a, yw->d, prob->nlocal, yx->d);
  }
};

// nwblock > 1 (ParOptQuasiDefBlockMat, src/ParOptSparseMat.cpp:11-229): S is block diagonal, factored block by block
class PackedBlockSolver : public QuasiDefSolver {
 public:
  // null when the buffers cannot be had
  static PackedBlockSolver *create(Problem *p, int nwblock) {
    PackedBlockSolver *s = new PackedBlockSolver(p, nwblock);
    Ctx *ctx = p->ctx;
    s->blk = vec_new(ctx, p->nwcon * (nwblock + 1) / 2);
    s->wones = vec_new(ctx, p->nwcon);
    int rc = (s->blk && s->wones) ? k_fill(ctx, s->wones->d, p->nwcon, 1.0) : PO_ERR_HIP;
    if (rc == PO_OK && hipMalloc((void **)&s->flag, 4 * sizeof(int)) != hipSuccess) rc = PO_ERR_HIP;
    if (rc == PO_OK) return s;
    delete s;
    return nullptr;
  }
  ~PackedBlockSolver() {
    vec_decref(blk);
    vec_decref(wones);
    if (flag) (void)hipFree(flag);
  }
  int factor(Vec *x, Vec *d, Vec *cw) override {  // :60-112
    Ctx *ctx = prob->ctx;
    PO_TRY(k_blk_init(ctx, cw->d, nb, nwblock, blk->d));
    if (prob->addSparseInnerProduct(1.0, x, d, blk) != 0) return PO_ERR_USER;
    const int flag0[4] = {0, 0x7fffffff, 0, 0};
    PO_HIP(hipMemcpyAsync(flag, flag0, sizeof(flag0), hipMemcpyHostToDevice, ctx->stream));
    PO_TRY(k_blk_factor(ctx, blk->d, nb, nwblock, flag));
    int got[4] = {0, 0, 0, 0};
    PO_HIP(hipMemcpyAsync(got, flag, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    PO_HIP(hipStreamSynchronize(ctx->stream));
    if (got[0] != 0) {  // the reference returns dpptrf's info, which its caller ignores (:1930)
      if (count == 0 && ctx->rank == 0) {  // warn once, like the CSR form
        fprintf(stderr,
                "ParOpt warning: the sparse constraint matrix is not positive definite (first failing row %d, block "
                "%d; %d pivots replaced)\n", got[1], got[1] / nwblock, got[0]);
      }
      count++;
    }
    return PO_OK;
  }
  int applyK0(Vec *x, Vec *d, Vec *, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *) override {
    return apply_through_jacobian(prob, x, d, bx, bw, yx, yw, [&] {  // applyFactor (:192-216)
      double *Y[1] = {yw->d};
      return k_blk_solve(prob->ctx, blk->d, nb, nwblock, Y, 1, 0);
    });
  }
  GramForm gramForm() const override { return {false, false}; }
  int gramSolve(const double *const *, int nv, double *const *U, double *const *, Vec *, Vec *,
                const double **weights) override {
    *weights = wones->d;  // S = U^T U per block: U_panel^T S^-1 U_panel = (U^-T P)^T (U^-T P)
    return k_blk_solve(prob->ctx, blk->d, nb, nwblock, U, nv, 1);
  }
  int correction(const double *const *U, int nv, const double *alpha, Vec *, Vec *out, Vec *acc) override {
    PO_TRY(combine(U, nv, alpha, out));
    double *Y[1] = {out->d};  // -U^-1 (Y alpha)
    PO_TRY(k_blk_solve(prob->ctx, blk->d, nb, nwblock, Y, 1, 2));
    PO_TRY(k_scale(prob->ctx, out->d, prob->nwcon, -1.0));
    return accumulate(out, acc);
  }
  const char *info() override { return text.c_str(); }
  long breakdowns() const override { return count; }

 private:
  PackedBlockSolver(Problem *p, int nwblock_)
      : QuasiDefSolver(p), nwblock(nwblock_), nb(p->nwcon / nwblock_), text("nblock: " + std::to_string(nwblock_)) {}
  int nwblock;
  int64_t nb;
  Vec *blk = nullptr;    // packed blocks: C + Aw D^-1 Aw^T, then its Cholesky factor U (A = U^T U)
  Vec *wones = nullptr;  // unit weights for the Gram of the half-solved panel
  int *flag = nullptr;
  long count = 0;  // factorizations that replaced a non-positive pivot
  std::string text;
};

// General CSR pattern: S is factored on the device by the problem's CsrSparse (borrowed: the pattern, the values and
// the products stay the problem's)
class CsrSolver : public QuasiDefSolver {
 public:
  using QuasiDefSolver::QuasiDefSolver;
  int factor(Vec *, Vec *d, Vec *cw) override { return prob->csr->factor(d->d, cw->d); }
  int applyK0(Vec *, Vec *d, Vec *, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *) override {
    return prob->csr->applyK0(d->d, bx, bw, yx->d, yw->d);
  }
  int panel(Vec *, Vec *d, const double *const *P, int nv, double *const *U, Vec *) override {
    return prob->csr->panelPermuted(d->d, P, nv, U);
  }
  GramForm gramForm() const override { return {false, false}; }
  int gramSolve(const double *const *, int nv, double *const *U, double *const *, Vec *, Vec *,
                const double **weights) override {
    *weights = prob->csr->unitWeights();  // Y = L^-1 U in place, S = L L^T
    return prob->csr->halfSolve(U, nv);
  }
  int correction(const double *const *U, int nv, const double *alpha, Vec *, Vec *out, Vec *acc) override {
    PO_TRY(prob->csr->correction(U, nv, alpha, out->d));  // -L^-T (Y alpha)
    return accumulate(out, acc);
  }
  const char *info() override { return prob->csr->factorInfo(); }
  long breakdowns() const override { return prob->csr->breakdowns; }
};

// General CSR pattern with dense columns taken out of S (csr.hpp): S^-1 is the factor of S0 plus a low-rank
// correction, so no half-solved panel Y with U^T S^-1 U = Y^T Y exists.  The Gram correction takes the SOLVED panel, as
// for a user's solver, filled for all columns in one sweep; factor, applyK0 and the factor line are the CSR form's.
// (Also chosen on a rank without a dense column when another rank has one: the form decides which collective the
// interior point issues, so it is the same on every rank.)
class CsrDenseColumnSolver : public CsrSolver {
 public:
  using CsrSolver::CsrSolver;
  int panel(Vec *, Vec *d, const double *const *P, int nv, double *const *U, Vec *) override {
    return prob->csr->panelNatural(d->d, P, nv, U);
  }
  GramForm gramForm() const override { return {true, true}; }
  int gramSolve(const double *const *, int nv, double *const *U, double *const *Yw, Vec *, Vec *,
                const double **weights) override {
    *weights = nullptr;
    return prob->csr->solvePanel(U, nv, Yw);  // Yw = -S^-1 U
  }
  int correction(const double *const *Yw, int nv, const double *alpha, Vec *, Vec *out, Vec *acc) override {
    PO_TRY(combine(Yw, nv, alpha, out));  // Yw alpha = -S^-1 (U alpha): no further solve
    return accumulate(out, acc);
  }
};

// createQuasiDefMat (src/ParOptProblem.h:72): the problem brings its own quasi-definite solver.  factor forms nothing
// and calls the user's factor(x, d, Cdiag) with cw = Cdiag left alone, applyK0 is the user's apply and nothing else.
// The user exposes no factor, so the Gram correction takes the SOLVED panel: one three-argument apply per column.
class UserSolver : public QuasiDefSolver {
 public:
  UserSolver(Problem *p, const po_quasidef_callbacks &cb) : QuasiDefSolver(p), qd(cb) {}
  int factor(Vec *x, Vec *d, Vec *cw) override {
    const int fail = qd.factor(qd.user, static_cast<po_vec>(x), static_cast<po_vec>(d), static_cast<po_vec>(cw));
    if (fail != 0) {  // the reference ignores the value (src/ParOptInteriorPoint.cpp:1930, 5429): warn once, count
      if (count == 0) set_error("the problem's quasi-definite solver reported a failed factorization (%d)", fail);
      count++;
      last_fail = fail;
    }
    return PO_OK;
  }
  int applyK0(Vec *, Vec *, Vec *, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *) override {
    BorrowedVec vbx(prob->ctx, prob->nlocal, bx), vbw(prob->ctx, prob->nwcon, bw);
    return apply(&vbx, bw ? static_cast<po_vec>(&vbw) : nullptr, static_cast<po_vec>(yx), static_cast<po_vec>(yw));
  }
  GramForm gramForm() const override { return {true, true}; }
  int gramSolve(const double *const *P, int nv, double *const *, double *const *Yw, Vec *, Vec *work,
                const double **weights) override {
    *weights = nullptr;
    for (int j = 0; j < nv; j++) {
      BorrowedVec bx(prob->ctx, prob->nlocal, P[j]), yw(prob->ctx, prob->nwcon, Yw[j]);
      PO_TRY(apply(&bx, nullptr, static_cast<po_vec>(work), &yw));
    }
    return PO_OK;
  }
  int correction(const double *const *Yw, int nv, const double *alpha, Vec *, Vec *out, Vec *acc) override {
    PO_TRY(combine(Yw, nv, alpha, out));  // Yw alpha = -S^-1 (U alpha): no further user call
    return accumulate(out, acc);
  }
  const char *info() override { return qd.factor_info ? qd.factor_info(qd.user) : nullptr; }
  long breakdowns() const override { return count; }
  void describeBreakdown() const override {  // (announced once only by factor)
    set_error("the problem's quasi-definite solver reported a failed factorization (%d)", last_fail);
  }
  const po_quasidef_callbacks *userTable() const override { return &qd; }

 private:
  int apply(po_vec bx, po_vec bw, po_vec yx, po_vec yw) {
    const int fail = qd.apply(qd.user, bx, bw, yx, yw);
    if (fail == 0) return PO_OK;
    set_error("the problem's quasi-definite solver failed in apply (%d)", fail);
    return PO_ERR_USER;
  }
  po_quasidef_callbacks qd;
  long count = 0;     // factor calls that returned non-zero
  int last_fail = 0;  // the last such value
};

}  // namespace

// The precedence of the forms, written once: user > grouped > CSR with dense columns > CSR > packed block > generic
// scalar.  Called wherever
// one of its inputs changes; `user` is the table to carry (userSolverTable() keeps what is attached, null detaches).
// A failure leaves the previous solver and block size in place.
int Problem::chooseSolver(const po_quasidef_callbacks *user, int nwblock_) {
  QuasiDefSolver *s = nullptr;
  if (user) {
    s = new UserSolver(this, *user);
  } else if (grouped) {
    s = new GroupedSolver(this);
  } else if (csr && csr_dense_form) {
    s = new CsrDenseColumnSolver(this);
  } else if (csr) {
    s = new CsrSolver(this);
  } else if (nwblock_ > 1) {
    s = PackedBlockSolver::create(this, nwblock_);
    if (!s) return PO_ERR_HIP;
  } else {
    s = new ScalarSolver(this);
  }
  delete solver;
  solver = s;
  nwblock = nwblock_;
  return PO_OK;
}

}  // namespace po
