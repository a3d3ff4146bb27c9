// The quasi-definite solver of the sparse constraints (ParOptQuasiDefMat, src/ParOptSparseMat.h:11-65), which a
// problem creates (createQuasiDefMat, src/ParOptProblem.h:72) and the interior point factors and applies:
//     K0 = [ D  Aw^T ; Aw  -C ],  S = C + Aw D^-1 Aw^T.
// One class per form (quasidef.cpp); a problem owns exactly one object, chosen in Problem::chooseSolver.  The Jacobian
// products stay the problem's (problem.hpp): a solver calls back into the problem that owns it.
#pragma once
#include "core.hpp"
#include "qn.hpp"
#include "wcon.hpp"

namespace po {

class Problem;

// A real po_vec handle that borrows raw device storage for the length of a user callback: host-side callbacks may ask
// it for a pinned mirror (po_vec_get_array), which is released here -- the handle never reaches vec_decref
struct BorrowedVec : po_vec_s {
  BorrowedVec(Ctx *c, int64_t n_, const double *d_) {
    ctx = c;
    n = n_;
    d = const_cast<double *>(d_);
    ref = 1;
    h = nullptr;
  }
  ~BorrowedVec() {
    if (h) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipHostFree(h);
      mirror_freed();
    }
  }
};

// What gramSolve leaves behind; fixed for the life of a solver object, so the interior point reads it before it sizes
// its panels.
struct GramForm {
  // true: the solver exposes no factor, so gramSolve fills a second panel Yw_j = -S^-1 U_j, the Gram correction is the
  // symmetrised cross product W += (U^T Yw + Yw^T U) / 2 and correction() combines Yw.  false: gramSolve works on U in
  // place, the correction is W -= U^T diag(weights) U and correction() combines U
  bool solved;
  // U still holds the plain image Aw (d o P) afterwards
  bool plain;
};

class QuasiDefSolver {
 public:
  explicit QuasiDefSolver(Problem *p) : prob(p) {}
  virtual ~QuasiDefSolver() {}
  // ParOptQuasiDefMat::factor (src/ParOptSparseMat.h:25): cw holds Cdiag on entry.  Scalar forms: cw <- 1/(Cdiag +
  // diag(Aw d Aw^T)).  Every other form keeps its factor to itself and leaves cw alone.
  virtual int factor(Vec *x, Vec *d, Vec *cw) = 0;
  // The same with Cdiag = sw/zsw + tw/ztw (:1912-1927) formed from the sparse slack blocks on the way
  virtual int factorFromSlacks(Vec *x, Vec *d, const WVars &v, Vec *cw);
  // (yx, yw) = K0^-1 (bx, bw) of ParOptQuasiDefBlockMat::apply (src/ParOptSparseMat.cpp:122-190): yx = d o bx;
  // yw = S^-1 (bw - Aw yx); yx = d o (bx + Aw^T yw).  bx must not alias yx; bw may be null (zero block); `wwork` is
  // w-sized scratch.
  virtual int applyK0(Vec *x, Vec *d, Vec *cw, const double *bx, const double *bw, Vec *yx, Vec *yw, Vec *wwork) = 0;
  // U_j = Aw (d o P_j), j < nv, in the row order gramSolve and correction want (the problem's order, except for the
  // CSR form, which permutes); `work` is n-sized scratch
  virtual int panel(Vec *x, Vec *d, const double *const *P, int nv, double *const *U, Vec *work);
  virtual GramForm gramForm() const = 0;
  // Second half of the Gram correction W -= U^T S^-1 U for the panel U = panel(P) (see GramForm).  In place: U <- Y
  // with U^T S^-1 U = Y^T diag(*weights) Y.  Solved: Yw_j = -S^-1 Aw (d o P_j) (`work` n-sized scratch that no P_j
  // aliases), *weights = nullptr.
  virtual int gramSolve(const double *const *P, int nv, double *const *U, double *const *Yw, Vec *cw, Vec *work,
                        const double **weights) = 0;
  // out = -S^-1 (U alpha) from the panel gramForm() names, as gramSolve left it: K0^-1 (P alpha, 0) = (d (P alpha +
  // Aw^T out), out), which turns the second quasi-definite apply of a bordered solve into a correction of the first.
  // acc != nullptr: acc += out as well, in the same launch where the form allows it
  virtual int correction(const double *const *U, int nv, const double *alpha, Vec *cw, Vec *out, Vec *acc) = 0;
  // one line for the output file, null when there is nothing to say (getFactorInfo, :61)
  virtual const char *info() = 0;
  // factorizations so far that met a non-positive pivot, or that the user's factor reported as failed
  virtual long breakdowns() const { return 0; }
  // po_quasidef_factor after a factor that raised breakdowns(): the library's forms have set the error text themselves
  virtual void describeBreakdown() const {}
  // the user's table (po_problem_set_quasidef_callbacks), null for the library's forms
  virtual const po_quasidef_callbacks *userTable() const { return nullptr; }

 protected:
  Problem *prob;  // the owner: Jacobian products, sizes, group map
  // out = alpha . U, then acc += out: the first and last step of the unfused corrections
  int combine(const double *const *U, int nv, const double *alpha, Vec *out);
  int accumulate(Vec *out, Vec *acc);
};

}  // namespace po
