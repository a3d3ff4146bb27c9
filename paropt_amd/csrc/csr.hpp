// The general sparse-constraint path: a fixed CSR pattern for the Jacobian Aw of the rank-local sparse
// constraints (ParOptSparseProblem, reference src/ParOptProblem.h:301-395, src/ParOptProblem.cpp:624-816)
// and the quasi-definite solve
//     [ D   Aw^T ] [ yx ]   [ bx ]
//     [ Aw  -C   ] [-yw ] = [ bw ]          S = C + Aw D^-1 Aw^T   sparse, SPD
// of ParOptQuasiDefSparseMat (src/ParOptSparseMat.cpp:234-450).
//
// Split of the work (MI355X first, not the reference's host supernodal code):
//   host, ONCE per pattern : sorted CSR/CSC, pattern of S, nested-dissection ordering from BFS level
//                            structures, elimination tree, pattern of L, dependency level sets
//   device, every iteration: S assembled straight into L's value array (one thread per structural
//                            entry), a level-scheduled row Cholesky (one wavefront per row), level-scheduled
//                            triangular solves for a whole panel of right-hand sides, CSR/CSC products
// Everything is rank-local (the reference's sparse constraints never couple ranks), deterministic
// (no atomics), and there is no host numeric path.
// Columns of Aw that enter (nearly) every row would make S dense: the analysis takes them out and the
// device puts them back by a low-rank correction of every solve (CsrSymbolic: DENSE COLUMNS).
//
// PARITY UNPINNED for the factorization itself: the reference's ParOptSparseCholesky.cpp needs METIS,
// which this image lacks, so no reference-run golden exists for it.  What IS pinned: trajectories of
// the reference's interior point on ParOptSparseProblem (its own CSR products) with a dense LAPACK
// S-solve supplied by oracle/ref_driver.cpp through createQuasiDefMat() (tests/golden/ipcsr_*.npz); a
// direct solve is unique up to round-off, and tests also compare against a dense numpy Cholesky.
#pragma once
#include <string>
#include <vector>

#include "core.hpp"
#include "qn.hpp"
#include "sparse_chol.hpp"

namespace po {

// host result of the one-time analysis (all indices int32; sizes checked)
struct CsrSymbolic {
  int w = 0, n = 0;
  int64_t nnz = 0;
  std::vector<int> rowp, cols, src;     // A sorted by column within each row; src = user slot of each entry
  std::vector<int> colp, rowsT, srcT;   // A^T: srcT indexes the SORTED value array
  std::vector<int> perm, iperm;         // perm[new] = old
  std::vector<int> parent;              // elimination tree of P S P^T
  std::vector<int> Lrowp, Lcols;        // rows of L (lower, columns ascending, diagonal last)
  std::vector<int> Ltp, Ltrows, Ltsrc;  // columns of L below the diagonal, Ltsrc = slot in the row storage
  std::vector<int> ent_a, ent_b, ent_slot;  // structural entries of lower(P S P^T): rows a,b of A -> slot in L
  // rows grouped by dependency level: ascending for the factorization and the forward solve, descending for
  // the backward solve.  Rows are NUMBERED level by level, so fwd_order is the identity and each level is a
  // contiguous range of rows (and of L's storage).
  std::vector<int> fwd_order, fwd_ptr;
  std::vector<int> fwd_maxlen, bwd_maxlen;  // longest ordinary row / column of each level (kernel variant choice)
  // Each level = ordinary rows [fwd_ptr[l], ord_end[l]) followed by the rows of its FRONTS (dense separator
  // cliques, front_ptr[l] .. front_ptr[l+1]-1 in front_start / front_size): row front_start + r ends with the
  // columns front_start .. front_start + r, so the front's lower triangle is the tails of its rows.
  std::vector<int> ord_end, front_ptr, front_start, front_size, front_of;
  std::vector<int> front_maxdesc;  // per level: longest part of a front row left of its front
  int max_front = 0;
  int64_t nnzS = 0, nnzL = 0;
  bool identity_src = true;
  // DENSE COLUMNS (at most kMaxDenseCols): columns of Aw taken out of S and put back by a low-rank correction,
  //     S = S0 + V E V^T,  S0 = C + As D^-1 As^T,  V = Aw[:, J],  E = diag(Dinv[J]).
  // Everything above except rowp/cols/src then describes S0 and As: the transposed index colp/rowsT/srcT leaves the
  // columns of J empty, the row storage keeps them.  Column dense_cols[j] (ascending) holds the entries
  // dense_ptr[j] .. dense_ptr[j+1]-1: row dense_rows (ascending), position dense_pos = iperm[row] in the elimination
  // order, value slot dense_slot in the SORTED value array.  Empty when no column qualifies: every array above is
  // then what the analysis without the rule produces.
  std::vector<int> dense_cols, dense_ptr, dense_rows, dense_pos, dense_slot;
  // THE MULTIFRONTAL FACTOR (factor_kind == PO_SPARSE_FACTOR_MULTIFRONTAL): S0 is factored by the engine of
  // sparse_chol.hpp instead of the row factor.  `chol` is its analysis of S0 with PO_ORDER_ND, perm / iperm are
  // ITS elimination order (so dense_pos, the permuted panels and every gather follow it), nnzL its fill.  ent_a / ent_b
  // are the structural entries of lower(P S0 P^T) as above and ent_off[e] is where entry e lies in the engine's L: the
  // engine's own value scatter (asm_src -> asm_dst) composed with the entry list, so S0 is assembled straight into
  // the front panels.  Nothing of the row factor exists then: parent, L*, Lt*, ent_slot, the level and front tables
  // stay empty.
  int factor_kind = 0;
  CholSymbolic chol;
  std::vector<int64_t> ent_off;
};

constexpr int kMaxDenseCols = 64;

// returns PO_OK or PO_ERR_ARG (message set); pure host code, testable without a GPU.  min_rows is the dense-column
// rule: > 0, every column with at least that many entries is dense; 0 (automatic), nothing is taken out unless the
// pattern would be refused (more than 1.5e9 pairs), then the columns with at least max(1024, w/8) entries; -1, never.
// factor_kind: PO_SPARSE_FACTOR_ROWS or PO_SPARSE_FACTOR_MULTIFRONTAL (CsrSymbolic).
int csr_analyse(int64_t n, int64_t w, const int *rowp, const int *cols, CsrSymbolic *out, int64_t min_rows = 0,
                int factor_kind = 0);

// Steps of the analysis shared with the multifrontal factor (sparse_chol.cpp).  adjp / adj is the graph of the
// matrix without its diagonal, both triangles; perm[new] = old and iperm is its inverse.
void sym_nd_order(const std::vector<int> &adjp, const std::vector<int> &adj, int w, std::vector<int> *perm);
void sym_etree(const std::vector<int> &adjp, const std::vector<int> &adj, const std::vector<int> &perm,
               const std::vector<int> &iperm, std::vector<int> *parent);
void sym_colcount(const std::vector<int> &adjp, const std::vector<int> &adj, const std::vector<int> &perm,
                  const std::vector<int> &iperm, const std::vector<int> &parent, std::vector<int> *colcount);

// KERNEL FORMS.  Every elimination level of the factorization and of the two triangular sweeps is launched in one of
// several forms; csr_level_plan() is the one place that chooses among them, from the analysis alone.  CsrSparse::factor
// and solveInPlace launch what it returns, and po_csr_symbolic_kernel_forms reports it without a device.
enum CsrForm {
  CF_LEVEL_THIN = 0,      // chol_level_thin_kernel: one thread per ordinary row
  CF_LEVEL_TABLE,         // chol_level_kernel<1>: one wavefront per row, lookups in the LDS hash table
  CF_LEVEL_SEARCH,        // chol_level_kernel<0>: the row is too long for the table, binary search
  CF_FRONT_ROWS_TABLE,    // chol_front_rows_kernel<1>
  CF_FRONT_ROWS_WIDE,     // chol_front_rows_wide_kernel<8>: eight wavefronts share a long front row
  CF_FRONT_ROWS_SEARCH,   // chol_front_rows_kernel<0>
  CF_FRONT_SYRK_TABLE,    // chol_front_syrk_kernel<1>
  CF_FRONT_SYRK_SEARCH,   // chol_front_syrk_kernel<0>
  CF_FRONT_DENSE_LDS,     // chol_front_dense_kernel on a front whose column fits LDS
  CF_FRONT_DENSE_GLOBAL,  // ... on a larger front, through global memory
  CF_TRSV_FWD_THIN,       // trsv_fwd_thin_kernel: one thread per (row, right-hand side)
  CF_TRSV_FWD_WAVE,       // trsv_fwd_kernel: one wavefront per (row, right-hand side), one workgroup per row
  CF_TRSV_FWD_WAVE_SPLIT, // ... the right-hand sides of a row split over gridDim.y workgroups
  CF_TRSV_BWD_THIN,
  CF_TRSV_BWD_WAVE,
  CF_TRSV_BWD_WAVE_SPLIT,
  CF_COUNT
};
const char *csr_form_name(int form);  // "level:thin", ... (null past CF_COUNT)

// fronts up to this many rows keep their row offsets and the current column in LDS (chol_front_dense_kernel)
constexpr int kFrontLds = 2048;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool front_in_lds(int rows) { return rows <= kFrontLds; }

// right-hand sides of the next launch when nv_left remain: one kernel's pointer table holds kMaxPanel
inline int csr_slab(int nv_left) { return nv_left > kMaxPanel ? kMaxPanel : nv_left; }

// What one level launches for a panel of nv <= kMaxPanel right-hand sides (the factorization ignores nv).  A form of
// -1: nothing of that kind in the level.
struct CsrLevelPlan {
  int level = -1, level_tcap = 0;                         // ordinary rows; capacity of the LDS table (0: none)
  int front_rows = -1, front_syrk = -1, front_tcap = 0;   // the part of the front rows left of their fronts
  bool front_dense_lds = false, front_dense_global = false;  // the kernel chooses per front: which sizes occur
  int trsv_fwd = -1, trsv_bwd = -1;                       // ordinary rows of the two sweeps
  int fwd_gy = 1, bwd_gy = 1;                             // gridDim.y of the wave forms
  int trsv_waves = 1;                                     // wavefronts per workgroup of the wave and front-row solves
};
CsrLevelPlan csr_level_plan(const CsrSymbolic &s, int level, int nv);
// counts[f] = number of levels that launch form f for a panel of nv right-hand sides (nv > kMaxPanel: in any slab)
void csr_kernel_forms(const CsrSymbolic &s, int nv, int counts[CF_COUNT]);

class CsrSparse {
 public:
  CsrSparse(Ctx *c, int64_t n_, int64_t w_);
  ~CsrSparse();
  // A CsrSparse is BUILT ONCE: one of setPattern / setPatternLight on a fresh object, and at most one
  // upgradeFromLight() afterwards.  Every device array is a DevArray (core.hpp): freed with the object, counted by
  // po_live_objects.
  int setPattern(const int *rowp, const int *cols);
  int64_t dense_min_rows = 0;  // the dense-column rule of csr_analyse; set before setPattern
  int factor_kind = 0;         // PO_SPARSE_FACTOR_*: which engine factors S0; set before setPattern
  // The pattern was recognised as the grouped one (problem.hpp): only what the user's callbacks and
  // getSparseJacobianData need -- host copies of the pattern, the value array, the constraint vector -- and NO
  // symbolic analysis (at w = 1 M rows it would cost seconds and hundreds of MB that the block form never uses).
  // upgradeFromLight() runs the analysis after all (the entries turned out not to be uniform): `data`, what the user
  // wrote into it and the Vec `cw` stay the objects they were, also when the analysis fails.
  int setPatternLight(const int *rowp, const int *cols);
  int upgradeFromLight();
  bool light = false;
  // the user's value array in the user's entry order (device, nnz doubles) and the constraint values
  DevArray<double> data;
  Vec *cw = nullptr;
  // call after `data` changed (evalObjConGradient): refreshes the column-sorted copy
  int valuesChanged();
  int spmv(double alpha, const double *px, double *out);     // out += alpha Aw px        (w)
  int spmvT(double alpha, const double *pzw, double *out);   // out += alpha Aw^T pzw     (n)
  int innerProduct(double alpha, const double *cvec, double *out);  // out_i += alpha sum_k a_ik^2 c_k
  int colSum(double scale, const double *y, double *out);    // out_j = scale * sum of y over the rows touching j
  // U_j = Aw (d o P_j), rows in the factor's elimination order (only the Gram correction reads them)
  int panelPermuted(const double *d, const double *const *P, int nv, double *const *U);
  int panelNatural(const double *d, const double *const *P, int nv, double *const *U);  // the same, Aw's row order
  int factor(const double *dinv, const double *cdiag);       // S = diag(cdiag) + Aw diag(dinv) Aw^T = L L^T
  int halfSolve(double *const *U, int nv);                   // U_j <- L^-1 U_j (elimination order, in place)
  // out (natural order) = -S^-1 (U alpha) from the half-solved panel Y = L^-1 U: -L^-T (Y alpha)
  int correction(const double *const *Y, int nv, const double *alpha, double *out);
  // (yx, yw) = K0^-1 (bx, bw); bw may be null; bx must not alias yx
  int applyK0(const double *dinv, const double *bx, const double *bw, double *yx, double *yw);
  // Yw_j (natural order) = -S^-1 U_j for a whole panel U in natural order, one sweep: permute, forward solve, the
  // low-rank step, backward solve, un-permute and negate.  U is left alone.
  int solvePanel(const double *const *U, int nv, double *const *Yw);
  int ndense() const { return (int)sym.dense_cols.size(); }
  const double *unitWeights() const { return ones; }
  const char *factorInfo();
  // host copies for getSparseJacobianData (src/ParOptProblem.cpp:689-703)
  std::vector<int> user_rowp, user_cols;
  CsrSymbolic sym;
  Ctx *ctx;
  int64_t n, w, nnz;
  int nlevels_f = 0;
  long breakdowns = 0;  // factorizations that met a non-positive pivot (see factor())

 private:
  int allocUser(const int *rowp, const int *cols);  // what the user sees: data, the vals alias, cw
  int analyse(const int *rowp, const int *cols);    // the analysis and its device tables; touches none of the above
  int sortedValues();                               // after both: vals, where it is not `data` itself
  int solveInPlace(double *const *Y, int nv, bool forward, bool backward);
  // dense columns (csr.hpp: CsrSymbolic): Y_j -= Yv K^-1 (Yv^T Y_j) on half-solved columns in the elimination order
  int lowRankStep(double *const *Y, int nv);
  // out[J] = dscale[J] (bx[J] + alpha A^T y[J]) with A = V (pattern_only: its indicator) and y in the order `idx` names
  int denseColumnsOut(bool pattern_only, const double *y, const int *idx, double alpha, const double *bx,
                      const double *dscale, double *out);
  int densePartials(int nv);  // room for the block partials of an r x nv product
  // THE PATTERN AND ITS TRANSPOSE.  vals: the column-sorted values, `data` itself when the user's order is already
  // sorted, sorted_vals otherwise
  double *vals = nullptr;
  DevArray<double> sorted_vals;
  DevArray<int> d_rowp, d_cols, d_src;
  DevArray<int> d_colp, d_rowsT, d_srcT;
  DevArray<int> d_perm, d_iperm;
  DevArray<int> d_ent_a, d_ent_b;
  DevArray<double> ones, wwork;
  DevArray<int> d_flag;
  int spmv_group = 1, spmvT_group = 1;
  // THE ROW FACTOR (empty under the multifrontal kind)
  DevArray<double> Lvals;
  DevArray<int> d_Lrowp, d_Lcols;
  DevArray<int> d_Ltp, d_Ltrows, d_Ltsrc;
  DevArray<int> d_fwd;
  DevArray<int> d_front_of, d_front_end, d_fstart, d_fsize;
  DevArray<int> d_ent_slot;
  // THE MULTIFRONTAL SIDE: the engine (owned; null with the row factor; its CholSymbolic is the analysis, sym.chol is
  // moved into it) and where each structural entry of S0 lies in its L
  SparseChol *mf = nullptr;
  DevArray<int64_t> d_ent_off;
  // THE DENSE COLUMNS (and the panel of solvePanel); a fresh one is the state without any
  struct DenseCols {
    int nb = 1;        // workgroups of the first reduction stage: a function of w alone
    int64_t ld = 0;    // stride of the r w-vectors below
    int maxlen = 0, part_cap = 0, spanel_cap = 0;
    DevArray<double> Vd, Yv, Vind;  // V and L^-1 P V (elimination order); indicator of V, on demand
    DevArray<double> Kfac, Zd, part, spanel;
    DevArray<unsigned char> mask;
    DevArray<int> cols, ptr, pos, slot;
  } dense;
  std::string info;
};

// kernels (csr.hip)
int k_csr_gather(Ctx *c, double *dst, const double *src, const int *idx, int64_t n);
int k_csr_spmv(Ctx *c, int group, const int *rowp, const int *cols, const double *vals, int64_t w, double alpha,
               const double *x, const double *scale, double beta, const double *b, double *out, const int *outperm);
int k_csr_spmvT(Ctx *c, int group, const int *colp, const int *rowsT, const int *srcT, const double *vals,
                int64_t n, double alpha, const double *y, const double *bx, const double *dscale, double *out);
int k_csr_colsum(Ctx *c, const int *colp, const int *rowsT, int64_t n, double scale, const double *y, double *out);
int k_csr_inner(Ctx *c, const int *rowp, const int *cols, const double *vals, int64_t w, double alpha,
                const double *cvec, double *out);
int k_csr_panel(Ctx *c, const int *rowp, const int *cols, const double *vals, int64_t w, const double *d,
                const double *const *P, int nv, double *const *U, const int *outperm);
int k_csr_assemble(Ctx *c, const int *rowp, const int *cols, const double *vals, const double *dinv,
                   const double *cdiag, const int *ent_a, const int *ent_b, const int *ent_slot, int64_t nent,
                   double *Lvals, const unsigned char *skip = nullptr);
// the same with 64-bit destinations (the multifrontal engine's panels)
int k_csr_assemble(Ctx *c, const int *rowp, const int *cols, const double *vals, const double *dinv,
                   const double *cdiag, const int *ent_a, const int *ent_b, const int64_t *ent_off, int64_t nent,
                   double *L, const unsigned char *skip = nullptr);
// (the forms, table capacities and grid shapes below are what csr_level_plan chose: the launchers decide nothing)
int k_chol_level(Ctx *c, const int *Lrowp, const int *Lcols, double *Lvals, const int *rows, int nrows, int *flag,
                 const CsrLevelPlan &plan);
int k_chol_fronts(Ctx *c, const int *Lrowp, const int *Lcols, double *Lvals, int row0, int nrows,
                  const int *front_of, const int *fstart, const int *fsize, int nfronts, const CsrLevelPlan &plan,
                  int *flag);
int k_trsv_fronts_fwd(Ctx *c, const int *Lrowp, const int *Lcols, const double *Lvals, int row0, int nrows,
                      const int *front_of, const int *fstart, const int *fsize, int nfronts, double *const *Y,
                      int nv, const CsrLevelPlan &plan);
int k_trsv_fronts_bwd(Ctx *c, const int *Lrowp, const int *Ltp, const int *Ltrows, const int *Ltsrc,
                      const double *Lvals, int row0, int nrows, const int *front_of, const int *front_end,
                      const int *fstart, const int *fsize, int nfronts, double *const *Y, int nv,
                      const CsrLevelPlan &plan);
int k_trsv_fwd_level(Ctx *c, const int *Lrowp, const int *Lcols, const double *Lvals, const int *rows, int nrows,
                     double *const *Y, int nv, const CsrLevelPlan &plan);
int k_trsv_bwd_level(Ctx *c, const int *Lrowp, const int *Ltp, const int *Ltrows, const int *Ltsrc,
                     const double *Lvals, const int *rows, int nrows, double *const *Y, int nv,
                     const CsrLevelPlan &plan);
// dense columns (csr.hip): scatter of V, the two-stage panel product and its consumers, the low-rank update
int k_dense_scatter(Ctx *c, const int *ptr, const int *pos, const int *slot, const double *vals, int r, int maxlen,
                    int64_t ld, double *V);
int dense_dot_blocks(int64_t w);
int k_dense_dot(Ctx *c, const double *A, int64_t lda, int r, const double *const *B, int nv, const int *idx,
                int64_t w, double *part);
int k_dense_kfactor(Ctx *c, const double *part, int nb, int r, const double *dinv, const int *J, double *Kfac,
                    int *flag, int64_t w);
int k_dense_ksolve(Ctx *c, const double *part, int nb, int r, int nv, const double *Kfac, double *Z);
int k_dense_update(Ctx *c, const double *Yv, int64_t ld, int r, double *const *Y, int nv, const double *Z, int64_t w);
int k_dense_out(Ctx *c, const double *part, int nb, int r, const int *J, double alpha, const double *bx,
                const double *dscale, double *out);
int k_csr_panel_gather(Ctx *c, double *const *dst, const double *const *src, int nv, const int *idx, double sign,
                       int64_t w);
// built-in chain constraints cw_i = 1 - sum_{k<span} x[i*stride + k]^2 and their Jacobian entries
int k_chain_con(Ctx *c, const double *x, int64_t w, int span, int stride, double *cw);
int k_chain_jac(Ctx *c, const double *x, int64_t w, int span, int stride, int reverse, double *data);
// ... plus nd variables xd that enter every row: cw_i -= sum_j xd[j]^2, rows of span + nd entries
int k_chain_dense_con(Ctx *c, const double *x, int64_t w, int span, int stride, const double *xd, int nd, double *cw);
int k_chain_dense_jac(Ctx *c, const double *x, int64_t w, int span, int stride, int reverse, const double *xd, int nd,
                      double *data);

}  // namespace po
