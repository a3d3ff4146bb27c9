// ParOptSparseCholesky (reference src/ParOptSparseCholesky.h:29-162): a sparse Cholesky factorization
//     L L^T = P A P^T
// of a user's own SPD matrix, as a supernodal MULTIFRONTAL method with dense fronts on the device.  It stands beside
// CsrSparse (csr.hpp), whose row factor stays the interior point's default; a problem that asks for
// PO_SPARSE_FACTOR_MULTIFRONTAL has CsrSparse own one of these and factor S through it.
//
// Split of the work:
//   host, once per pattern (sparse_chol.cpp, no device needed): symmetrised pattern, ordering, elimination tree in
//     postorder, fundamental supernodes, the row structure of every supernode, level sets over the supernode tree,
//     relative indices child -> parent front, the scatter table A -> L, the layout of the work arena and the launch
//     tables of every level;
//   device, every factorization (sparse_chol.hip): level by level, every front of a level in the same launches --
//     assemble (zero + extend-add, the parent gathers its children in a fixed order, no atomics), partial Cholesky of
//     the first s columns (one wavefront for a small front; diagonal block / trsm / MFMA tile update per block column
//     for the others), and level-scheduled forward and backward solves for up to kCholMaxRhs right-hand sides a sweep.
//     With a cap on packed groups (below; off by default) a subtree of tiny fronts is run by one lane instead.
//
// Ordering.  PO_ORDER_ND is the nested dissection of csr.cpp (sym_nd_order).  PO_ORDER_NATURAL is the identity, or the
// caller's perm (perm[new] = old).  PO_ORDER_AMD is ACCEPTED AND GIVEN THE SAME NESTED DISSECTION: this project has no
// minimum-degree code, and the reference's is not taken over.
//
// Supernode J: s columns first .. first + s - 1 and b rows below them (below_rows, ascending); its front is dense of
// order m = s + b.  The (s + b) x s panel of L is stored column-major with an even leading dimension (16-byte aligned
// columns); the b x b update matrix lives in the arena until the parent has gathered it.  Only lower triangles are
// read or written anywhere.
//
// Schur complement (opt-in: chol_analyse with a Schur set of ns > 0 unknowns).  The set is ordered LAST, in the caller's
// order, as ONE final supernode with s = ns, b = 0 that is assembled and never eliminated: after factor() its panel
// holds the lower triangle of S = A22 - A21 A11^-1 A12 (both factorization kinds).  The ordering type is applied to
// the graph induced on the interior unknowns; for the analysis the set is a clique, so any A22 entry lies inside the
// pattern.  That supernode is in no factor list, no sweep list, no chunk list and no packed group; the interior
// subtrees that touch the set are its children, and their update matrices (factorization) and update vectors (forward
// sweep) reach it through two gather tables built by the analysis (schur_*), one launch each, a lane per destination,
// sources summed in child order: the sums of chol_assemble_kernel / chol_fwd_kernel without the walk over the
// children.  The solve splits into condense (forward sweep over the interior, g = b2 - A21 A11^-1 b1 in the Schur
// entries) and expand (backward sweep over the interior with x2 in the Schur entries).  ns = 0 is the plain analysis.
#pragma once
#include <vector>

#include "core.hpp"

namespace po {

constexpr int kCholNB = 32;      // block width of a blocked front
constexpr int kCholSmall = 32;   // a front of order <= this is factored by one wavefront in LDS
constexpr int kCholTile = 64;    // trsm row chunk and edge of an update tile (one workgroup)
constexpr int kCholChunk = 32;   // target columns of a front that one assembling workgroup owns
constexpr int kCholMaxRhs = 32;  // right-hand sides per solve sweep
constexpr int kCholTiny = 8;     // a front of order <= this may be packed: a whole group of them is run by one lane
constexpr int kCholLongRow = 32; // a row of the retained matrix with more entries is multiplied by a whole wavefront
// Fronts per packed group at most: the default of SW_CHOL_PACK, 0 = no packing.  It IS 0: on the chain pattern every
// cap from 8 to 64 is several times faster than no packing, but on the grid patterns every one of them is 1 - 7 %
// slower (a lane walks its group's fronts one after the other in levels that launch their other fronts anyway), and
// the cap was to be the best one that costs the grids nothing (HISTORY.md, profiles/r19_bench_chol_packing.jsonl).
constexpr int kCholPackMax = 0;
// Panel width of the dense sweeps with the factored Schur complement (a multiple of kCholNB): the default of
// SW_CHOL_SCHUR_W, read by chol_analyse.  Chosen from {64, 128, 256} by tools/bench_sparse_schur_solve.py.
constexpr int kCholSchurW = 128;
constexpr int kCholSchurRows = 64;  // rows of the Schur front that one workgroup of the forward update owns
constexpr int kCholSchurCols = 8;   // right-hand sides a workgroup of the forward update / backward gather carries

struct CholSymbolic {
  int n = 0, order = 0;
  std::vector<int> colp, rows;   // the creation pattern as given
  std::vector<int> perm, iperm;  // perm[new] = old
  int nsn = 0;
  std::vector<int> sn_first;     // nsn + 1
  std::vector<int> sn_parent, sn_level, sn_of;
  std::vector<int> sn_b, sn_ld, upd_ld;
  std::vector<int64_t> rows_ptr;     // nsn + 1, into below_rows and rel
  std::vector<int> below_rows, rel;  // rel: position of each below-row in the PARENT's front
  std::vector<int64_t> panel_off, upd_off, sol_off;
  int64_t Lsize = 0, arena = 0, sol_arena = 0;
  std::vector<int> child_ptr, child;
  int nlev = 0;
  // Packed groups (SW_CHOL_PACK, read by chol_analyse).  A front is tiny when its order is <= kCholTiny and packable
  // when it and its whole subtree are tiny; a packable subtree of at most pack_cap fronts whose parent's subtree is not
  // one is a group, and every tiny front left over is a group of one.  Group g = fronts grp_first[g] .. grp_root[g]
  // (postorder: the subtree of its root), run by ONE lane in the launches of level grp_level[g] = sn_level[root];
  // ascending by first front.  glev_first / glev_root list them level by level for the device.
  int pack_cap = 0;
  std::vector<int> front_order;  // nsn: s + b
  std::vector<int> grp_first, grp_root, grp_level;
  std::vector<int> glev_ptr, glev_first, glev_root;
  // level l = the UNPACKED supernodes lev_sn[lev_ptr[l] .. lev_ptr[l+1]): the small fronts first (lev_nsmall[l] of
  // them), then the blocked ones with the most block columns first, so the fronts that still have block column kb
  // form a prefix
  std::vector<int> lev_ptr, lev_sn, lev_nsmall;
  std::vector<int> chunk_ptr, chunk_sn, chunk_c0;  // assembling workgroups of each level
  // block column kb of level l: step = step_ptr[l] + kb; step_nact fronts take part; tab[step_tab[step] .. + nact]
  // is the running count of their row tiles (a trsm chunk, or a row of update tiles, each)
  std::vector<int> step_ptr, step_nact, step_tab, tab;
  // value scatter of the creation pattern: destination d (asm_dst, an offset into L) sums asm_src[asm_ptr[d] ..]
  std::vector<int> asm_ptr, asm_src;
  std::vector<int64_t> asm_dst;
  int64_t nnzL = 0, work_bytes = 0;
  int max_s = 0, max_front = 0;
  // The retained matrix (chol_matrix_table, built when keeping is switched on): the FULL symmetric matrix in
  // elimination order as compressed rows sorted by column.  mat_vidx indexes the compact value array, one double per
  // destination of the value scatter (asm_dst.size() of them), so the two copies of an off-diagonal entry share one.
  // mat_long lists the rows of more than kCholLongRow entries: a wavefront multiplies each, a lane every other row.
  std::vector<int> mat_rowp, mat_col, mat_vidx, mat_long;
  int mat_maxrow = 0;  // entries of the longest row
  // Schur set (header comment): schur = the set in the caller's order = perm[n - ns ..]; schur_sn = its supernode
  // (-1: none).  Factorization: destination d (schur_dst, an offset into L, lower triangle of the Schur panel) adds
  // arena[schur_src[schur_ptr[d] ..]] in child order.  Forward sweep: Schur row i adds, for right-hand side r,
  // arena[schur_vsrc[q] + r * schur_vld[q]], q in schur_vptr[i] .. schur_vptr[i + 1], in child order.
  int ns = 0, schur_sn = -1;
  int schur_w = kCholSchurW;  // panel width of the dense sweeps with the factored S (SW_CHOL_SCHUR_W)
  std::vector<int> schur;
  std::vector<int64_t> schur_ptr, schur_src, schur_dst;
  std::vector<int64_t> schur_vptr, schur_vsrc;
  std::vector<int> schur_vld;
  int64_t ldy() const { return ((int64_t)n + 3) / 4 * 4 + 4; }
};

// What one level launches: the launchers of sparse_chol.hip loop over this and chol_kernel_forms counts it.
struct CholLevelPlan {
  int nchunk, nsmall, nsteps;  // factorization: assembling workgroups, one-wavefront fronts, block columns
  int nfront;                  // sweeps: unpacked fronts, a workgroup each
  int ngroup;                  // packed groups: a lane each (factorization), a lane per right-hand side (sweeps)
  int nschur;                  // 1 at the level of the Schur supernode: its gather launch (factorization, forward sweep)
};
inline CholLevelPlan chol_level_plan(const CholSymbolic &s, int l) {
  return {s.chunk_ptr[l + 1] - s.chunk_ptr[l], s.lev_nsmall[l], s.step_ptr[l + 1] - s.step_ptr[l],
          s.lev_ptr[l + 1] - s.lev_ptr[l], s.glev_ptr[l + 1] - s.glev_ptr[l],
          s.schur_sn >= 0 && s.sn_level[s.schur_sn] == l && !s.schur_dst.empty() ? 1 : 0};
}
enum CholForm {
  CHF_ASSEMBLE, CHF_SMALL, CHF_BLOCKED, CHF_PACK_FACTOR, CHF_FWD, CHF_BWD, CHF_PACK_FWD, CHF_PACK_BWD, CHF_COUNT
};
const char *chol_form_name(int form);
// counts[form] = the levels that launch the form: in one factorization, and in one forward and one backward sweep over
// nv right-hand sides (every slab of kCholMaxRhs columns counts its levels again)
void chol_kernel_forms(const CholSymbolic &s, int nv, int counts[CHF_COUNT]);
// the forms a handle with a Schur set launches on top of those: names after chol_form_name(CHF_COUNT + f)
enum CholSchurForm { CHF_SCHUR_GATHER, CHF_SCHUR_FWD, CHF_SCHUR_COUNT };
void chol_schur_forms(const CholSymbolic &s, int nv, int counts[CHF_SCHUR_COUNT]);
// row tiles of a front of order m with sz columns once block column kb is through: a trsm chunk, or a row of update
// tiles, each.  The launch tables of every blocked front are made of it, the Schur front's own (schurFactor) too.
inline int chol_row_tiles(int sz, int m, int kb) {
  const int r0 = sz < (kb + 1) * kCholNB ? sz : (kb + 1) * kCholNB;
  return (m - r0 + kCholTile - 1) / kCholTile;
}
// The panel loop of the dense sweeps with the factored Schur complement (sparse_chol.hip, "dense sweeps"): panels of W
// columns of the ns x ns triangle.  Forward, right-looking, ascending: diag(p0, w), then below(p0, w) where rows lie
// under the panel.  Backward, left-looking, descending: below(p0, w) where rows lie under the panel, then diag(p0, w).
// Every call is one launch; the count is returned, so the launcher and po_sparse_chol_schur_solve_info share the loop.
template <class Diag, class Below>
int chol_schur_panels(int ns, int W, bool forward, Diag diag, Below below) {
  const int np = (ns + W - 1) / W;
  int launches = 0;
  for (int i = 0; i < np; i++) {
    const int p0 = (forward ? i : np - 1 - i) * W, w = ns - p0 < W ? ns - p0 : W;
    const bool under = p0 + w < ns;
    if (!forward && under) below(p0, w), launches++;
    diag(p0, w), launches++;
    if (forward && under) below(p0, w), launches++;
  }
  return launches;
}
// launches of one forward and one backward dense sweep over one slab (the sign pass of an LDLT solve not counted)
int chol_schur_solve_launches(const CholSymbolic &s);
// the levels of the factorization that launch anything
int chol_factor_levels(const CholSymbolic &s);
// po_sparse_chol_packing / po_csr_symbolic_frontal_packing (paropt_amd.h)
void chol_packing(const CholSymbolic &s, int64_t info[4], const int **group_first, const int **group_root,
                  const int **group_level, const int **front_order, const int64_t **upd_off);

// PO_OK or PO_ERR_ARG with a message; pure host code
int chol_analyse(int64_t size, const int *colp, const int *rows, int order, const int *perm, CholSymbolic *out);
// the same with a Schur set of nschur distinct unknowns (header comment); NATURAL with perm: perm must end with the set
int chol_analyse(int64_t size, const int *colp, const int *rows, int order, const int *perm, int64_t nschur,
                 const int *schur, CholSymbolic *out);
// the scatter table of any pattern onto the factor: entries at the permuted-lower position, in entry order per
// destination (the reference's setValues, src/ParOptSparseCholesky.cpp:205-252); an entry outside the pattern of L is
// PO_ERR_ARG (the reference drops it silently)
int chol_scatter_table(const CholSymbolic &s, int64_t n, const int *colp, const int *rows, std::vector<int> *ptr,
                       std::vector<int64_t> *dst, std::vector<int> *src);
// the retained matrix's compressed rows (mat_*) from the scatter table of the creation pattern; pure host code
void chol_matrix_table(CholSymbolic *s);

class SparseChol {
 public:
  SparseChol(Ctx *c) : ctx(c) {}
  CholSymbolic sym;
  Ctx *ctx;  // null: analysis only
  // after chol_analyse: device tables, L, arena.  embedded: the owner assembles L itself (beginAssembly) and solves
  // through sweep(), so the value scatter, its staging array and the right-hand-side buffer are not allocated
  int upload(bool embedded = false);
  int setValuesDevice(const double *dvals);
  int setValuesHost(int64_t n, const int *colp, const int *rows, const double *vals);
  int factor(int *info);
  // PO_CHOL_LLT (default) or PO_CHOL_LDLT: P A P^T = L S L^T, S = diag(+-1), for symmetric quasi-definite matrices
  // (no pivoting; sparse_chol.hip, "signed forms").  Read by the next factor(); a solve follows the kind of the
  // factorization it solves with.  The first LDLT allocates the sign array (n doubles, elimination order).
  int setFactorization(int kind);
  int factorization() const { return kind; }
  // {positive, negative, replaced} pivots of the last factor(), counted on the device and read with its flag.  LLT:
  // {n, 0, 0}, or PO_ERR_ARG after a factorization that replaced pivots (its kernels do not count them)
  int inertia(int64_t out[3]) const;
  int solveDevice(double *dx, int nrhs, int64_t ldx);
  int solveHost(double *x, int nrhs, int64_t ldx);
  // SCHUR COMPLEMENT (sym.ns > 0).  getSchur*: the full symmetric ns x ns S, column-major, in the caller's Schur
  // order, after factor() until the next setValues*.  condense / expand: the two halves of the solve, in place in the
  // caller's numbering; between them the interior entries hold an opaque intermediate.
  int getSchurDevice(double *dS, int64_t lds);
  int getSchurHost(double *S, int64_t lds);
  int condenseDevice(double *dx, int nrhs, int64_t ldx);
  int condenseHost(double *x, int nrhs, int64_t ldx);
  int expandDevice(double *dx, int nrhs, int64_t ldx);
  int expandHost(double *x, int nrhs, int64_t ldx);
  // the Schur front's assembly alone, for measurements (tools/bench_sparse_schur.py): the table-driven gather, or the
  // same sums by chol_assemble_kernel over a chunk list of that front; `reps` launches on the stream, no host read.
  // The front accumulates, so the values in it are meaningless afterwards: set values again before factor().
  int schurAssemblyProbe(bool chunked, int reps);
  // FACTORED SCHUR COMPLEMENT (opt-in; nothing below is allocated or launched before the first schurFactor*).
  // schurFactor*: valid after factor() until the next setValues*; copies the lower triangle of S into a buffer F of
  // its own (ns x ns, column-major, leading dimension rounded as a front's), adds the lower triangle of `add`
  // (optional; symmetric ns x ns in the order of the set, column-major, ldadd >= ns) entry by entry and factors
  // S~ = S + add in place with the block-column kernels of the fronts, in the kind of the factor() that produced S
  // (LDLT: the signs go to d_sign[n - ns ..]).  *info = 0, or 1 + the permuted index n - ns + k of the first pivot
  // replaced.  The Schur front itself is not touched: getSchur* keeps returning S, and schurFactor* may be called
  // again with another add.  Afterwards solveDevice / solveHost work on the handle (the whole solve), and
  // solveRefined* too when there was no add (the retained A is then the matrix solved).
  int schurFactorDevice(const double *dadd, int64_t ldadd, int *info);
  int schurFactorHost(const double *add, int64_t ldadd, int *info);
  // S~ x2 = g in place on ns-vectors in the order of the set, nrhs columns at x2 + j ldx2
  int schurSolveDevice(double *dx2, int nrhs, int64_t ldx2);
  int schurSolveHost(double *x2, int nrhs, int64_t ldx2);
  // {positive, negative, replaced} pivots of S~ (sum ns); the LLT rule of inertia()
  int schurInertia(int64_t out[3]) const;
  bool schurFactored() const { return schur_factored; }
  int64_t schurFactorBytes() const { return fbytes; }
  // RETAINED MATRIX (opt-in).  A is the symmetric matrix whose permuted lower triangle the value scatter sums into the
  // factor (the rule of chol_scatter_table).  While keeping is on, every setValues* also sums the compact values
  // `aval` (the same sums, bit for bit); factor() leaves them alone.  On an analysis-only object only the tables.
  int setKeepMatrix(bool on);
  bool keepMatrix() const { return keep; }
  // shift (host, size doubles, the user's numbering; null clears): the next setValues* adds shift[perm[k]] to the
  // diagonal entry k of L after the scatter, so factor() factors A + diag(shift); aval does not get it
  int setDiagonalShift(const double *shift);
  // y = A x in the user's numbering, nrhs columns (x at dx + j ldx, y at dy + j ldy), queued on the context's stream
  int matvecDevice(const double *dx, int64_t ldx, double *dy, int64_t ldy, int nrhs);
  int matvecHost(const double *x, int64_t ldx, double *y, int64_t ldy, int nrhs);
  // Solve and refine against the retained A (sparse_chol.hip, "refined solve"): per column j the steps taken,
  // eta before the first correction and eta of the x returned (each pointer nullable, nrhs entries).
  // max_steps < 0: 5; tol < 0 or NaN: eps.
  int solveRefinedDevice(double *dx, int nrhs, int64_t ldx, int max_steps, double tol, int *steps, double *eta0,
                         double *eta);
  int solveRefinedHost(double *x, int nrhs, int64_t ldx, int max_steps, double tol, int *steps, double *eta0,
                       double *eta);
  // The interior point's side (csr.cpp: CsrSparse).  beginAssembly queues the zeroing of L and hands it out: the
  // caller writes lower(P A P^T) at the offsets of asm_dst with kernels of its own on the same stream.
  // factorAssembled queues the numeric factorization of what was written and returns without a host read: a
  // non-positive pivot is replaced by 1, flag[0] is set and flag[1] takes the smallest permuted index (the caller
  // sets flag[0] = 0 and flag[1] above every index beforehand, and reads them when it likes).  Always the unsigned
  // (L L^T) kernels.
  int beginAssembly(double **Lout);
  int factorAssembled(int *flag);
  // Triangular sweeps over a panel given as a HOST table of nv device vectors that are already in the elimination
  // order, in place: forward Y <- L^-1 Y, backward Y <- L^-T Y, or both.  No permutation, no copy; any nv (slabs of
  // kCholMaxRhs columns).  Every column is solved by the same operations whatever nv is.
  int sweep(double *const *Y, int nv, bool forward, bool backward);

 private:
  struct DevTables;       // the table of device pointers every kernel takes (sparse_chol.hip: CholDev)
  DevTables dev() const;
  int scatter(const int *d_ptr, const int64_t *d_dst, const int *d_src, int64_t ndst, const double *dvals);
  template <bool kSigned>
  int launchFactor(int *flag);
  // forward sweep, sign pass (LDLT), backward sweep on a panel of nr columns in elimination order, in place
  void solvePanel(double *P, int nr);
  int needMatrix(const char *who);
  int matrixNorm();
  // R = B - A X (B null: R = A X) on panels in elimination order; stats (device, null: none) takes the bit patterns of
  // max|r| and max|x| per column
  void productPanel(const double *X, const double *B, double *R, int nr, unsigned long long *stats);
  int hostBuffer(int64_t count);
  int refuseWholeSolve(const char *who) const;
  int halfSolveCheck(const char *who, int nrhs, int64_t ldx);
  int halfSolveHost(bool condense, double *x, int nrhs, int64_t ldx);
  void launchSchurGather(int reps);
  void launchSchurFwd(double *P, int nr);
  int schurFactorCheck(const char *who, int64_t ldadd);
  template <bool kSigned>
  void launchSchurFactor(int *flag);
  // forward or backward dense sweep with F in place on ns rows at Yb (leading dimension ld), nr columns
  void schurSweep(double *Yb, int64_t ld, int nr, bool forward);
  bool keep = false, have_aval = false, have_anorm = false;
  double anorm = 0.0;
  DevArray<int> d_mrowp, d_mcol, d_mvidx, d_mlong, d_sn_of;
  DevArray<double> aval, d_shift, Bp, Xp, ybuf;
  DevArray<unsigned long long> d_stats;  // 3 x kCholMaxRhs column maxima (r, x, b) and ||A||_inf, as bit patterns
  int64_t ybuf_cap = 0;
  bool have_values = false, factored = false, have_inertia = false, uncounted = false;
  int kind = 0, factored_kind = 0;
  int64_t inertia_[3] = {0, 0, 0};
  // every device array is freed with the object and counted by po_live_objects (core.hpp: DevArray)
  DevArray<double> d_sign;  // s_k = +-1.0 in elimination order (LDLT)
  DevArray<double> L, arena, Y, avals, xbuf;
  int64_t xbuf_cap = 0;
  DevArray<int> d_flag;
  DevArray<int> d_perm, d_first, d_b, d_ld, d_uld;
  DevArray<int> d_below, d_rel, d_child_ptr, d_child;
  DevArray<int64_t> d_rows_ptr, d_panel, d_upd, d_sol;
  DevArray<int> d_glev_first, d_glev_root;
  DevArray<int> d_lev_sn, d_chunk_sn, d_chunk_c0, d_tab;
  DevArray<int> d_asm_ptr, d_asm_src;
  DevArray<int64_t> d_asm_dst;
  // Schur set only (never allocated without one)
  bool schur_ready = false;
  DevArray<int64_t> d_schur_ptr, d_schur_src, d_schur_dst, d_schur_vptr, d_schur_vsrc;
  DevArray<int> d_schur_vld, d_probe_sn, d_probe_c0;
  DevArray<double> sbuf;
  int64_t sbuf_cap = 0;
  // factored Schur complement (never allocated before schurFactor*): F, its one-front table for the factorization
  // kernels (ftab_i: first[2], nb, ld, uld, list, then the row-tile counts {0, tiles} of every block column;
  // ftab_l: panel, upd), a flag block of its own
  bool schur_factored = false, schur_added = false, schur_have_inertia = false;
  int64_t schur_inertia_[3] = {0, 0, 0};
  int64_t fbytes = 0;
  int ldF = 0;
  DevArray<double> F, addbuf;
  DevArray<int> ftab_i, d_sflag;
  DevArray<int64_t> ftab_l;
};

}  // namespace po
