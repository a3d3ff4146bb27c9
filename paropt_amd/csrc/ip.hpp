// Host-side mirror of ParOptInteriorPoint (reference src/ParOptInteriorPoint.h:128-217) for the
// quasi-Newton branch: dense constraints, plus the sparse "weighting" constraints with nwblock = 1
// (ip_w.cpp).  Same public method names, option names/defaults and return codes; every n- or
// w-sized operation is a HIP kernel launch (core.hpp, wcon.hpp).
#pragma once
#include <stdlib.h>
#include <map>
#include <string>
#include <vector>

#include "bordered.hpp"
#include "problem.hpp"
#include "qn.hpp"

namespace po {

// Typed option registry with the names, defaults and ranges of
// ParOptInteriorPoint::addDefaultOptions (src/ParOptInteriorPoint.cpp:536-727).
class Options {
 public:
  enum Type { STR = 1, BOOL = 2, INT = 3, FLOAT = 4, ENUM = 5 };
  struct Entry {
    Type type;
    std::string s;
    int i = 0, ilo = 0, ihi = 0;
    double f = 0, flo = 0, fhi = 0;
    std::vector<std::string> choices;
  };
  Options();
  // ParOptTrustRegion::addDefaultOptions (src/ParOptTrustRegion.cpp:739-847) into the same registry
  void addTrustRegionDefaults();
  // ParOptMMA::addDefaultOptions (src/ParOptMMA.cpp:234-289)
  void addMMADefaults();
  int set(const char *name, const char *value);
  int set(const char *name, int value);
  int set(const char *name, double value);
  const char *str(const char *name) const;
  int integer(const char *name) const;
  double real(const char *name) const;
  bool has(const char *name) const { return e.count(name) > 0; }
  // calls fn for every entry that `skip` (may be null) does not hold: po_options_visit_defaults
  int visit(const Options *skip, po_option_visitor fn, void *user) const;
  // takes over every entry of `src` that `base` does not hold (the trust-region / MMA options of a driver whose
  // interior-point solver was created separately: one registry serves both, as in the reference)
  void adoptExtras(const Options &src, const Options &base);

 private:
  std::map<std::string, Entry> e;
};

// the iteration table of a solver, written to `fname` on the root rank when optimize() returns (empty name: no file)
void write_history_file(Ctx *ctx, const std::string &fname, const char *solver, const std::string &history);

class InteriorPoint {
 public:
  InteriorPoint(Problem *prob);
  ~InteriorPoint();
  int allocate();  // device storage (fails with PO_ERR_HIP when HBM is exhausted)
  // SURVEY 8a' bookkeeping (po_ip_get_debug_ints)
  const std::vector<int> &gPivots() const { return kkt.gpiv; }
  Vec *lowerBounds() { return lb; }
  Vec *upperBounds() { return ub; }
  // the caller may write lb / ub through a handle: the kernels read the vectors until the next optimize()
  void clearUniformBounds() { bounds_uni[0] = bounds_uni[1] = 0; }
  int checkFlag() const { return check_flag; }
  int clampCounts(double out[8]);
  // checkKKTStep (:6212-6360), step_verification_frequency: appends the block maxima of the linearised KKT
  // residual at the current (unscaled) step to the iteration history
  int checkKKTStep(int iteration, double mu);

  Options options;
  int optimize(const char *checkpoint);
  void getOptimizedPoint(Vec **x, const double **z, Vec **zl, Vec **zu);
  void getOptimizedSlacks(const double **s, const double **t, const double **zs, const double **zt);
  void getOptimizedSparse(Vec *v[5]);  // zw, sw, tw, zsw, ztw (null when nwcon = 0)
  void getIterationCounters(int *niter_, int *neval_, int *ngeval_);
  double getBarrierParameter() const { return barrier_param; }
  int getComplementarity(double *comp);
  void setPenaltyGamma(double gamma);
  void setPenaltyGammaArray(const double *gamma);  // per-constraint values (:1160-1172)
  int resetDesignAndBounds();
  void resetQuasiNewtonHessian();
  // drivers that own the quasi-Newton object / swap the problem (trust region): :1193-1234, :745-764
  int setQuasiNewton(CompactQuasiNewton *qn_);
  int resetProblemInstance(Problem *p);
  int writeSolutionFile(const char *filename);
  int readSolutionFile(const char *filename);
  int debugKKTStep(double mu);
  // State-injected known-answer tests (po_ip_debug_set_state / po_ip_debug_kkt): the caller has written x, zl, zu
  // (and the sparse blocks) through the borrowed handles; this takes the dense blocks and mu, evaluates the problem
  // at x (objective, constraints, gradient, Jacobian) and drops every quantity carried between passes.
  int debugSetState(const double *z, const double *s, const double *t, const double *zs, const double *zt, double mu);
  // mode 0: residual + Schur complements + ONE bordered solve, the stored-step kernels (computeKKTStep :2700-2737);
  // mode 1: the sequence of a plain quasi-Newton iteration of optimize() -- dinv_d1, the fused Gram pass (unformed
  //         L-SR1 columns), first solve pass with the refinement's products, refinement pass -- with the
  //         bound-multiplier steps stored.  Afterwards the matrices AS ASSEMBLED are kept in Gmat0 / Ce0.
  int debugKKT(double mu, int mode, double tau);
  std::vector<double> Gmat0, Ce0;   // G and Ce before their LU factorizations (filled inside debugKKT only)
  bool debug_keep_schur = false;
  double debug_norms[4] = {0, 0, 0, 0};  // max_prime, max_dual, max_infeas, res_norm of the last debugKKT
  const std::vector<double> &gramMatrix() const { return kkt.W; }
  const std::vector<int> &cPivots() const { return kkt.cpiv; }
  const double *stepMins() const { return step_mins; }
  Vec *dinvVec() { return Dinv; }
  Vec *rxVec() { return rx; }
  void flushHistory();
  // checkGradients(dh) (:6196-6199): the problem's finite-difference check at the current point; the report text
  // (what the reference prints) is returned
  int checkGradients(double dh, std::string *report);
  // checkMeritFuncGradient(xpt, dh) (:3280-3432): forward difference of the merit function along the current step
  // (xpt == nullptr) or, from xpt, along -g/|g| with the reference's fixed slack steps; out = {fd, actual}
  int checkMeritFuncGradient(Vec *xpt, double dh, double out[2]);
  // Hessian-vector products by differences of the Lagrangian's gradient (ip_hvec_fd.cpp; no reference counterpart).
  // mode: PO_HVEC_EXACT (the problem's evalHvecProduct, the default), PO_HVEC_FD_WHEN_MISSING (differences from the
  // first evalHvecProduct that returns non-zero on), PO_HVEC_FD_ALWAYS; rel_step <= 0: the default of the form
  int setHvecFiniteDifference(int mode, int central, double rel_step);
  // differenced products so far and the evalObjCon + evalObjConGradient pairs they cost (NOT part of neval / ngeval,
  // which keep counting the evaluations the algorithm asked for); both restart with optimize()
  void getHvecFiniteDifferenceCount(int *products, int *evaluations) const;
  double hvecFiniteDifferenceStep() const { return hvec_fd_h; }  // h of the last differenced product (0: none yet)
  // hvec = H(x, z, zw) p at the current point by the configured mode (p, hvec: two different n-sized vectors)
  int evalHvec(const double *z, Vec *zw, Vec *p, Vec *hvec);

  Problem *prob;
  Ctx *ctx;
  int64_t n;
  int c;
  CompactQuasiNewton *qn;
  po_qn_s qn_handle;

  // state
  Vec *x, *zl, *zu, *lb, *ub, *g;
  std::vector<Vec *> Ac;
  Dense vars, res, step, refine;
  double fobj, barrier_param, rho_penalty_search;
  std::vector<double> cvals;
  int niter, neval, ngeval, nhvec;

  // observer + history
  po_ip_iteration_fn iter_cb;
  void *iter_cb_user;
  std::string history;
  std::vector<std::string> phase_names;
  std::vector<double> phase_seconds;
  std::string phase_names_joined;
  // Event timing of the problem's callbacks (the "user_eval" phase).  Off by default: every event record
  // is a packet between two kernels and costs the stream dispatch latency -- 850 / 853 against 863 / 866 inner it/s
  // at config 5 in one call (5-6 callbacks per 1.2 ms inner iteration), nothing measurable at n >= 10 M.
  // po_ip_set_callback_timing switches it on (bench.py does, for the figure it reports).
  bool user_timing = dbg_switch(SW_USER_TIMING) != 0;

  // step storage (exposed for the single-step known-answer tests)
  Vec *px, *pzl, *pzu;

  // sparse constraint blocks (nwblock = 1): zw, sw, tw, zsw, ztw of the variables / residual / step
  int64_t nw;        // local number of sparse constraints
  bool has_w;        // some rank has sparse constraints (uniform across ranks)
  double nw_global;  // total count (for the complementarity average)
  Vec *wvar[5], *wresv[5], *wstepv[5];

 private:
  // work vectors
  Vec *Dinv, *rx, *tvec, *xt, *y_qn, *s_qn;
  Vec *vA;  // A^T pz of the current (unscaled) step, accumulated by the solves
  std::vector<double> gamma_s, gamma_t;
  int use_lower, use_upper;
  bool qn_created;
  bool qn_owned;

  // small dense systems: the weighted Gram W of the panel and the factors of the bordered solve
  Bordered kkt;
  std::vector<double> Wt_buf, W2_buf;  // landing areas of Gram launches deferred to a batch flush (setUpKKTSystem)
  // the head solveKKT and solveKKTW share, and what every pass form of theirs is handed: the panel, its coefficients
  // in the step (sol.coef) and the scalars of the solve
  Bordered::Sol solveBordered(const Dense &b, const double *dots, bool refine_pass);
  struct SolvePass {
    const std::vector<const double *> &P;
    const std::vector<double> &alpha;
    int m;
    double beta_mu, tau;
  };

  // What the carried buffers and caches hold, grouped by the event that makes them stale.  Each group is dropped as a
  // whole by its event method (group = {}: a member added later cannot be missed); a flag consumed by the one pass
  // that reads it is cleared there.  The values recorded with a flag sit below its group.
  struct StepFlags {  // the current step in px / pzl / pzu and what was taken of it; stale when a solve writes a step
    bool ptpx_valid = false;           // ptpx = P^T px
    bool tdots_valid = false;          // tdots = P^T t' of the fused first pass (consumed by the refinement pass)
    bool merit_cache_valid = false;    // merit_cache
    bool fused_merit_valid = false;    // fused_merit
    bool px_amax_valid = false;        // px_amax_w
    bool w_comp_valid = false;         // w_comp_poly
    bool w_merit_cache_valid = false;  // w_merit_cache
    bool vA_valid = false;             // vA = A^T pz, maintained by the solves
    bool residual_fused = false;       // the first pass already wrote the refinement right-hand side t'
    bool pz_stored = true;             // pzl / pzu hold the step (false after a lean step: px only; step_beta_mu)
    bool step_deferred = false;        // the first pass stored no step (alpha_first, coef_first, diag_first)
    bool px_first_only = false;        // sparse path: the first pass stored px only
  } step_flags;
  // P^T px of the current (unscaled) step, P = [Ac | Z]: maintained analytically from the solves
  // (px = t + Dinv*(P alpha)  =>  P^T px = P^T t + W alpha), so that neither iterative refinement
  // nor the merit derivative needs another pass over the panel
  std::vector<double> ptpx;
  std::vector<double> tdots;
  // merit pieces of the current (unscaled) step, produced together with the complementarity check of scaleKKTStep
  MeritSums merit_cache;
  // the same pieces taken by the refinement pass itself (k_solve2r with g), or handed over by the corrector solve
  // (corr_out: what k_solve2c reduced); the log-barrier sums of the iterate are those of the accepted trial point of
  // the last line search (same kernel arithmetic, same element order as the separate pass took them)
  FusedMeritSums fused_merit;
  CorrectorSums corr_out;
  double px_amax_w = 0.0;  // max|px| taken inside evalMeritInitDeriv's batch (sparse-constraint path)
  // Sparse constraints: the sparse blocks' share of the complementarity polynomial comes out of the step kernel
  // (w_step_out -> w_comp_poly) and the sparse merit sums ride in the refinement's batch (w_merit_cache, at sx = 1)
  double w_step_out[5] = {0, 0, 0, 0, 0}, w_comp_poly[3] = {0, 0, 0}, w_merit_cache[10] = {0};
  // Lean step: in the plain quasi-Newton iteration the refinement pass stores px only; the bound-multiplier steps are
  // re-formed from it inside the multiplier update (kkt_res_update_kernel, with the barrier term step_beta_mu of the
  // step's solve) -- two output streams of the refinement pass less.  lean_step_allowed is set by optimize() around the
  // step computation of an iteration whose every later consumer of (pzl, pzu) is that update.
  bool lean_step_allowed = false;
  double step_beta_mu = 0.0;
  std::vector<double> alpha_first, coef_first;  // coefficients of a deferred first pass (solve, refinement residual)
  double diag_first = 0.0;
  double step_mins[2];         // fraction-to-boundary minima {max_x, max_z} of the current step
  double sx = 1.0, sz = 1.0;  // lazily applied step scalings (scaleKKTStep :3253-3268)

  // what the scratch vectors tvec, Dinv, d1v, wd2 and Uw hold; stale when they are lent out (checkGradients) or the
  // state is written from outside
  struct ScratchFlags {
    bool spec_dt_valid = false;         // Dinv / t of the next first solve (spec_dt_diag, spec_dt_bmu, spec_dt_mu)
    bool t0_valid = false;              // tvec = t of the next first solve, t0dots = P^T t (t0_mu)
    bool t_is_plain_dinv_d1 = false;    // tvec / Dinv are exactly what dinv_d1_kernel forms (t0_diag)
    bool first_t_recomputable = false;  // ... and the first solve's t can be re-formed in registers
    bool wd2_ready = false;             // wd2 = d2 of the next block solve
    bool panel_valid = false;           // Uw is the panel image of the current setUpKKTSystem (panel_form)
  } scratch_flags;
  // Dinv / t of the next first solve left behind by the residual pass of the new point when no quasi-Newton update
  // comes in between (spec_dt_want); valid for the diagonal and the barrier parameter recorded with them
  bool spec_dt_want = false;
  double spec_dt_diag = 0.0, spec_dt_bmu = 0.0, spec_dt_mu = 0.0;
  double t0_mu = 0.0;
  std::vector<double> t0dots;  // P^T t of the next first solve, out of setUpKKTSystem's Gram pass
  // tvec / Dinv hold exactly what dinv_d1_kernel formed for (t0_diag, t0_mu) from the bound data and rx: a pass that
  // loads those anyway may re-form them in registers instead of reading them (k_solve2r with t1 == nullptr)
  double t0_diag = 0.0;

  // what was evaluated at the current iterate x; stale when x, the bounds or the problem instance change other than
  // by the step update
  struct IterateFlags {
    bool ac_valid = false;            // Ac holds the Jacobian at x
    bool acz_valid = false;           // acz = A^T z (acz_age)
    bool cwx_valid = false;           // cwx = cw(x)
    bool trial_cw_valid = false;      // wtmp = cw(xt) of the last trial point
    bool iterate_logs_valid = false;  // iterate_logs
    bool trial_logs_valid = false;    // trial_logs
    bool residual_cached = false;     // rx / norms of the current state were already evaluated (step update)
    bool spec_valid = false;          // spec_max for spec_mu
    bool s_qn_from_trial = false;     // s_qn holds s_qn_a * px, written by the last trial pass of the line search
  } iterate_flags;
  // A^T z of a problem with linear dense constraints, kept by recurrence (computeResidual / computeStepAndUpdate)
  static const int kAczRefresh = 16;
  Vec *acz = nullptr;
  int acz_age = 0;
  double trial_logs[2] = {0, 0}, iterate_logs[2] = {0, 0};
  // Monotone barrier strategy with the infinity norm: the residual pass also takes max|rzl|, max|rzu| for the barrier
  // parameter the strategy would switch to (a function of the current one alone), so that the switch needs neither
  // the mu-only pass over the bound data nor its host synchronisation
  bool spec_enabled = false;
  double spec_mu = 0.0, spec_max[2] = {0.0, 0.0};
  double s_qn_a = 0.0;

  void stepWillChange() { step_flags = {}; }
  void scratchLent() { scratch_flags = {}; }
  void iterateReplaced() { iterate_flags = {}; }
  void stateReplaced() {  // x, the multipliers or the problem written from outside: nothing carried survives
    stepWillChange();
    scratchLent();
    iterateReplaced();
  }

  // residual bookkeeping of the last computeResidual call; res_out / wres_out: landing areas of its reductions (inside
  // a BatchScope the values arrive at the flush, see after_reduce)
  ResidualSums res_out;
  double wres_out[12] = {0};
  double comp_prod, comp_count, max_rx, max_rzl, max_rzu;
  double l1_rx = 0, l1_rzl = 0, l1_rzu = 0, l2_rx = 0, l2_rzl = 0, l2_rzu = 0;
  bool corrector_active;  // Mehrotra predictor-corrector: s_qn / y_qn hold the corrector products
  // ... unless the corrector solve forms them itself (k_corr_d1_dots + k_solve2c)
  bool corrector_fused = false;
  int norm_type;  // 0 infinity, 1 l1, 2 l2 (ParOptNormType)

  // ---- second-order information (ip_gmres.cpp) ----
  Vec *hdiag;                  // use_diag_hessian: diagonal of the Lagrangian Hessian (zero until evaluated)
  std::vector<Vec *> gmresW;   // Krylov basis of computeKKTGMRESStep
  bool inexact_newton_step;    // the current step came from computeKKTGMRESStep
  int gatherCounts(int64_t mine, std::vector<int64_t> *all);
  int solutionFileOffsets(int64_t *nvars_total, int64_t *var_off, int64_t *nw_total, int64_t *w_off);
  int ensureHdiag();
  int solveKKTAlpha(const double *bx, double alpha, const Dense &b, double mu, bool use_qn, bool full,
                    double tau, Dense &out);
  int evalObjBarrierDeriv(const Dense &p, double *pmerit);
  // sparse-constraint variants of the two above (ip_gmres.cpp); wscalev = alpha-scaled copy of the w residual
  int solveKKTAlphaW(const double *bx, double alpha, const Dense &b, double mu, bool use_qn, bool full,
                     double tau, Dense &out);
  Vec *wscalev[5];
  double w_merit_last[10];  // k_w_merit sums of the last evalObjBarrierDeriv (sparse part)
  int computeKKTGMRESStep(double rtol, double atol, bool use_qn, double tau, int *gmres_iters);

  // ---- Hessian-vector products, exact or differenced (ip_hvec_fd.cpp) ----
  int hvec_mode = PO_HVEC_EXACT, hvec_central = 0;
  double hvec_rel = 0.0;        // 0: sqrt(eps) forward, cbrt(eps) central
  bool hvec_fd_active = false;  // PO_HVEC_FD_WHEN_MISSING: the problem's product has failed once
  int hvec_fd_products = 0, hvec_fd_evals = 0;
  double hvec_fd_h = 0.0;
  // scratch, allocated by the first differenced product: the perturbed point, (g, A_1 .. A_c) of the plus side and,
  // central form, of the minus side; CSR form: the iterate's Jacobian entries and constraint values while the
  // problem's arrays hold those of a perturbed point
  Vec *hvec_xp = nullptr;
  std::vector<Vec *> hvec_work[2];
  Vec *hvec_csr_data = nullptr, *hvec_csr_cw = nullptr;
  int64_t hvec_csr_nnz = 0;
  int hvecProduct(const double *z, Vec *zw, Vec *p, Vec *hvec);  // every product of the solver goes through here
  int hvecFiniteDifference(const double *z, Vec *zw, Vec *p, Vec *hvec);
  int hvecScratch(int sides, int nc);
  int hvecEvalAt(double a, Vec *p, int side, bool with_jac);

  // ---- sparse-constraint path (ip_w.cpp) ----
  Vec *gsw, *gtw, *Cw, *wd2, *wyw, *wtmp, *wtmp2;
  // cw(x) of the CURRENT iterate: the residual (twice per iteration: new barrier parameter), the
  // refinement's residual and the merit derivative all need the sparse constraint values at the same point; the
  // reference calls evalSparseCon each time (:1358, 3740), here the callback runs once per point and the accepted
  // trial point of the line search hands its values over.  Dropped whenever x or the problem instance changes.
  Vec *cwx = nullptr;
  int sparseConAtIterate(const double **cw);
  Vec *d1v;                 // n-sized: raw d1, then v = d1 + P alpha
  std::vector<Vec *> Uw;    // U_j = Aw (Dinv o P_j)
  // the report of the problem's solver at the last Gram correction (quasidef.hpp): whether Uw is still the plain
  // panel image, and whether a solved panel Yw_j = -S^-1 U_j beside it is the one sparseCorrection combines
  GramForm panel_form = {false, false};
  std::vector<Vec *> Yw;
  std::vector<const double *> correctionPanel(int m) const;  // Yw (panel_form.solved) or Uw, m columns
  double w_sums[7], w_maxs[5];  // reductions of the last w residual (k_w_res layout)
  double nextMonotoneMu() const;
  WVars wv() const;
  WVars wr() const;
  WVars wp() const;
  int allocateW();
  int applyK0(const double *bx, const double *bw, Vec *yx, Vec *yw);
  // d2out: also wd2 = d2 of the block solve that follows (one launch less); wd2_ready tells solveKKTW
  int computeResidualW(double mu, bool norms = true, bool with_d2 = false);
  int sparseGramCorrection(const std::vector<const double *> &P, int m, Vec *work = nullptr, bool may_defer = false,
                           bool panel_done = false);
  int panelImageVectors(int m, std::vector<double *> &U);  // Uw[0..m) as raw pointers (allocated on demand)
  int solveKKTW(const Dense &b, double mu, bool use_qn, bool refine_pass, double tau, Dense &out,
                bool fuse_residual = false);
  // its pass forms (ip_w.cpp); mins_x / mins_w: the fraction-to-boundary minima of the design and sparse blocks
  int fusedFirstPassW(const SolvePass &sp, int k, double mins_x[2], double mins_w[2]);
  int correctionPanelSolve(const SolvePass &sp, bool refine_pass, bool first_px_only, const double *cl,
                           const double *cu, double mins_x[2], double mins_w[2]);
  int blockSolveFallback(const SolvePass &sp, bool refine_pass, const double *cl, const double *cu, double mins_x[2],
                         double mins_w[2]);
  int initLeastSquaresMultipliersW();
  int wCompStep(double ax, double az, double *prod);

  Bounds bounds() const;
  std::vector<const double *> panel(bool use_qn, int *k) const;
  // the panel of a caller that may not stream it, asked for on first use: zPointers() forms unformed L-SR1 columns
  struct LazyPanel {
    const InteriorPoint *ip;
    bool use_qn;
    bool asked = false;
    std::vector<const double *> P;
    std::vector<const double *> &get();
  };
  // P^T px of the current (unscaled) step, c + kq values: ptpx when the solves kept it, else one k_mdot pass over P
  int stepPanelDots(LazyPanel &P, std::vector<double> &dots);
  // d0 M^-1 d0 Z^T p from ztp = Z^T p (kq = qn->size() values)
  std::vector<double> compactInverse(const double *ztp, int kq) const;
  // The design rows of the linearised KKT residual at the step (addKKTResStep :1461-1483) as coefficients of the
  // panel [Ac | Z] with kq quasi-Newton columns: coef[0..c) = z, the step of the dense multipliers, and
  //   RES_SIGMA:  diag = qn_sigma (no quasi-Newton term)
  //   RES_QN:     diag = qn_sigma + b0, coef[c..c+kq) = d0 M^-1 d0 Z^T px, ztpx = Z^T px
  //   RES_HVEC, RES_HDIAG: -H px (Hessian-vector product) or -h o px, formed into xt, replaces the quasi-Newton term,
  //               sigma included: diag = 0, coef[c+kq] = -1 for xt as one more column of the caller's panel
  // The caller sizes coef and zeroes it; entries of no term are left alone.
  enum ResTerm { RES_SIGMA, RES_QN, RES_HVEC, RES_HDIAG };
  int residualCoefs(ResTerm term, const double *z, const double *ztpx, int kq, std::vector<double> &coef,
                    double *diag);

  int createQuasiNewton();
  int refreshQuasiNewton();  // validates a user-written approximation and refreshes its cached compact form
  int initAndCheckDesignAndBounds();
  int initLeastSquaresMultipliers();
  int initAffineStepMultipliers();
  void denseResidual(double mu, Dense &r) const;
  struct MultUpdate {  // a bound-multiplier step that rides in the residual pass (computeStepAndUpdate)
    double a = 0.0, az = 0.0, eps = 0.0;
    bool acz_follow = false;
  };
  int computeResidual(double mu, bool vectors, Vec *yqn_complete = nullptr, const MultUpdate *upd = nullptr);
  void resNorms(const Dense &r, double *max_prime, double *max_dual, double *max_infeas,
                double *res_norm) const;
  double compFromSums(double prod, double count, const Dense &v, double wprod = 0.0) const;
  // diag_only: keep b0 of the quasi-Newton approximation in Dinv but leave its low-rank part out
  // (the "diagonal quasi-Newton step" of :4923-4980)
  int setUpKKTSystem(bool use_qn, bool diag_only = false, const double *rhs_mu = nullptr);
  // its steps: (1) Dinv and, where the right-hand side of the first solve is known already, that vector from the same
  // pass -- t = Dinv o d1 in tvec (dense constraints) or the raw d1 in d1v (sparse constraints);
  enum RhsFormed { RHS_NONE, RHS_T, RHS_RAW_D1 };
  int formDinvAndRhs(double diag, bool use_hdiag, const double *rhs_mu, int kz, RhsFormed *formed);
  // (2) the Gram pass of the panel, (3) kkt.factor
  struct GramPlan {
    std::vector<const double *> V;  // the panel in launch order: [Ac | Z], or [Z | Ac] with kform > 0
    int kform = 0;                  // leading columns the pass forms itself: L-SR1's Z_j = Y_j - b0 S_j, V_j = Y_j
    std::vector<const double *> S;  // ... from these S_j,
    std::vector<double *> Zout;     // ... written out here for the later passes
    double b0 = 0.0;
    bool with_t = false;  // tvec rides as the pre-weighted last column: P^T t lands in t0dots
    const GramGroups *groups = nullptr;  // structured sparse constraints: the panel image rides too (k_wgram)
    bool may_defer = false;              // inside an open batch the result arrives at the flush
  };
  int gramPass(const GramPlan &plan, bool *groups_done);
  int solveKKT(const Dense &b, double mu, bool use_qn, bool refine_pass, double tau, Dense &out,
               bool fuse_residual = false);
  // the pass forms of solveKKT (ip.cpp)
  int fusedFirstPass(const SolvePass &sp, const std::vector<double> &coef, double diag);
  int recomputingRefinementPass(const SolvePass &sp, bool corr);
  int correctorSolve(const SolvePass &sp);
  int storedStepSolve(const SolvePass &sp, bool refine_pass, const double *coef2, double diag, const double *cl,
                      const double *cu);
  int computeKKTStepWithRefinement(double mu, bool use_qn, double tau);
  int mehrotraStep(bool use_qn, double comp, bool corrector, double min_frac, double abs_res_tol, double *tau_out);
  int scaleKKTStep(double tau, double comp, double *alpha_x, double *alpha_z, int *ceq,
                   bool inexact = false);
  int evalMeritInitDeriv(double max_x, double *merit, double *pmerit);
  double evalMeritFromSums(double fk, const double *ck, const double *sk, const double *tk,
                           double pos, double neg, const double *wsums = nullptr) const;
  struct TrialSums {  // of one trial point of the line search (evalTrial)
    double sums[2], wsums[5];  // barrier sums of the design block, slack sums of the sparse blocks
    int fail_obj;              // what evalObjCon returned
  };
  int evalTrial(double alpha, bool with_sparse, double eps, double *sq, TrialSums &t);
  int lineSearch(double alpha_min, double *alpha, double m0, double dm0, int *fail);
  // computeStepAndUpdate and its parts (form_point: the line search did not form this point)
  struct UpdatePlan {  // which pass carries the multiplier step and the brackets of y_qn: set by updateMultipliers
    bool do_qn = false, fast_yqn = false, fuse_upd = false, fuse_upd_noqn = false;
    MultUpdate upd;
  };
  int computeStepAndUpdate(double alpha, bool form_point, int *update_type);
  int updateMultipliers(double alpha, double eps, UpdatePlan &plan);
  void updateDenseVariables(double alpha, double eps);
  int acceptTrialPoint(double alpha, bool form_point, double eps);
  int evalGradientAtIterate();
  int quasiNewtonUpdate(double alpha, const UpdatePlan &plan, int *update_type);

  // ---- optimize() as a sequence of stages (ip.cpp, "optimize") ----
  enum class Barrier { MONOTONE, MEHROTRA, MPC, COMP_FRACTION };
  enum class StepKind { INEXACT_NEWTON, QUASI_NEWTON, SEQ_LINEAR, DIAG_QUASI_NEWTON, DIAG_HESSIAN };
  // The options optimize() reads ONCE, when it starts.  Every other option is read where it is used, each time it is
  // used, and stays so: an iteration callback may call setOption during a run (monotone_barrier_fraction / _power,
  // the Eisenstat-Walker pair, nk_switch_tol, max_gmres_rtol, gmres_atol, use_qn_gmres_precon, output_level,
  // gradient_check_step_length, min_rho_penalty_search, rel_bound_barrier and what lineSearch / computeStepAndUpdate
  // read).
  struct RunOptions {
    double abs_res_tol, rel_func_tol, function_precision, design_precision, min_fraction_to_boundary;
    Barrier barrier_strategy;  // of the input; a run starts monotone and switches at the first barrier reduction
    bool use_hvec_product, use_diag_hessian, use_quasi_newton_update, sequential_linear_method, use_line_search;
    int max_major_iters, hessian_reset_freq, write_output_frequency, step_verification_frequency,
        gradient_verification_frequency;
    std::string starting_point_strategy;
  };
  RunOptions readRunOptions() const;
  struct MajorState {  // what one major iteration hands to the next
    double fobj_prev = 0.0, alpha_prev = 0.0, alpha_xprev = 0.0, alpha_zprev = 0.0, dm0_prev = 0.0;
    double res_norm_prev = 0.0;
    int no_merit_function_improvement = 0, line_search_test = 0, line_search_failed = 0;
    std::string info;  // the tokens of the last iteration, as the next table row prints them
    Barrier barrier_strategy = Barrier::MONOTONE;  // always start monotone (:4427-4441)
  };
  struct IterRecord {  // what one major iteration decides and its table row / info column report
    bool rel_function_test = false;
    double max_prime = 0.0, max_dual = 0.0, max_infeas = 0.0, res_norm = 0.0, comp = 0.0, tau = 0.0;
    StepKind kind = StepKind::QUASI_NEWTON;
    int gmres_iters = 0;
    double alpha = 1.0, alpha_x = 1.0, alpha_z = 1.0;
    int ceq_step = 0, line_fail = 2 /* LS_FAILURE */, update_type = 0;
    bool monotone_barrier_converged = false, qn_hessian_reset = false, line_search_skipped = false;
    bool retried_after_reset = false;  // retryAfterReset ran: reported as a diagonal quasi-Newton step (:5130-5173)
  };
  bool mehrotra(const MajorState &st) const {
    return st.barrier_strategy == Barrier::MEHROTRA || st.barrier_strategy == Barrier::MPC;
  }
  int uploadLiveMirrors();
  int startRun(const RunOptions &opt);
  int iterationHead(const RunOptions &opt, int k, const char **checkpoint, IterRecord &it);
  void residualNorms(double mu, IterRecord &it);
  int updateBarrierAndNorms(const RunOptions &opt, int k, MajorState &st, IterRecord &it);
  void appendTableRow(int k, const MajorState &st, const IterRecord &it);
  bool stopTest(const RunOptions &opt, int k, const MajorState &st, const IterRecord &it);
  int newtonKrylovAttempt(const RunOptions &opt, const MajorState &st, IterRecord &it);
  int chooseStepKind(const RunOptions &opt, const MajorState &st, IterRecord &it);
  int computeStep(const RunOptions &opt, int k, const MajorState &st, IterRecord &it);
  void resetQuasiNewton(IterRecord &it);
  int meritDerivative(MajorState &st, const IterRecord &it, double *m0, double *dm0);
  int stepWithLineSearchSkipped(const RunOptions &opt, const MajorState &st, IterRecord &it);
  int retryAfterReset(MajorState &st, IterRecord &it, double *m0, double *dm0);
  int stepByLineSearch(const RunOptions &opt, MajorState &st, IterRecord &it, double m0, double dm0);
  int stepWithoutLineSearch(const RunOptions &opt, IterRecord &it, double m0, double dm0);
  void closeIteration(const RunOptions &opt, MajorState &st, IterRecord &it);
  void phaseBegin();
  void phaseEnd(const char *name);
  double phase_t0;
  // HIP-event time of the user's problem callbacks (evalObjCon / evalObjConGradient): reported as the phase
  // "user_eval", a SUBSET of the init / line_search / step_update phases that contain the calls
  static const int kUserRing = 16;
  hipEvent_t user_ev[2 * kUserRing];
  int user_pending = 0;
  bool user_events_ready = false;
  double user_seconds = 0.0;
  void userBegin();
  void userEnd();
  void userHarvest();
  // Kernel forms, fixed at construction by the test switches (SW_* in core.hpp, INTEGRATION.md "Diagnostics"); each
  // member is true on the default path and false only under its switch
  struct Forms {
    bool analytic_panel_dots;   // P^T px from the W-based algebra (false: re-measured with an mdot pass)
    bool fuse_merit;            // the refinement pass takes the merit / complementarity sums of the final step
    bool lean_step;             // ... and, in the plain quasi-Newton iteration, stores px only
    bool recompute_dt;          // the solve passes re-form Dinv / t in registers where the bound data allow
    bool recompute_first_step;  // the fused first pass stores no step: the refinement pass re-forms it
    bool recompute_rhs;         // ... and the refinement right-hand side is re-formed as well
    bool fuse_mult_update;      // the bound-multiplier update rides in the residual pass of the new point
  };
  static Forms readForms();
  const Forms forms = readForms();
  int check_flag = 0;  // OR of the bound-repair bits of every initAndCheckDesignAndBounds call (:4290-4344)
  // uniform lb / ub of this rank as the last initAndCheckDesignAndBounds found them (bounds() hands them to the
  // kernels); every other writer of lb / ub clears them
  int bounds_uni[2] = {0, 0};
  double bounds_val[2] = {0.0, 0.0};
};

}  // namespace po

struct po_ip_s {
  po::InteriorPoint *ip;
};
