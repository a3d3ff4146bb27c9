// A min-max problem in epigraph form on the facade: minimise the largest of the chain terms
//     f_i(x) = (x_i - a_i)^2 + (x_{i+1} - b_i)^2,   i < n - 1,
// as  min t  subject to  cw_i = t - f_i(x) >= 0  for every i, with t the last variable.  The epigraph variable enters
// EVERY sparse constraint: its column of the sparse Jacobian is dense and would fill the Schur complement
// S = C + Aw D^-1 Aw^T completely.  setDenseColumnThreshold() (or, from about 38 730 constraints on, the automatic
// rule) takes it out of the factored matrix -- what is left is the tridiagonal S0 of the chain -- and the solver puts it
// back by a low-rank update.  One dense constraint c0 = 10 + sum_{i even} x_i >= 0 as in sparse_rosenbrock_amd.cpp.
//
// build: make -C examples minmax_amd ; run: ./examples/minmax_amd nvars=200
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ParOptAMD.hpp"

class MinMax : public ParOptSparseProblem {
 public:
  MinMax(po_ctx ctx, int n_) : ParOptSparseProblem(ctx), n(n_) {
    setProblemSizes(n + 1, 1, n - 1);
    setNumInequalities(1, n - 1);
    std::vector<int> rowp(n), cols(3 * (n - 1));
    for (int i = 0; i < n - 1; i++) {
      rowp[i] = 3 * i;
      cols[3 * i] = i;
      cols[3 * i + 1] = i + 1;
      cols[3 * i + 2] = n;  // t
    }
    rowp[n - 1] = 3 * (n - 1);
    setDenseColumnThreshold((n - 1) / 2 > 3 ? (n - 1) / 2 : 3);  // before the pattern is handed over
    setSparseJacobianData(rowp.data(), cols.data());
  }
  static double a(int i) { return 0.5 * sin(1.0 + i); }
  static double b(int i) { return 0.5 * cos(1.0 + i); }
  double term(const ParOptScalar *x, int i) const {
    return (x[i] - a(i)) * (x[i] - a(i)) + (x[i + 1] - b(i)) * (x[i + 1] - b(i));
  }
  void getVarsAndBounds(ParOptVec *xvec, ParOptVec *lbvec, ParOptVec *ubvec) {
    ParOptScalar *x, *lb, *ub;
    xvec->getArray(&x);
    lbvec->getArray(&lb);
    ubvec->getArray(&ub);
    for (int i = 0; i < n; i++) {
      x[i] = 0.0;
      lb[i] = -2.0;
      ub[i] = 2.0;
    }
    x[n] = 1.0;
    lb[n] = 0.0;
    ub[n] = 20.0;
  }
  int evalSparseObjCon(ParOptVec *xvec, ParOptScalar *fobj, ParOptScalar *cons, ParOptVec *sparse) {
    ParOptScalar *x, *c;
    xvec->getArray(&x);
    sparse->getArray(&c);
    *fobj = x[n];
    double c0 = 10.0;
    for (int i = 0; i < n; i += 2) c0 += x[i];
    cons[0] = c0;
    for (int i = 0; i < nwcon; i++) c[i] = x[n] - term(x, i);
    return 0;
  }
  int evalSparseObjConGradient(ParOptVec *xvec, ParOptVec *gvec, ParOptVec **Ac, ParOptScalar *data) {
    ParOptScalar *x, *g, *a0;
    xvec->getArray(&x);
    gvec->getArray(&g);
    Ac[0]->getArray(&a0);
    for (int i = 0; i <= n; i++) {
      g[i] = 0.0;
      a0[i] = (i < n && i % 2 == 0) ? 1.0 : 0.0;
    }
    g[n] = 1.0;
    for (int i = 0; i < nwcon; i++) {
      data[3 * i] = -2.0 * (x[i] - a(i));
      data[3 * i + 1] = -2.0 * (x[i + 1] - b(i));
      data[3 * i + 2] = 1.0;
    }
    return 0;
  }
  int n;
};

int main(int argc, char *argv[]) {
  int nvars = 200;
  for (int k = 1; k < argc; k++) sscanf(argv[k], "nvars=%d", &nvars);
  if (nvars < 3) nvars = 3;
  po_ctx ctx = NULL;
  if (po_ctx_create(0, &ctx) != 0) {
    fprintf(stderr, "no MI355X available: %s\n", po_last_error());
    return 2;
  }
  MinMax *prob = new MinMax(ctx, nvars);
  prob->incref();
  ParOptOptions *options = new ParOptOptions();
  options->incref();
  ParOptInteriorPoint::addDefaultOptions(options);
  options->setOption("qn_type", "bfgs");
  options->setOption("qn_subspace_size", 10);
  options->setOption("abs_res_tol", 1e-6);
  options->setOption("barrier_strategy", "monotone");
  options->setOption("max_major_iters", 200);
  options->setOption("output_file", "");
  ParOptInteriorPoint *opt = new ParOptInteriorPoint(prob, options);
  opt->incref();
  int rc = opt->optimize();
  int niter, neval, ngeval;
  opt->getIterationCounters(&niter, &neval, &ngeval);
  ParOptVec *xvec, *zw = NULL;
  ParOptScalar *z, *x;
  opt->getOptimizedPoint(&xvec, &z, &zw, NULL, NULL);
  xvec->getArray(&x);
  double worst = 0.0;
  for (int i = 0; i + 1 < nvars; i++) worst = fmax(worst, prob->term(x, i));
  const int *dense = NULL;
  const int ndense = prob->getDenseColumns(&dense);
  const char *info = prob->getFactorInfo();
  printf("{\"rc\": %d, \"niter\": %d, \"neval\": %d, \"ngeval\": %d, \"t\": %.15e, \"max_term\": %.15e, "
         "\"ndense\": %d, \"dense_column\": %d, \"zwnorm\": %.15e, \"factor_info\": \"%s\"}\n", rc, niter, neval, ngeval,
         x[nvars], worst, ndense, ndense > 0 ? dense[0] : -1, zw ? zw->norm() : 0.0, info ? info : "");
  opt->decref();
  options->decref();
  prob->decref();
  po_ctx_destroy(ctx);
  return rc;
}
