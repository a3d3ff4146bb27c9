// The inexact Newton-Krylov step (use_hvec_product) for a problem that has NO evalHvecProduct: the Rosenbrock problem
// of examples/rosenbrock_amd.cpp -- f = sum (1-x_i)^2 + 100 (x_{i+1}-x_i^2)^2, c0 = 0.25 - sum x^2 >= 0,
// c1 = 10 + sum_{i even} x_i >= 0, -2 <= x <= 1, x0 = -1 -- written against the facade exactly as a user of the
// reference would write it, first derivatives only.  ParOptInteriorPoint::setHvecFiniteDifference lets the solver take
// its Hessian-vector products as differences of the Lagrangian's gradient: one evalObjCon + evalObjConGradient at
// x + h p per product (two with central=1), into vectors the solver owns.
//
// build: make -C examples newton_krylov_fd_amd ; run: ./examples/newton_krylov_fd_amd nvars=100 [central=1]
#include <stdlib.h>
#include <string.h>

#include "ParOptAMD.hpp"

class Rosenbrock : public ParOptProblem {
 public:
  Rosenbrock(po_ctx ctx, int n) : ParOptProblem(ctx) {
    setProblemSizes(n, 2, 0);
    setNumInequalities(2, 0);
  }
  void getVarsAndBounds(ParOptVec *xvec, ParOptVec *lbvec, ParOptVec *ubvec) {
    ParOptScalar *x, *lb, *ub;
    xvec->getArray(&x);
    lbvec->getArray(&lb);
    ubvec->getArray(&ub);
    for (int i = 0; i < nvars; i++) {
      x[i] = -1.0;
      lb[i] = -2.0;
      ub[i] = 1.0;
    }
  }
  int evalObjCon(ParOptVec *xvec, ParOptScalar *fobj, ParOptScalar *cons) {
    ParOptScalar *x;
    xvec->getArray(&x);
    double f = 0.0, c0 = 0.25, c1 = 10.0;
    for (int i = 0; i + 1 < nvars; i++) {
      const double r = x[i + 1] - x[i] * x[i];
      f += (1.0 - x[i]) * (1.0 - x[i]) + 100.0 * r * r;
    }
    for (int i = 0; i < nvars; i++) c0 -= x[i] * x[i];
    for (int i = 0; i < nvars; i += 2) c1 += x[i];
    *fobj = f;
    cons[0] = c0;
    cons[1] = c1;
    nevals++;
    return 0;
  }
  int evalObjConGradient(ParOptVec *xvec, ParOptVec *gvec, ParOptVec **Ac) {
    ParOptScalar *x, *g, *a0, *a1;
    xvec->getArray(&x);
    gvec->getArray(&g);
    Ac[0]->getArray(&a0);
    Ac[1]->getArray(&a1);
    for (int i = 0; i < nvars; i++) g[i] = 0.0;
    for (int i = 0; i + 1 < nvars; i++) {
      const double r = x[i + 1] - x[i] * x[i];
      g[i] += -2.0 * (1.0 - x[i]) - 400.0 * r * x[i];
      g[i + 1] += 200.0 * r;
    }
    for (int i = 0; i < nvars; i++) a0[i] = -2.0 * x[i];
    for (int i = 0; i < nvars; i++) a1[i] = (i % 2 == 0) ? 1.0 : 0.0;  // every entry: the vector may be scratch
    ngevals++;
    return 0;
  }
  // (no evalHvecProduct: the base class answers "not available")
  int nevals = 0, ngevals = 0;  // every call, the extra ones of the differenced products included
};

int main(int argc, char *argv[]) {
  int nvars = 100, central = 0, exact_only = 0;
  for (int k = 1; k < argc; k++) {
    sscanf(argv[k], "nvars=%d", &nvars);
    sscanf(argv[k], "central=%d", &central);
    sscanf(argv[k], "exact_only=%d", &exact_only);
  }
  po_ctx ctx = NULL;
  if (po_ctx_create(0, &ctx) != 0) {
    fprintf(stderr, "no MI355X available: %s\n", po_last_error());
    return 2;
  }
  Rosenbrock *rosen = new Rosenbrock(ctx, nvars);
  rosen->incref();
  ParOptOptions *options = new ParOptOptions();
  options->incref();
  ParOptInteriorPoint::addDefaultOptions(options);  // (an empty ParOptOptions knows no names: setOption would refuse)
  int bad = options->setOption("use_hvec_product", 1);
  bad |= options->setOption("gmres_subspace_size", 15);
  bad |= options->setOption("nk_switch_tol", 1e3);  // the Krylov step from the first iteration on
  bad |= options->setOption("max_gmres_rtol", 1.0);
  bad |= options->setOption("output_file", "");
  if (bad) {
    fprintf(stderr, "an option was not accepted\n");
    return 3;
  }
  ParOptInteriorPoint *opt = new ParOptInteriorPoint(rosen, options);
  opt->incref();
  // exact_only=1 leaves the default (PO_HVEC_EXACT): the run then ends with "evalHvecProduct failed or is not provided"
  if (!exact_only) opt->setHvecFiniteDifference(PO_HVEC_FD_WHEN_MISSING, central);
  int rc = opt->optimize();
  int niter, neval, ngeval, nhvec, products = 0, evaluations = 0;
  opt->getIterationCounters(&niter, &neval, &ngeval, &nhvec);
  opt->getHvecFiniteDifferenceCount(&products, &evaluations);
  ParOptVec *x;
  ParOptScalar *z;
  opt->getOptimizedPoint(&x, &z, NULL, NULL, NULL);
  ParOptScalar *xv;
  x->getArray(&xv);
  printf("{\"rc\": %d, \"niter\": %d, \"neval\": %d, \"ngeval\": %d, \"nhvec\": %d, \"fd_products\": %d, "
         "\"fd_evaluations\": %d, \"problem_evals\": %d, \"problem_gevals\": %d, \"z0\": %.17e, \"z1\": %.17e, \"x\": [",
         rc, niter, neval, ngeval, nhvec, products, evaluations, rosen->nevals, rosen->ngevals, z[0], z[1]);
  for (int i = 0; i < nvars; i++) printf("%s%.17e", i ? ", " : "", xv[i]);
  printf("]}\n");
  opt->decref();
  options->decref();
  rosen->decref();
  po_ctx_destroy(ctx);
  return rc;
}
