// A problem that brings its own solver for the sparse-constraint block: createQuasiDefMat() returns a user-written
// ParOptQuasiDefMat instead of one of the library's two.  The problem is the chain-constrained Rosenbrock function of
// sparse_rosenbrock_amd.cpp (cw_i = 1 - x_i^2 - x_{i+1}^2 >= 0); the solver is a DENSE one with HIP kernels of its
// own, compiled outside the library: it forms S = C + Aw D^-1 Aw^T from the CSR entries where the library keeps them
// (getSparseJacobianDataDevice), factors S = L L^T in one workgroup, and answers
//     apply:  yw = S^-1 (bw - Aw D^-1 bx),   yx = D^-1 (bx + Aw^T yw)
// on the context's stream, so no vector ever visits the host.  A dense S is only sensible for a few thousand sparse
// constraints; the point is the interface: a banded, arrow or Kronecker solver plugs in the same way.
//
// Cost seen by the solver object per KKT system: one factor, one three-argument apply per column of the panel
// [dense constraint gradients | quasi-Newton columns] and one four-argument apply per bordered solve.
//
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip -Iinclude examples/dense_quasidef_amd.cpp -Lparopt_amd
//        -lparopt_amd -Wl,-rpath,$PWD/paropt_amd -o examples/dense_quasidef_amd ; run: ./examples/dense_quasidef_amd nvars=100
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ParOptAMD.hpp"

namespace {

constexpr int kThreads = 256;

double *device_array(ParOptVec *v) {
  double *d = NULL;
  po_vec_get_device_array(v->handle(), &d);
  return d;
}

// S[i][j] = [i == j] C_i + sum over the entries (i, p), (j, q) with equal column of a_ip dinv[col] a_jq
__global__ void assemble_kernel(int w, const int *rowp, const int *cols, const double *a, const double *dinv,
                                const double *cdiag, double *S) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= w * w) return;
  const int i = idx / w, j = idx - i * w;
  double s = (i == j) ? cdiag[i] : 0.0;
  for (int p = rowp[i]; p < rowp[i + 1]; p++)
    for (int q = rowp[j]; q < rowp[j + 1]; q++)
      if (cols[p] == cols[q]) s += a[p] * dinv[cols[p]] * a[q];
  S[idx] = s;
}

// in-place Cholesky of the lower triangle, one workgroup; *fail = 1 + the first row with a non-positive pivot
__global__ void cholesky_kernel(int w, double *S, int *fail) {
  __shared__ double pivot;
  for (int k = 0; k < w; k++) {
    if (threadIdx.x == 0) {
      double p = S[k * w + k];
      if (!(p > 0.0)) {
        if (*fail == 0) *fail = k + 1;
        p = 1.0;
      }
      pivot = sqrt(p);
      S[k * w + k] = pivot;
    }
    __syncthreads();
    for (int i = k + 1 + threadIdx.x; i < w; i += blockDim.x) S[i * w + k] /= pivot;
    __syncthreads();
    const int m = w - k - 1;
    for (int t = threadIdx.x; t < m * m; t += blockDim.x) {
      const int i = k + 1 + t / m, j = k + 1 + t % m;
      if (j <= i) S[i * w + j] -= S[i * w + k] * S[j * w + k];
    }
    __syncthreads();
  }
}

// r_i = bw_i - sum_p a_ip dinv[col] bx[col]   (bw == NULL: zero block)
__global__ void rhs_kernel(int w, const int *rowp, const int *cols, const double *a, const double *dinv,
                           const double *bx, const double *bw, double *r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w) return;
  double s = bw ? bw[i] : 0.0;
  for (int p = rowp[i]; p < rowp[i + 1]; p++) s -= a[p] * dinv[cols[p]] * bx[cols[p]];
  r[i] = s;
}

// y <- L^-T L^-1 y, one workgroup (column-oriented substitutions)
__global__ void solve_kernel(int w, const double *L, double *y) {
  for (int k = 0; k < w; k++) {
    if (threadIdx.x == 0) y[k] /= L[k * w + k];
    __syncthreads();
    const double yk = y[k];
    for (int i = k + 1 + threadIdx.x; i < w; i += blockDim.x) y[i] -= L[i * w + k] * yk;
    __syncthreads();
  }
  for (int k = w - 1; k >= 0; k--) {
    if (threadIdx.x == 0) y[k] /= L[k * w + k];
    __syncthreads();
    const double yk = y[k];
    for (int i = threadIdx.x; i < k; i += blockDim.x) y[i] -= L[k * w + i] * yk;
    __syncthreads();
  }
}

__global__ void copy_kernel(int n, const double *src, double *dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// t[col] += a_ip yw_i over all entries
__global__ void transpose_add_kernel(int w, const int *rowp, const int *cols, const double *a, const double *yw,
                                     double *t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w) return;
  for (int p = rowp[i]; p < rowp[i + 1]; p++) atomicAdd(&t[cols[p]], a[p] * yw[i]);
}
__global__ void scale_kernel(int n, const double *dinv, double *y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] *= dinv[i];
}

int blocks(int n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

class DenseChainSolver : public ParOptQuasiDefMat {
 public:
  DenseChainSolver(ParOptSparseProblem *_prob, po_ctx ctx, int _n, int _w)
      : nfactor(0), napply3(0), napply4(0), prob(_prob), n(_n), w(_w), nnz(0), d_rowp(NULL), d_cols(NULL), d_a(NULL),
        d_S(NULL), d_fail(NULL), dinv(NULL) {
    stream = (hipStream_t)po_ctx_stream(ctx);
  }
  ~DenseChainSolver() {
    (void)hipStreamSynchronize(stream);
    (void)hipFree(d_rowp);
    (void)hipFree(d_cols);
    (void)hipFree(d_S);
    (void)hipFree(d_fail);
  }
  int factor(ParOptVec *, ParOptVec *Dinv, ParOptVec *Cdiag) {
    if (!d_S && !setup()) return 1;
    nfactor++;
    dinv = device_array(Dinv);  // borrowed until the next factor
    (void)hipMemsetAsync(d_fail, 0, sizeof(int), stream);
    assemble_kernel<<<blocks(w * w), kThreads, 0, stream>>>(w, d_rowp, d_cols, d_a, dinv, device_array(Cdiag), d_S);
    cholesky_kernel<<<1, kThreads, 0, stream>>>(w, d_S, d_fail);
    int fail = 0;
    (void)hipMemcpyAsync(&fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, stream);
    (void)hipStreamSynchronize(stream);
    return fail;
  }
  void apply(ParOptVec *bx, ParOptVec *yx, ParOptVec *yw) {
    napply3++;
    solve(bx, NULL, yx, yw);
  }
  void apply(ParOptVec *bx, ParOptVec *bw, ParOptVec *yx, ParOptVec *yw) {
    napply4++;
    solve(bx, bw, yx, yw);
  }
  const char *getFactorInfo() {
    info = "dense user solver: " + std::to_string(w) + " x " + std::to_string(w);
    return info.c_str();
  }
  long nfactor, napply3, napply4;

 private:
  bool setup() {
    const int *rowp = NULL, *cols = NULL;
    const ParOptScalar *a = NULL;
    nnz = prob->getSparseJacobianDataDevice(&rowp, &cols, &a);
    if (!rowp || !a) return false;
    d_a = a;
    if (hipMalloc((void **)&d_rowp, sizeof(int) * (w + 1)) != hipSuccess ||
        hipMalloc((void **)&d_cols, sizeof(int) * (nnz > 0 ? nnz : 1)) != hipSuccess ||
        hipMalloc((void **)&d_S, sizeof(double) * (size_t)w * w) != hipSuccess ||
        hipMalloc((void **)&d_fail, sizeof(int)) != hipSuccess)
      return false;
    (void)hipMemcpyAsync(d_rowp, rowp, sizeof(int) * (w + 1), hipMemcpyHostToDevice, stream);
    (void)hipMemcpyAsync(d_cols, cols, sizeof(int) * nnz, hipMemcpyHostToDevice, stream);
    (void)hipStreamSynchronize(stream);
    return true;
  }
  void solve(ParOptVec *bx, ParOptVec *bw, ParOptVec *yx, ParOptVec *yw) {
    const double *bxd = device_array(bx);
    double *yxd = device_array(yx), *ywd = device_array(yw);
    rhs_kernel<<<blocks(w), kThreads, 0, stream>>>(w, d_rowp, d_cols, d_a, dinv, bxd, bw ? device_array(bw) : NULL, ywd);
    solve_kernel<<<1, kThreads, 0, stream>>>(w, d_S, ywd);
    copy_kernel<<<blocks(n), kThreads, 0, stream>>>(n, bxd, yxd);
    transpose_add_kernel<<<blocks(w), kThreads, 0, stream>>>(w, d_rowp, d_cols, d_a, ywd, yxd);
    scale_kernel<<<blocks(n), kThreads, 0, stream>>>(n, dinv, yxd);
  }
  ParOptSparseProblem *prob;
  hipStream_t stream;
  int n, w, nnz;
  int *d_rowp, *d_cols;
  const double *d_a;  // the library's device array of Jacobian entries (borrowed)
  double *d_S;
  int *d_fail;
  const double *dinv;
  std::string info;
};

class ChainRosenbrock : public ParOptSparseProblem {
 public:
  ChainRosenbrock(po_ctx _ctx, int n) : ParOptSparseProblem(_ctx), solver(NULL) {
    setProblemSizes(n, 2, n - 1);
    setNumInequalities(2, n - 1);
    std::vector<int> rowp(n), cols(2 * (n - 1));
    for (int i = 0; i < n - 1; i++) {
      rowp[i] = 2 * i;
      cols[2 * i] = i;
      cols[2 * i + 1] = i + 1;
    }
    rowp[n - 1] = 2 * (n - 1);
    setSparseJacobianData(rowp.data(), cols.data());
  }
  // the problem's own solver instead of ParOptQuasiDefSparseMat (asked for once, owned by the solver that asks)
  ParOptQuasiDefMat *createQuasiDefMat() {
    solver = new DenseChainSolver(this, ctx, nvars, nwcon);
    return solver;
  }
  DenseChainSolver *solver;
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
  int evalSparseObjCon(ParOptVec *xvec, ParOptScalar *fobj, ParOptScalar *cons, ParOptVec *sparse) {
    ParOptScalar *x, *c;
    xvec->getArray(&x);
    sparse->getArray(&c);
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
    for (int i = 0; i < nwcon; i++) c[i] = 1.0 - x[i] * x[i] - x[i + 1] * x[i + 1];
    return 0;
  }
  int evalSparseObjConGradient(ParOptVec *xvec, ParOptVec *gvec, ParOptVec **Ac, ParOptScalar *data) {
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
    for (int i = 0; i < nvars; i += 2) a1[i] = 1.0;
    for (int i = 0; i < nwcon; i++) {
      data[2 * i] = -2.0 * x[i];
      data[2 * i + 1] = -2.0 * x[i + 1];
    }
    return 0;
  }
};

int main(int argc, char *argv[]) {
  int nvars = 100;
  for (int k = 1; k < argc; k++) sscanf(argv[k], "nvars=%d", &nvars);
  po_ctx ctx = NULL;
  if (po_ctx_create(0, &ctx) != 0) {
    fprintf(stderr, "no MI355X available: %s\n", po_last_error());
    return 2;
  }
  ChainRosenbrock *rosen = new ChainRosenbrock(ctx, nvars);
  rosen->incref();
  ParOptOptions *options = new ParOptOptions();
  options->incref();
  options->setOption("qn_type", "bfgs");
  options->setOption("qn_subspace_size", 10);
  options->setOption("abs_res_tol", 1e-6);
  options->setOption("barrier_strategy", "monotone");
  options->setOption("max_major_iters", 150);
  options->setOption("output_file", "");
  ParOptInteriorPoint *opt = new ParOptInteriorPoint(rosen, options);
  opt->incref();
  int rc = opt->optimize();
  int niter, neval, ngeval;
  opt->getIterationCounters(&niter, &neval, &ngeval);
  ParOptVec *x, *zw = NULL;
  ParOptScalar *z;
  opt->getOptimizedPoint(&x, &z, &zw, NULL, NULL);
  ParOptScalar fobj, cons[2];
  ParOptVec *cw = new ParOptBasicVec(ctx, nvars - 1);
  cw->incref();
  rosen->evalSparseObjCon(x, &fobj, cons, cw);
  const char *info = rosen->getFactorInfo();
  DenseChainSolver *s = rosen->solver;
  printf("{\"rc\": %d, \"niter\": %d, \"neval\": %d, \"ngeval\": %d, \"fobj\": %.15e, \"xnorm\": %.15e, "
         "\"z0\": %.15e, \"z1\": %.15e, \"zwnorm\": %.15e, \"factor_info\": \"%s\", \"nfactor\": %ld, \"napply3\": %ld, "
         "\"napply4\": %ld}\n", rc, niter, neval, ngeval, fobj, x->norm(), z[0], z[1], zw ? zw->norm() : 0.0,
         info ? info : "", s ? s->nfactor : 0L, s ? s->napply3 : 0L, s ? s->napply4 : 0L);
  cw->decref();
  opt->decref();
  options->decref();
  rosen->decref();
  po_ctx_destroy(ctx);
  return rc;
}
