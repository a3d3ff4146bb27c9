// A compact quasi-Newton approximation written by the USER: a limited-memory BFGS (both update types, both initial
// diagonals) as a subclass of ParOptCompactQuasiNewton, handed to ParOptInteriorPoint::setQuasiNewton.  Its pairs are
// ParOptVecs; its n-sized work runs in HIP kernels of its own, compiled outside the library and launched on the
// context's stream over po_vec_get_device_array pointers:
//
//   update:  ONE pass computes s^T [S | Y], s.s, s.y, y.y with s, y and every stored column read once, and writes s and
//            y into a spare pair slot on the way (k + 4 streams, k = 2 * pairs held).  An accepted pair enters by pointer
//            rotation; a skipped one leaves the spare slot spare, so the oldest pair survives a skip.  The curvature
//            test's s^T B s comes from the same dots (Z = [S | Y]).  Only the damped branch pays extra passes
//            (r = (1 - theta) B s + theta y into the spare slot, then r.r and r.s).
//   mult / multAdd:  one dot pass and one combination pass (2k + 3 streams), not k axpy calls.
//
// Reductions: per wave64 with shuffles, per workgroup through LDS in a fixed order, across workgroups by a second
// kernel in a fixed order -- no atomics, bit-reproducible for a fixed grid.  Across ranks the partial sums go through
// one po_ctx_allreduce.
//
// The library evaluates B through getCompactMat() alone: what a class behind the public interface
// cannot do is take Z^T s from the step's panel products or swap buffers with the solver, so per update it streams
// k + 4 doubles per variable where the built-in class streams 5.
//
// main() solves the workload of tests/golden/ip_quadratic_n1000_c8_bfgs20 and prints one JSON line.
// build: make -C examples user_quasi_newton_amd ; run: ./examples/user_quasi_newton_amd n=1000 c=8 m=20 iters=150
// -DUSER_QN_NO_MAIN -shared: extern "C" constructors, so that Python can attach the class to any problem.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ParOptAMD.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 4;       // 16-byte loads per lane and tile: one wave covers 64 * kTile pairs = 512 doubles
constexpr int kMaxCols = 64;   // 2 * (largest subspace)
constexpr int kExtra = 3;      // s.s, s.y, y.y behind the column dots

struct ColTable {
  const double *p[kMaxCols];
};
struct CoefTable {
  double a[kMaxCols];
};

double *device_array(ParOptVec *v) {
  double *d = NULL;
  po_vec_get_device_array(v->handle(), &d);
  return d;
}

__device__ inline double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// partials[block][0..k-1] = s . Z_j, and with kPair also [k] = s.s, [k+1] = s.y, [k+2] = y.y of the block's share, while
// s and y are copied to s_out / y_out (when given) from the registers that hold them.  n odd: the last 16-byte access
// reaches one element past the end (library vectors are allocated to an even count); that element is masked to zero.
template <bool kPair>
__global__ void __launch_bounds__(kThreads)
    panel_dots_kernel(const double *__restrict__ s, const double *__restrict__ y, ColTable Z, int k, long n,
                      double *__restrict__ s_out, double *__restrict__ y_out, double *__restrict__ partials) {
  __shared__ double acc[kWaves][kMaxCols + kExtra];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nout = k + (kPair ? kExtra : 0);
  for (int j = lane; j < nout; j += 64) acc[wave][j] = 0.0;
  __syncthreads();
  const long npairs = (n + 1) >> 1;
  const long ntiles = (npairs + 64 * kTile - 1) / (64 * kTile);
  for (long t = (long)blockIdx.x * kWaves + wave; t < ntiles; t += (long)gridDim.x * kWaves) {
    const long q0 = t * 64 * kTile + lane;
    double2 sv[kTile], yv[kTile];
    double ss = 0.0, sy = 0.0, yy = 0.0;
#pragma unroll
    for (int i = 0; i < kTile; i++) {
      const long q = q0 + (long)i * 64;
      sv[i] = make_double2(0.0, 0.0);
      yv[i] = make_double2(0.0, 0.0);
      if (q < npairs) {
        sv[i] = reinterpret_cast<const double2 *>(s)[q];
        if (2 * q + 1 >= n) sv[i].y = 0.0;
        if (kPair) {
          yv[i] = reinterpret_cast<const double2 *>(y)[q];
          if (2 * q + 1 >= n) yv[i].y = 0.0;
          if (s_out) {
            reinterpret_cast<double2 *>(s_out)[q] = sv[i];
            reinterpret_cast<double2 *>(y_out)[q] = yv[i];
          }
          ss += sv[i].x * sv[i].x + sv[i].y * sv[i].y;
          sy += sv[i].x * yv[i].x + sv[i].y * yv[i].y;
          yy += yv[i].x * yv[i].x + yv[i].y * yv[i].y;
        }
      }
    }
    for (int j = 0; j < k; j++) {
      const double2 *zp = reinterpret_cast<const double2 *>(Z.p[j]);
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < kTile; i++) {
        const long q = q0 + (long)i * 64;
        if (q < npairs) {
          const double2 z = zp[q];  // (a masked s kills whatever sits past the end)
          a += sv[i].x * z.x + sv[i].y * z.y;
        }
      }
      a = wave_sum(a);
      if (lane == 0) acc[wave][j] += a;
    }
    if (kPair) {
      ss = wave_sum(ss);
      sy = wave_sum(sy);
      yy = wave_sum(yy);
      if (lane == 0) {
        acc[wave][k] += ss;
        acc[wave][k + 1] += sy;
        acc[wave][k + 2] += yy;
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nout; j += kThreads)
    partials[(long)blockIdx.x * nout + j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
}

// out[j] = sum over the workgroups in a fixed order (one wave per value)
__global__ void __launch_bounds__(64)
    final_sum_kernel(const double *__restrict__ partials, int nblocks, int nout, double *__restrict__ out) {
  const int j = blockIdx.x;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) acc += partials[(long)b * nout + j];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[j] = acc;
}

// out <- a x + b out + sum_j c_j Z_j in one pass (b == 0: out is not read)
__global__ void __launch_bounds__(kThreads)
    combine_kernel(double *__restrict__ out, double a, const double *__restrict__ x, double b, ColTable Z, CoefTable c,
                   int k, long n) {
  const long npairs = (n + 1) >> 1;
  for (long q = (long)blockIdx.x * kThreads + threadIdx.x; q < npairs; q += (long)gridDim.x * kThreads) {
    const double2 xv = reinterpret_cast<const double2 *>(x)[q];
    double2 v = make_double2(a * xv.x, a * xv.y);
    if (b != 0.0) {
      const double2 o = reinterpret_cast<const double2 *>(out)[q];
      v.x += b * o.x;
      v.y += b * o.y;
    }
    for (int j = 0; j < k; j++) {
      const double2 z = reinterpret_cast<const double2 *>(Z.p[j])[q];
      v.x += c.a[j] * z.x;
      v.y += c.a[j] * z.y;
    }
    if (2 * q + 1 >= n) v.y = 0.0;
    reinterpret_cast<double2 *>(out)[q] = v;
  }
}

// x <- A^-1 x for a small dense column-major A (partial pivoting); A is overwritten
void dense_solve(int k, std::vector<double> &A, double *x) {
  for (int c = 0; c < k; c++) {
    int p = c;
    for (int i = c + 1; i < k; i++)
      if (fabs(A[i + (size_t)k * c]) > fabs(A[p + (size_t)k * c])) p = i;
    if (p != c) {
      for (int j = 0; j < k; j++) std::swap(A[c + (size_t)k * j], A[p + (size_t)k * j]);
      std::swap(x[c], x[p]);
    }
    const double piv = A[c + (size_t)k * c];
    for (int i = c + 1; i < k; i++) {
      const double f = A[i + (size_t)k * c] / piv;
      if (f == 0.0) continue;
      for (int j = c; j < k; j++) A[i + (size_t)k * j] -= f * A[c + (size_t)k * j];
      x[i] -= f * x[c];
    }
  }
  for (int c = k - 1; c >= 0; c--) {
    for (int j = c + 1; j < k; j++) x[c] -= A[c + (size_t)k * j] * x[j];
    x[c] /= A[c + (size_t)k * c];
  }
}

}  // namespace

class UserLBFGS : public ParOptCompactQuasiNewton {
 public:
  UserLBFGS(po_ctx _ctx, int _n, int _m, ParOptBFGSUpdateType _update_type = PAROPT_SKIP_NEGATIVE_CURVATURE)
      : ctx(_ctx), n(_n), m(_m > kMaxCols / 2 ? kMaxCols / 2 : _m), update_type(_update_type),
        diag_type(PAROPT_YTY_OVER_YTS), d_partials(NULL), d_out(NULL), h_out(NULL) {
    stream = static_cast<hipStream_t>(po_ctx_stream(ctx));
    for (int i = 0; i < m + 1; i++) {  // one slot more than pairs: the spare that the update pass writes into
      S.push_back(new ParOptBasicVec(ctx, n));
      Y.push_back(new ParOptBasicVec(ctx, n));
      S.back()->incref();
      Y.back()->incref();
    }
    const long npairs = ((long)n + 1) >> 1, ntiles = (npairs + 64 * kTile - 1) / (64 * kTile);
    long g = (ntiles + kWaves - 1) / kWaves;
    grid = (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
    (void)hipMalloc((void **)&d_partials, sizeof(double) * (size_t)grid * (kMaxCols + kExtra));
    (void)hipMalloc((void **)&d_out, sizeof(double) * (kMaxCols + kExtra));
    (void)hipHostMalloc((void **)&h_out, sizeof(double) * (kMaxCols + kExtra), hipHostMallocDefault);
    B.assign((size_t)m * m, 0.0);
    L.assign((size_t)m * m, 0.0);
    D.assign(m, 0.0);
    clear();
    for (int i = 0; i < 6; i++) calls[i] = 0;
  }
  ~UserLBFGS() {
    if (h) po_qn_destroy(h);
    h = NULL;
    (void)hipStreamSynchronize(stream);
    for (ParOptVec *v : S) v->decref();
    for (ParOptVec *v : Y) v->decref();
    (void)hipFree(d_partials);
    (void)hipFree(d_out);
    (void)hipHostFree(h_out);
  }
  void setBFGSUpdateType(ParOptBFGSUpdateType t) { update_type = t; }
  void setInitDiagonalType(ParOptQuasiNewtonDiagonalType t) { diag_type = t; }
  void reset() {
    calls[0]++;
    clear();
  }
  int update(ParOptVec *, const ParOptScalar *, ParOptVec *, ParOptVec *s, ParOptVec *y) {
    calls[1]++;
    const int k = 2 * msub;
    ParOptVec *ss = S[slot[msub]], *ys = Y[slot[msub]];  // the spare slot
    // one pass: s^T [S | Y], s.s, s.y, y.y, and (s, y) -> spare
    dots<true>(s, y, k, ss, ys);
    std::vector<double> dt(h_out, h_out + k + kExtra);
    const double sTs = dt[k], yTy0 = dt[k + 2];
    double yTs = dt[k + 1], yTy = yTy0;
    if (1e-8 * yTy >= fabs(yTs)) return 2;
    std::vector<double> coef(dt.begin(), dt.begin() + k);
    applyCompactInverse(coef.data());
    double sTBs = b0 * sTs;
    for (int i = 0; i < k; i++) sTBs -= dt[i] * coef[i];
    const bool sts = diag_type == PAROPT_YTS_OVER_STS;
    double b0_init;
    if (yTs >= 1e-12) {
      b0_init = sts ? yTs / sTs : yTy / yTs;
    } else {
      b0_init = 0.5 * (fabs(yTy / yTs) + fabs(yTs / sTs));
    }
    int rc = 0;
    if (yTs >= 0.01 * sTBs) {
      b0 = b0_init;
    } else if (update_type == PAROPT_SKIP_NEGATIVE_CURVATURE) {
      return 2;
    } else {  // damped: r = (1 - theta) B s + theta y replaces y in the spare slot (extra passes allowed here)
      rc = 1;
      const double theta = 0.8 * sTBs / (sTBs - yTs);
      CoefTable c;
      ColTable Zt = table(k);
      for (int i = 0; i < k; i++) c.a[i] = -(1.0 - theta) * coef[i];
      // spare y slot holds y already: r = (1 - theta) b0 s + theta * (spare) + sum c_j Z_j
      combine_kernel<<<cgrid(), kThreads, 0, stream>>>(device_array(ys), (1.0 - theta) * b0, device_array(s), theta, Zt, c,
                                                       k, (long)n);
      // r.s and r.r: the pair pass with (x, y) = (r, s) gives [.., r.r, r.s, s.s]
      ColTable none;
      none.p[0] = NULL;
      panel_dots_kernel<true><<<grid, kThreads, 0, stream>>>(device_array(ys), device_array(s), none, 0, (long)n, NULL,
                                                             NULL, d_partials);
      finish(kExtra);
      yTy = h_out[0];
      yTs = h_out[1];
      b0 = sts ? yTs / sTs : yTy / yTs;
    }
    store(dt.data(), dt.data() + msub, sTs, yTs);
    rebuild();
    return rc;
  }
  void mult(ParOptVec *x, ParOptVec *y) {
    calls[2]++;
    apply(1.0, x, 0.0, y);
  }
  void multAdd(ParOptScalar alpha, ParOptVec *x, ParOptVec *y) {
    calls[3]++;
    apply(alpha, x, 1.0, y);
  }
  int getCompactMat(ParOptScalar *_b0, const ParOptScalar **_d, const ParOptScalar **_M, ParOptVec ***_Z) {
    calls[4]++;
    if (_b0) *_b0 = b0;
    if (_d) *_d = d.data();
    if (_M) *_M = M.data();
    if (_Z) *_Z = Z.data();
    return (int)Z.size();
  }
  int getMaxLimitedMemorySize() {
    calls[5]++;
    return 2 * m;
  }
  long calls[6];  // reset, update, mult, multAdd, getCompactMat, getMaxLimitedMemorySize

 private:
  void clear() {
    msub = 0;
    b0 = 1.0;
    slot.resize(m + 1);
    for (int i = 0; i < m + 1; i++) slot[i] = i;  // slot[0..msub-1]: the pairs held, oldest first; slot[msub]: spare
    std::fill(B.begin(), B.end(), 0.0);
    std::fill(L.begin(), L.end(), 0.0);
    std::fill(D.begin(), D.end(), 0.0);
    M.clear();
    d.clear();
    Z.clear();
  }
  int cgrid() const {
    const long npairs = ((long)n + 1) >> 1;
    const long g = (npairs + kThreads - 1) / kThreads;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
  }
  ColTable table(int k) {
    ColTable t;
    for (int j = 0; j < k; j++) t.p[j] = device_array(Z[j]);
    return t;
  }
  // fixed-order sum over the workgroups, one host copy, one reduction over the ranks
  void finish(int nout) {
    final_sum_kernel<<<nout, 64, 0, stream>>>(d_partials, grid, nout, d_out);
    (void)hipMemcpyAsync(h_out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, stream);
    (void)hipStreamSynchronize(stream);
    po_ctx_allreduce(ctx, h_out, nout, 0);
  }
  template <bool kPair>
  void dots(ParOptVec *x, ParOptVec *y, int k, ParOptVec *xo, ParOptVec *yo) {
    ColTable t = table(k);
    panel_dots_kernel<kPair><<<grid, kThreads, 0, stream>>>(device_array(x), y ? device_array(y) : NULL, t, k, (long)n,
                                                            xo ? device_array(xo) : NULL, yo ? device_array(yo) : NULL,
                                                            d_partials);
    finish(k + (kPair ? kExtra : 0));
  }
  // rz <- d M^-1 d rz
  void applyCompactInverse(double *rz) {
    const int k = (int)Z.size();
    if (k == 0) return;
    for (int i = 0; i < k; i++) rz[i] *= d[i];
    std::vector<double> A(M);
    dense_solve(k, A, rz);
    for (int i = 0; i < k; i++) rz[i] *= d[i];
  }
  // y <- beta y + alpha B x: one dot pass, one combination pass
  void apply(double alpha, ParOptVec *x, double beta, ParOptVec *y) {
    const int k = (int)Z.size();
    CoefTable c;
    if (k > 0) {
      dots<false>(x, NULL, k, NULL, NULL);
      std::vector<double> rz(h_out, h_out + k);
      applyCompactInverse(rz.data());
      for (int i = 0; i < k; i++) c.a[i] = -alpha * rz[i];
    }
    combine_kernel<<<cgrid(), kThreads, 0, stream>>>(device_array(y), alpha * b0, device_array(x), beta, table(k), c, k,
                                                     (long)n);
  }
  // the spare slot becomes the newest pair (pointer rotation); sS / sY: dots of s with the pairs held before
  void store(const double *sS, const double *sY, double sTs, double sTy) {
    if (m == 0) return;
    int shift = 0;
    if (msub < m) {
      msub++;  // slot[msub - 1] was the spare; slot[msub] is the next one
    } else {
      shift = 1;
      const int oldest = slot[0];
      for (int i = 0; i < m; i++) slot[i] = slot[i + 1];
      slot[m] = oldest;  // the oldest pair's storage is the new spare
      for (int i = 0; i < m - 1; i++) D[i] = D[i + 1];
      for (int i = 0; i < m - 1; i++)
        for (int j = 0; j < m - 1; j++) B[i + (size_t)j * m] = B[i + 1 + (size_t)(j + 1) * m];
      for (int i = 0; i < m - 1; i++)
        for (int j = 0; j < i; j++) L[i + (size_t)j * m] = L[i + 1 + (size_t)(j + 1) * m];
    }
    const int k = msub;
    for (int i = 0; i < k - 1; i++) {
      B[(k - 1) + (size_t)i * m] = B[i + (size_t)(k - 1) * m] = sS[i + shift];
      L[(k - 1) + (size_t)i * m] = sY[i + shift];
    }
    B[(k - 1) + (size_t)(k - 1) * m] = sTs;
    D[k - 1] = sTy;
  }
  void rebuild() {
    const int k = msub;
    M.assign((size_t)4 * k * k, 0.0);
    for (int i = 0; i < k; i++)
      for (int j = 0; j < k; j++) M[i + (size_t)2 * k * j] = b0 * B[i + (size_t)m * j];
    for (int i = 0; i < k; i++)
      for (int j = 0; j < i; j++) M[i + (size_t)2 * k * (j + k)] = M[j + k + (size_t)2 * k * i] = L[i + (size_t)m * j];
    for (int i = 0; i < k; i++) M[k + i + (size_t)2 * k * (k + i)] = -D[i];
    d.assign(2 * k, 1.0);
    for (int i = 0; i < k; i++) d[i] = b0;
    Z.clear();
    for (int i = 0; i < k; i++) Z.push_back(S[slot[i]]);
    for (int i = 0; i < k; i++) Z.push_back(Y[slot[i]]);
  }

  po_ctx ctx;
  hipStream_t stream;
  int n, m, msub, grid;
  ParOptBFGSUpdateType update_type;
  ParOptQuasiNewtonDiagonalType diag_type;
  double b0;
  std::vector<ParOptVec *> S, Y, Z;
  std::vector<int> slot;
  std::vector<double> B, L, D, M, d;
  double *d_partials, *d_out, *h_out;
};

#ifdef USER_QN_NO_MAIN
// the class for Python (ctypes): an object, its po_qn handle (bound here), its call counts
extern "C" {
void *user_qn_create(po_ctx ctx, long n, int m, int damped, int yts_over_sts, po_qn *handle) {
  UserLBFGS *q = new UserLBFGS(ctx, (int)n, m, damped ? PAROPT_DAMPED_UPDATE : PAROPT_SKIP_NEGATIVE_CURVATURE);
  q->incref();
  q->setInitDiagonalType(yts_over_sts ? PAROPT_YTS_OVER_STS : PAROPT_YTY_OVER_YTS);
  if (handle) *handle = q->handle(ctx, (int)n);
  return q;
}
void user_qn_calls(void *obj, long out[6]) {
  for (int i = 0; i < 6; i++) out[i] = static_cast<UserLBFGS *>(obj)->calls[i];
}
void user_qn_destroy(void *obj) { static_cast<UserLBFGS *>(obj)->decref(); }
}
#else
#define CHECK(call)                                                        \
  do {                                                                     \
    if ((call) != 0) {                                                     \
      fprintf(stderr, "%s failed: %s\n", #call, po_last_error());          \
      return 1;                                                            \
    }                                                                      \
  } while (0)

// The golden's workload is the library's built-in separable quadratic, which the facade has no class for: the problem
// and the solver are made through the C ABI, the approximation is the C++ object above, bound by the facade.
int main(int argc, char *argv[]) {
  int n = 1000, c = 8, m = 20, iters = 150;
  for (int k = 1; k < argc; k++) {
    sscanf(argv[k], "n=%d", &n);
    sscanf(argv[k], "c=%d", &c);
    sscanf(argv[k], "m=%d", &m);
    sscanf(argv[k], "iters=%d", &iters);
  }
  po_ctx ctx = NULL;
  if (po_ctx_create(0, &ctx) != 0) {
    fprintf(stderr, "no MI355X available: %s\n", po_last_error());
    return 2;
  }
  po_problem prob = NULL;
  CHECK(po_problem_create_separable(ctx, PO_PROBLEM_QUADRATIC, n, c, 0, 1.0, 100.0, &prob));
  po_ip ip = NULL;
  CHECK(po_ip_create(prob, &ip));
  CHECK(po_ip_set_option_str(ip, "output_file", ""));
  CHECK(po_ip_set_option_str(ip, "qn_type", "bfgs"));
  CHECK(po_ip_set_option_int(ip, "qn_subspace_size", m));
  CHECK(po_ip_set_option_float(ip, "abs_res_tol", 1e-8));
  CHECK(po_ip_set_option_str(ip, "starting_point_strategy", "affine_step"));
  CHECK(po_ip_set_option_str(ip, "barrier_strategy", "monotone"));
  CHECK(po_ip_set_option_float(ip, "start_affine_multiplier_min", 0.01));
  CHECK(po_ip_set_option_float(ip, "penalty_gamma", 1000.0));
  CHECK(po_ip_set_option_int(ip, "max_major_iters", iters));
  UserLBFGS *qn = new UserLBFGS(ctx, n, m);
  qn->incref();
  CHECK(po_ip_set_quasi_newton(ip, qn->handle(ctx, n)));
  int rc = po_ip_optimize(ip, NULL);
  int niter = 0, neval = 0, ngeval = 0;
  double fobj = 0.0, rho = 0.0, xnorm = 0.0, check = -1.0;
  po_vec x = NULL;
  CHECK(po_ip_get_counters(ip, &niter, &neval, &ngeval));
  CHECK(po_ip_get_objective(ip, &fobj, &rho));
  CHECK(po_ip_get_optimized_point(ip, &x, NULL, NULL, NULL));
  CHECK(po_vec_norm(x, &xnorm));
  CHECK(po_qn_check_compact(qn->handle(), 0, &check));
  printf("{\"rc\": %d, \"niter\": %d, \"neval\": %d, \"ngeval\": %d, \"fobj\": %.15e, \"xnorm\": %.15e, "
         "\"check_compact\": %.3e, \"nreset\": %ld, \"nupdate\": %ld, \"nmult\": %ld, \"nmultadd\": %ld, "
         "\"ncompact\": %ld, \"nmaxsize\": %ld}\n",
         rc, niter, neval, ngeval, fobj, xnorm, check, qn->calls[0], qn->calls[1], qn->calls[2], qn->calls[3],
         qn->calls[4], qn->calls[5]);
  po_ip_destroy(ip);  // the solver first: it borrows the approximation
  qn->decref();
  po_problem_destroy(prob);
  po_ctx_destroy(ctx);
  return rc;
}
#endif
