// Device side of the multifrontal sparse Cholesky (sparse_chol.hpp): numeric factorization and solves, level by level,
// every front of a level in the same launches.  gfx950 only.
//
// Kernels per level of the factorization:
//   chol_assemble_kernel   a workgroup owns kCholChunk target columns of one front: zeroes the update-matrix part and
//                          gathers the children's update matrices through their relative indices, child after child
//                          (fixed order, no atomics: two entries of one child never share a target)
//   chol_small_kernel      front of order <= kCholSmall: one wavefront, the whole front in LDS, scalar fp64
//   per block column of kCholNB columns of the larger fronts (right-looking):
//   chol_diag_kernel       the diagonal block in LDS, one wavefront per front
//   chol_trsm_kernel       rows below it, kCholTile rows per workgroup, one row per lane, the block's triangle in LDS
//   chol_update_kernel     C -= A B^T on the rest of the front (panel columns and the b x b update matrix alike), one
//                          workgroup per 64 x 64 tile of the lower triangle, grid over (row tile of any front, column
//                          tile) through the level's running tile counts -- a large front spreads over the whole GPU
//   chol_pack_factor_kernel  the packed groups of the level (tiny fronts and their subtrees, SW_CHOL_PACK): a lane per
//                          group does what chol_assemble + chol_small do for each of its fronts, see "packed groups"
// Solves, level by level, a workgroup per front: chol_fwd / chol_bwd (solveDevice: its own permuted buffer, both
// sweeps) and chol_fwd_panel / chol_bwd_panel (sweep: the interior point's pointer-table panels, see there).  The packed
// groups of a level: chol_pack_fwd / chol_pack_bwd, a lane per group and right-hand side, both forms.
// Retained matrix (opt-in, see "retained matrix" below): chol_compact_kernel (the compact values at every set_values),
// chol_shift_kernel (the diagonal shift, into L only), chol_mat_rows / chol_mat_long (product, residual with column
// maxima, ||A||_inf), chol_colmax, chol_update_masked; the driver is SparseChol::solveRefinedDevice.
//
// Matrix instruction: v_mfma_f64_4x4x4_4b_f64 with the operand layout measured in wgram.hip (A lane = i + 4 b + 16 k,
// B lane = j + 4 b + 16 k, D lane = j + 4 b + 16 i).  It sustains 75.8 TFLOP/s against 47 for 16x16x4 (wgram.hip), the
// fp64 vector peak is the same as the matrix peak, so what it buys is operand reuse: per k-step of 4 a wavefront reads
// 2 + 8 operands from LDS for 16 instructions (a 32 x 32 block of the tile), where a vector kernel would read one
// operand pair per 1-4 fma.  The four blocks b are four row groups of the tile and the A operand (the column block) is
// the same in all four, so the 16 lanes of a result register hold 16 consecutive rows of one column: stores into the
// column-major front are 128-byte runs.
#include "sparse_chol.hpp"

#include <string.h>

namespace po {

namespace {

struct CholDev {
  const int *first, *nb, *ld, *uld;
  const int64_t *panel, *upd, *sol, *rows_ptr;
  const int *below, *rel, *child_ptr, *child;
  double *L, *arena;
};

constexpr int kLdsLd = kCholNB + 1;
constexpr int kOpLd = kCholTile + 16;  // operand tiles: == 16 mod 32 doubles, two k rows hit disjoint bank pairs

__device__ inline double *front_entry(double *P, int ld, double *U, int uld, int s, int row, int col) {
  return col < s ? P + (int64_t)col * ld + row : U + (int64_t)(col - s) * uld + (row - s);
}

__global__ void chol_scatter_kernel(const int *__restrict__ ptr, const int64_t *__restrict__ dst,
                                    const int *__restrict__ src, int64_t ndst, const double *__restrict__ vals,
                                    double *L) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndst) return;
  double sum = 0.0;
  for (int p = ptr[d]; p < ptr[d + 1]; p++) sum += vals[src[p]];
  L[dst[d]] = sum;
}

__global__ __launch_bounds__(128) void chol_assemble_kernel(CholDev d, const int *__restrict__ chunk_sn,
                                                            const int *__restrict__ chunk_c0) {
  const int J = chunk_sn[blockIdx.x], c0 = chunk_c0[blockIdx.x];
  const int s = d.first[J + 1] - d.first[J], b = d.nb[J], m = s + b;
  const int c1 = min(c0 + kCholChunk, m);
  const int ld = d.ld[J], uld = d.uld[J];
  double *P = d.L + d.panel[J], *U = d.arena + d.upd[J];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int z0 = max(c0, s);
  if (c1 > z0) {
    const int total = (c1 - z0) * b;
    for (int idx = tid; idx < total; idx += nt) {
      const int col = z0 + idx / b, row = s + idx % b;
      if (row >= col) U[(int64_t)(col - s) * uld + (row - s)] = 0.0;
    }
  }
  __syncthreads();
  for (int c = d.child_ptr[J]; c < d.child_ptr[J + 1]; c++) {
    const int C = d.child[c], bc = d.nb[C], ulc = d.uld[C];
    const int *__restrict__ rel = d.rel + d.rows_ptr[C];
    const double *__restrict__ Uc = d.arena + d.upd[C];
    int ja = 0, jb = 0;
    {  // rel ascends: the child's columns that land in [c0, c1)
      int lo = 0, hi = bc;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rel[mid] < c0) lo = mid + 1; else hi = mid;
      }
      ja = lo;
      hi = bc;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rel[mid] < c1) lo = mid + 1; else hi = mid;
      }
      jb = lo;
    }
    const int total = (jb - ja) * bc;
    for (int idx = tid; idx < total; idx += nt) {
      const int j = ja + idx / bc, i = idx % bc;
      if (i < j) continue;
      *front_entry(P, ld, U, uld, s, rel[i], rel[j]) += Uc[(int64_t)j * ulc + i];
    }
    __syncthreads();
  }
}

// The flag block, four ints: [0] a pivot was replaced, [1] the smallest permuted index of one, and from the signed
// forms only [2] negative pivots (chol_count_negative_kernel), [3] replaced pivots.  Integer atomics: whatever the
// order, the same block.
__device__ inline void flag_pivot(int *flag, int index) {
  flag[0] = 1;
  atomicMin(&flag[1], index);  // (the smallest index wins whatever the order: deterministic)
}

// SIGNED FORMS (kSigned, PO_CHOL_LDLT): P A P^T = L S L^T with S = diag(+-1) and a positive diagonal of L.  Column k:
// s_k = sign(piv), l_kk = sqrt|piv|, l_ik = a_ik / (s_k l_kk), a_ij -= l_ik (s_k l_jk).  In every kernel s_k sits on
// the COLUMN operand l_jk (here F[k][j], the triangle D of chol_trsm_kernel, Cs of chol_update_kernel, F[tri(j, k)]
// of the packed kernel), so with all signs + every form does the unsigned form's operations on the same values.
// A pivot that is zero or NaN is flagged and replaced by +1.  sgn[index0 + k] = s_k is written by the one thread that
// forms the pivot.  The unsigned instantiations are the code as it was, instruction for instruction: they do not
// count the pivots they replace (one more atomic on that never-taken path was measured at + 1.3 % on the
// factorization of the 300 x 300 grid, HISTORY.md R22).
__device__ inline double signed_pivot(double &piv, int *flag, int index, double *sgn, bool writer) {
  double sk = 1.0;
  if (!(piv > 0.0 || piv < 0.0)) {
    if (writer) {
      flag_pivot(flag, index);
      atomicAdd(&flag[3], 1);
    }
    piv = 1.0;
  } else if (piv < 0.0) {
    sk = -1.0;
    piv = -piv;
  }
  if (writer) sgn[index] = sk;
  return sk;
}

// The sign switch, once: the pivot of column `index` (tested, flagged and replaced by 1 where it cannot be used, its
// sign s_k returned -- 1 in the unsigned form), the divisor of the column below it and the column operand that
// carries s_k.  The unsigned forms multiply by nothing.
template <bool kSigned>
__device__ inline double form_pivot(double &piv, int *flag, int index, double *sgn, bool writer) {
  if (kSigned) return signed_pivot(piv, flag, index, sgn, writer);
  if (!(piv > 0.0)) {
    if (writer) flag_pivot(flag, index);
    piv = 1.0;
  }
  return 1.0;
}
template <bool kSigned>
__device__ inline double pivot_divisor(double sk, double r) { return kSigned ? sk * r : r; }
template <bool kSigned>
__device__ inline double column_operand(double sk, double v) { return kSigned ? sk * v : v; }

// Partial Cholesky of the first s columns of the m x m lower triangle F (column-major, kLdsLd) in LDS by ONE
// wavefront.  A non-positive (or NaN) pivot is flagged and replaced by 1, as chol_front_dense_kernel does.
template <bool kSigned>
__device__ inline void lds_partial_chol(double *F, int m, int s, int index0, int *flag, double *sgn) {
  const int tid = threadIdx.x, i = tid & 31, half = tid >> 5;
  for (int k = 0; k < s; k++) {
    double piv = F[k * kLdsLd + k];
    const double sk = form_pivot<kSigned>(piv, flag, index0 + k, sgn, tid == 0);
    const double r = sqrt(piv);
    __syncthreads();
    if (tid == 0) F[k * kLdsLd + k] = r;
    if (half == 0 && i > k && i < m) F[k * kLdsLd + i] /= pivot_divisor<kSigned>(sk, r);
    __syncthreads();
    if (i > k && i < m) {
      const double lik = F[k * kLdsLd + i];
      for (int j = k + 1 + half; j <= i; j += 2)
        F[j * kLdsLd + i] -= lik * column_operand<kSigned>(sk, F[k * kLdsLd + j]);
    }
    __syncthreads();
  }
}

template <bool kSigned>
__global__ __launch_bounds__(64) void chol_small_kernel(CholDev d, const int *__restrict__ list, int *flag,
                                                        double *sgn) {
  __shared__ double F[kCholSmall * kLdsLd];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, b = d.nb[J], m = s + b;
  const int ld = d.ld[J], uld = d.uld[J];
  double *P = d.L + d.panel[J], *U = d.arena + d.upd[J];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < m * m; idx += 64) {
    const int col = idx / m, row = idx % m;
    if (row >= col) F[col * kLdsLd + row] = *front_entry(P, ld, U, uld, s, row, col);
  }
  __syncthreads();
  lds_partial_chol<kSigned>(F, m, s, first, flag, sgn);
  for (int idx = tid; idx < m * m; idx += 64) {
    const int col = idx / m, row = idx % m;
    if (row >= col) *front_entry(P, ld, U, uld, s, row, col) = F[col * kLdsLd + row];
  }
}

template <bool kSigned>
__global__ __launch_bounds__(64) void chol_diag_kernel(CholDev d, const int *__restrict__ list, int kb, int *flag,
                                                       double *sgn) {
  __shared__ double F[kCholNB * kLdsLd];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, ld = d.ld[J];
  const int k0 = kb * kCholNB, w = min(kCholNB, s - k0);
  double *P = d.L + d.panel[J] + (int64_t)k0 * ld + k0;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < w * w; idx += 64) {
    const int col = idx / w, row = idx % w;
    if (row >= col) F[col * kLdsLd + row] = P[(int64_t)col * ld + row];
  }
  __syncthreads();
  lds_partial_chol<kSigned>(F, w, w, first + k0, flag, sgn);
  for (int idx = tid; idx < w * w; idx += 64) {
    const int col = idx / w, row = idx % w;
    if (row >= col) P[(int64_t)col * ld + row] = F[col * kLdsLd + row];
  }
}

// which active front does row tile t belong to: tab[a] <= t < tab[a + 1]
__device__ inline int tile_front(const int *__restrict__ tab, int nact, int t) {
  int lo = 0, hi = nact;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// kSigned: the rows solve against S L11^T -- column k of the triangle in LDS is s_k times that of L11, the diagonal
// included, and the substitution below is the unsigned one.
template <bool kSigned>
__global__ __launch_bounds__(kCholTile) void chol_trsm_kernel(CholDev d, const int *__restrict__ list,
                                                              const int *__restrict__ tab, int nact, int kb,
                                                              const double *__restrict__ sgn) {
  __shared__ double D[kCholNB * kLdsLd], X[kCholTile * kLdsLd];
  const int t = blockIdx.x, a = tile_front(tab, nact, t), J = list[a];
  const int s = d.first[J + 1] - d.first[J], m = s + d.nb[J], ld = d.ld[J];
  const int k0 = kb * kCholNB, w = min(kCholNB, s - k0);
  double *P = d.L + d.panel[J] + (int64_t)k0 * ld;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kCholNB * kCholNB; idx += kCholTile) {
    const int col = idx / kCholNB, row = idx % kCholNB;
    double v = row == col ? 1.0 : 0.0;  // (identity outside a partial block)
    if (col < w && row < w && row >= col) {
      v = P[(int64_t)col * ld + k0 + row];
      if (kSigned) v *= sgn[d.first[J] + k0 + col];
    }
    D[col * kLdsLd + row] = v;
  }
  __syncthreads();
  const int row = k0 + w + (t - tab[a]) * kCholTile + tid;
  if (row >= m) return;
  // the lane's row lives in LDS (stride 33: no bank conflicts), so the loops need no unrolling and no registers
  double *x = X + tid * kLdsLd;
  for (int k = 0; k < w; k++) x[k] = P[(int64_t)k * ld + row];
  for (int k = 0; k < w; k++) {
    const double xk = x[k] / D[k * kLdsLd + k];
    P[(int64_t)k * ld + row] = xk;
    for (int j = k + 1; j < w; j++) x[j] -= xk * D[k * kLdsLd + j];
  }
}

// kSigned: C -= A S B^T, the signs multiply the column operand Cs as it is loaded.
template <bool kSigned>
__global__ __launch_bounds__(256) void chol_update_kernel(CholDev d, const int *__restrict__ list,
                                                          const int *__restrict__ tab, int nact, int kb,
                                                          const double *__restrict__ sgn) {
  __shared__ double Rs[kCholNB * kOpLd], Cs[kCholNB * kOpLd];
  const int t = blockIdx.x, a = tile_front(tab, nact, t);
  const int ti = t - tab[a], tj = blockIdx.y;
  if (tj > ti) return;
  const int J = list[a];
  const int s = d.first[J + 1] - d.first[J], m = s + d.nb[J], ld = d.ld[J], uld = d.uld[J];
  const int k0 = kb * kCholNB, w = min(kCholNB, s - k0), r0 = k0 + w;
  double *P = d.L + d.panel[J], *U = d.arena + d.upd[J];
  const double *__restrict__ Pk = P + (int64_t)k0 * ld;
  const int R0 = r0 + ti * kCholTile, C0 = r0 + tj * kCholTile;
  const int tid = threadIdx.x;
  {
    const int row = tid & 63, kq = tid >> 6;
#pragma unroll
    for (int it = 0; it < kCholNB / 4; it++) {
      const int kk = kq + 4 * it;
      const bool live = kk < w;
      Rs[kk * kOpLd + row] = (live && R0 + row < m) ? Pk[(int64_t)kk * ld + R0 + row] : 0.0;
      double cv = (live && C0 + row < m) ? Pk[(int64_t)kk * ld + C0 + row] : 0.0;
      if (kSigned && live) cv *= sgn[d.first[J] + k0 + kk];
      Cs[kk * kOpLd + row] = cv;
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, wr = wave & 1, wc = wave >> 1;
  if (ti == tj && wr < wc) return;  // this quarter lies above the diagonal
  double acc[2][8];
#pragma unroll
  for (int rb = 0; rb < 2; rb++) {
#pragma unroll
    for (int cb = 0; cb < 8; cb++) acc[rb][cb] = 0.0;
  }
  const int ksteps = (w + 3) / 4;
  for (int kk = 0; kk < ksteps; kk++) {
    const int k = kk * 4 + (lane >> 4);
    double bop[2], aop[8];
#pragma unroll
    for (int rb = 0; rb < 2; rb++) bop[rb] = Rs[k * kOpLd + wr * 32 + rb * 16 + (lane & 15)];
#pragma unroll
    for (int cb = 0; cb < 8; cb++) aop[cb] = Cs[k * kOpLd + wc * 32 + cb * 4 + (lane & 3)];
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
#pragma unroll
      for (int cb = 0; cb < 8; cb++)
        acc[rb][cb] = __builtin_amdgcn_mfma_f64_4x4x4f64(aop[cb], bop[rb], acc[rb][cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int rb = 0; rb < 2; rb++) {
    const int row = R0 + wr * 32 + rb * 16 + (lane & 15);
#pragma unroll
    for (int cb = 0; cb < 8; cb++) {
      const int col = C0 + wc * 32 + cb * 4 + (lane >> 4);
      if (row < m && col < m && row >= col) *front_entry(P, ld, U, uld, s, row, col) -= acc[rb][cb];
    }
  }
}

// ---- packed groups (sparse_chol.hpp: CholSymbolic::grp_*) ----------------------------------------------------------
// A front of order <= kCholTiny holds a few lanes' worth of arithmetic, and the bottom levels of every elimination tree
// are made of them.  ONE LANE runs a whole group of such fronts -- a subtree in postorder -- so a level costs one
// launch of one thread per group (factorization) or per (group, right-hand side) (sweeps) instead of a workgroup per
// front, and a chain of one-column fronts inside a group costs no launch at all.  No barriers and nothing shared
// between lanes: a lane past the end of the list simply leaves.
// For every front these kernels do the floating-point operations of chol_assemble_kernel + chol_small_kernel, of
// chol_fwd / chol_bwd and of chol_fwd_panel / chol_bwd_panel in the same order, so L and every solve are bit for bit
// what the unpacked kernels give.  Contraction is therefore OFF in them and every fused multiply-add of the unpacked
// kernels is written out (__fma_rn); where those reduce over lanes (the backward sum) the same tree is spelled out.
// A lane's working set is addressed through rel / below, so it lives in a slot of LDS (odd stride in doubles), never
// in a private array.
constexpr int kPackLanes = 64;
constexpr int kPackB = kCholTiny - 1;                      // rows below the columns of a tiny front at most
// A CHILD of a tiny front may carry more: its rows below are rows of the parent's front, up to all kCholTiny of them
// (such a child has order > kCholTiny and is never packed itself, its tiny parent is then a group of one).
constexpr int kPackChildB = kCholTiny;
constexpr int kPackTri = kCholTiny * (kCholTiny + 1) / 2;  // entries of the lane's triangle
constexpr int kPackFactorSlot = kPackTri + 1;              // 37 doubles
constexpr int kPackSweepSlot = kPackTri + 2 * kCholTiny + 1;  // triangle, block of the vector, update vector: 53

// What a lane needs of a front, loaded one front ahead: the loads of the next front are in flight while the current
// one is worked on (a lane's fronts are a chain of dependent global loads otherwise).
struct PackFront {
  int first, s, b, ld, uld, c0, c1;
  int64_t panel, rows_ptr, off;  // off: the update matrix (factorization) or the update vector (sweeps)
};
__device__ inline PackFront pack_front(const CholDev &d, int J, bool sweep) {
  PackFront f;
  f.first = d.first[J];
  f.s = d.first[J + 1] - f.first;
  f.b = d.nb[J];
  f.ld = d.ld[J];
  f.uld = d.uld[J];
  f.c0 = d.child_ptr[J];
  f.c1 = d.child_ptr[J + 1];
  f.panel = d.panel[J];
  f.rows_ptr = d.rows_ptr[J];
  f.off = sweep ? d.sol[J] : d.upd[J];
  return f;
}

// entry (row, col), row >= col, of the packed lower triangle of order <= kCholTiny (column after column)
__device__ inline int tri(int row, int col) { return col * kCholTiny - col * (col - 1) / 2 + row - col; }

// The s panel columns of a front into the lane's triangle.  Global loads are issued a whole column (a whole vector,
// a whole child, ...) at a time into registers with constant indices and only then used: a load per loop iteration
// would make a lane wait out the memory latency entry by entry.
__device__ inline void pack_load_panel(double *F, const double *P, int ld, int s, int m) {
  for (int col = 0; col < s; col++) {
    const double *pc = P + (int64_t)col * ld + col;
    const int len = m - col, base = tri(col, col);
    double v[kCholTiny];
#pragma unroll
    for (int i = 0; i < kCholTiny; i++) v[i] = i < len ? pc[i] : 0.0;
#pragma unroll
    for (int i = 0; i < kCholTiny; i++) {
      if (i < len) F[base + i] = v[i];
    }
  }
}

template <bool kSigned>
__global__ __launch_bounds__(kPackLanes) void chol_pack_factor_kernel(CholDev d, const int *__restrict__ gfirst,
                                                                      const int *__restrict__ groot, int ngroup,
                                                                      int *flag, double *sgn) {
#pragma clang fp contract(off)
  __shared__ double Fs[kPackLanes * kPackFactorSlot];
  const int g = blockIdx.x * kPackLanes + threadIdx.x;
  if (g >= ngroup) return;
  double *F = Fs + threadIdx.x * kPackFactorSlot;
  const int root = groot[g];
  PackFront next = pack_front(d, gfirst[g], false);
  for (int J = gfirst[g]; J <= root; J++) {
    const PackFront f = next;
    if (J < root) next = pack_front(d, J + 1, false);
    const int first = f.first, s = f.s, b = f.b, m = s + b;
    const int ld = f.ld, uld = f.uld;
    double *P = d.L + f.panel, *U = d.arena + f.off;
    pack_load_panel(F, P, ld, s, m);
    for (int col = s; col < m; col++) {
      for (int row = col; row < m; row++) F[tri(row, col)] = 0.0;
    }
    for (int c = f.c0; c < f.c1; c++) {
      const int C = d.child[c], bc = d.nb[C], ulc = d.uld[C];
      const int *__restrict__ rel = d.rel + d.rows_ptr[C];
      const double *Uc = d.arena + d.upd[C];
      int rl[kPackChildB];
#pragma unroll
      for (int i = 0; i < kPackChildB; i++) rl[i] = i < bc ? rel[i] : 0;
#pragma unroll
      for (int j = 0; j < kPackChildB; j++) {
        if (j < bc) {
          double v[kPackChildB];
#pragma unroll
          for (int i = j; i < kPackChildB; i++) v[i] = i < bc ? Uc[(int64_t)j * ulc + i] : 0.0;
#pragma unroll
          for (int i = j; i < kPackChildB; i++) {
            if (i < bc) F[tri(rl[i], rl[j])] += v[i];
          }
        }
      }
    }
    for (int k = 0; k < s; k++) {
      double piv = F[tri(k, k)];
      const double sk = form_pivot<kSigned>(piv, flag, first + k, sgn, true);
      const double r = sqrt(piv);
      F[tri(k, k)] = r;
      for (int i = k + 1; i < m; i++) F[tri(i, k)] /= pivot_divisor<kSigned>(sk, r);
      for (int i = k + 1; i < m; i++) {
        const double lik = F[tri(i, k)];
        for (int j = k + 1; j <= i; j++)
          F[tri(i, j)] = __fma_rn(-lik, column_operand<kSigned>(sk, F[tri(j, k)]), F[tri(i, j)]);
      }
    }
    for (int col = 0; col < m; col++) {
      for (int row = col; row < m; row++) *front_entry(P, ld, U, uld, s, row, col) = F[tri(row, col)];
    }
  }
}

struct CholPtrs {
  double *p[kCholMaxRhs];
};

// kPanel: the right-hand sides of sweep() (a pointer table, reciprocal pivots, column-oriented substitution as in
// chol_fwd_panel / chol_bwd_panel); otherwise those of solveDevice (Yb, ldy; row-oriented with a division as in
// chol_fwd / chol_bwd).  Thread = (group, right-hand side), the right-hand side fastest: the lanes of a group load the
// same front data and the same entries of L -- one request a wavefront -- and each walks its own vector, whose
// neighbouring entries the group's next fronts use.  (The group index fastest was measured first: with 21 right-hand
// sides every lane then fetches the front data and L for itself, and the chain's Gram panel was slower than unpacked.)
template <bool kPanel>
__global__ __launch_bounds__(kPackLanes) void chol_pack_fwd_kernel(CholDev d, const int *__restrict__ gfirst,
                                                                   const int *__restrict__ groot, int ngroup,
                                                                   CholPtrs Yp, double *Yb, int64_t ldy, int nrhs) {
#pragma clang fp contract(off)
  __shared__ double slots[kPackLanes * kPackSweepSlot];
  const int64_t t = (int64_t)blockIdx.x * kPackLanes + threadIdx.x;
  if (t >= (int64_t)ngroup * nrhs) return;
  const int g = (int)(t / nrhs), r = (int)(t % nrhs);
  double *F = slots + threadIdx.x * kPackSweepSlot, *yl = F + kPackTri, *ul = yl + kCholTiny;
  double *Y = kPanel ? Yp.p[r] : Yb + r * ldy;
  const int root = groot[g];
  PackFront next = pack_front(d, gfirst[g], true);
  for (int J = gfirst[g]; J <= root; J++) {
    const PackFront f = next;
    if (J < root) next = pack_front(d, J + 1, true);
    const int first = f.first, s = f.s, b = f.b, m = s + b;
    double *u = d.arena + f.off + (int64_t)r * f.uld;
    pack_load_panel(F, d.L + f.panel, f.ld, s, m);
    {
      double v[kCholTiny];
#pragma unroll
      for (int k = 0; k < kCholTiny; k++) v[k] = k < s ? Y[first + k] : 0.0;
#pragma unroll
      for (int k = 0; k < kCholTiny; k++) yl[k] = v[k];
    }
    for (int i = 0; i < b; i++) ul[i] = 0.0;
    for (int c = f.c0; c < f.c1; c++) {
      const int C = d.child[c], bc = d.nb[C];
      const int *__restrict__ rel = d.rel + d.rows_ptr[C];
      const double *uc = d.arena + d.sol[C] + (int64_t)r * d.uld[C];
      int rl[kPackChildB];
      double v[kPackChildB];
#pragma unroll
      for (int i = 0; i < kPackChildB; i++) {
        rl[i] = i < bc ? rel[i] : 0;
        v[i] = i < bc ? uc[i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < kPackChildB; i++) {
        if (i < bc) {
          if (rl[i] < s) {
            yl[rl[i]] += v[i];
          } else {
            ul[rl[i] - s] += v[i];
          }
        }
      }
    }
    if (kPanel) {
      for (int j = 0; j < s; j++) {
        const double yj = yl[j] * (1.0 / F[tri(j, j)]);
        yl[j] = yj;
        for (int i = j + 1; i < s; i++) yl[i] = __fma_rn(-F[tri(i, j)], yj, yl[i]);
      }
    } else {
      for (int j = 0; j < s; j++) {
        double acc = yl[j];
        for (int k = 0; k < j; k++) acc = __fma_rn(-F[tri(j, k)], yl[k], acc);
        yl[j] = acc / F[tri(j, j)];
      }
    }
    for (int k = 0; k < s; k++) Y[first + k] = yl[k];
    for (int i = s; i < m; i++) {
      double acc = 0.0;
      for (int k = 0; k < s; k++) acc = __fma_rn(F[tri(i, k)], yl[k], acc);
      u[i - s] = ul[i - s] - acc;
    }
  }
}

template <bool kPanel>
__global__ __launch_bounds__(kPackLanes) void chol_pack_bwd_kernel(CholDev d, const int *__restrict__ gfirst,
                                                                   const int *__restrict__ groot, int ngroup,
                                                                   CholPtrs Yp, double *Yb, int64_t ldy, int nrhs) {
#pragma clang fp contract(off)
  __shared__ double slots[kPackLanes * kPackSweepSlot];
  const int64_t t = (int64_t)blockIdx.x * kPackLanes + threadIdx.x;
  if (t >= (int64_t)ngroup * nrhs) return;
  const int g = (int)(t / nrhs), r = (int)(t % nrhs);
  double *F = slots + threadIdx.x * kPackSweepSlot, *z = F + kPackTri;
  double *Y = kPanel ? Yp.p[r] : Yb + r * ldy;
  const int gf = gfirst[g];
  PackFront next = pack_front(d, groot[g], true);
  for (int J = groot[g]; J >= gf; J--) {
    const PackFront f = next;
    if (J > gf) next = pack_front(d, J - 1, true);
    const int first = f.first, s = f.s, b = f.b, m = s + b;
    const int *__restrict__ rows = d.below + f.rows_ptr;
    pack_load_panel(F, d.L + f.panel, f.ld, s, m);
    double x[kPackB];  // the solution at the rows below: ancestors, finished by this lane or by an earlier launch
    {
      int rw[kPackB];
      double v[kCholTiny];
#pragma unroll
      for (int i = 0; i < kPackB; i++) rw[i] = i < b ? rows[i] : 0;
#pragma unroll
      for (int i = 0; i < kPackB; i++) x[i] = i < b ? Y[rw[i]] : 0.0;
#pragma unroll
      for (int k = 0; k < kCholTiny; k++) v[k] = k < s ? Y[first + k] : 0.0;
#pragma unroll
      for (int k = 0; k < kCholTiny; k++) z[k] = v[k];
    }
    for (int k = 0; k < s; k++) {
      // The unpacked kernels give lane i the product of below-row i (added to 0.0) and reduce by a __shfl_xor
      // butterfly, offsets 32 .. 1, in which the lanes past the rows hold 0.0: lane 0 ends with this tree.
      double q[kCholTiny];
#pragma unroll
      for (int i = 0; i < kPackB; i++) q[i] = i < b ? __fma_rn(F[tri(s + i, k)], x[i], 0.0) + 0.0 : 0.0;
      q[kPackB] = 0.0;
      const double sum = ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7]));
      z[k] = z[k] - sum;
    }
    if (kPanel) {
      for (int j = s - 1; j >= 0; j--) {
        const double xj = z[j] * (1.0 / F[tri(j, j)]);
        z[j] = xj;
        for (int i = 0; i < j; i++) z[i] = __fma_rn(-F[tri(j, i)], xj, z[i]);
      }
    } else {
      for (int k = s - 1; k >= 0; k--) {
        double acc = z[k];
        for (int j = k + 1; j < s; j++) acc = __fma_rn(-F[tri(j, k)], z[j], acc);
        z[k] = acc / F[tri(k, k)];
      }
    }
    for (int k = 0; k < s; k++) Y[first + k] = z[k];
  }
}

// ---- solves ------------------------------------------------------------------------------------------------------
__global__ void chol_permute_kernel(double *Y, int64_t ldy, double *x, int64_t ldx, const int *__restrict__ perm,
                                    int n, int nrhs, int out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * nrhs) return;
  const int p = (int)(idx % n), r = (int)(idx / n);
  if (out) {
    x[perm[p] + r * ldx] = Y[p + r * ldy];
  } else {
    Y[p + r * ldy] = x[perm[p] + r * ldx];
  }
}

// The negative pivots of a signed factorization, from its signs: one atomic a workgroup.  (An atomic a pivot, from
// the thread that forms it, was measured first: half a million of them on one address cost the tridiagonal matrix
// of a million unknowns 5 ms, three times its factorization.)
__global__ __launch_bounds__(256) void chol_count_negative_kernel(const double *__restrict__ sgn, int n, int *flag) {
  __shared__ int part[4];
  int count = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    count += sgn[i] < 0.0 ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = part[0] + part[1] + part[2] + part[3];
    if (total > 0) atomicAdd(&flag[2], total);
  }
}

// y_k <- s_k y_k between the forward and the backward sweep of a signed factorization (L S L^T x = b)
__global__ void chol_sign_kernel(double *Y, int64_t ldy, const double *__restrict__ sgn, int n, int nrhs) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * nrhs) return;
  const int p = (int)(idx % n), r = (int)(idx / n);
  Y[p + r * ldy] *= sgn[p];
}

__device__ inline void load_triangle(double *D, const double *P, int ld, int w) {
  for (int idx = threadIdx.x; idx < w * w; idx += blockDim.x) {
    const int col = idx / w, row = idx % w;
    if (row >= col) D[col * kLdsLd + row] = P[(int64_t)col * ld + row];
  }
}

// Forward: the front's block = its rows of the right-hand side plus the children's update vectors (fixed order),
// y_J = L11^-1 (.), and the update vector u = (children's part below) - L21 y_J for the parent.
__global__ __launch_bounds__(256) void chol_fwd_kernel(CholDev d, const int *__restrict__ list, double *Y, int64_t ldy,
                                                       int nrhs) {
  __shared__ double D[kCholNB * kLdsLd], yb[kCholNB * kCholMaxRhs];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, b = d.nb[J], m = s + b;
  const int ld = d.ld[J], ul = d.uld[J];
  const double *__restrict__ P = d.L + d.panel[J];
  double *u = d.arena + d.sol[J];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < b * nrhs; idx += 256) u[idx % b + (int64_t)(idx / b) * ul] = 0.0;
  __syncthreads();
  for (int c = d.child_ptr[J]; c < d.child_ptr[J + 1]; c++) {
    const int C = d.child[c], bc = d.nb[C], ulc = d.uld[C];
    const int *__restrict__ rel = d.rel + d.rows_ptr[C];
    const double *__restrict__ uc = d.arena + d.sol[C];
    for (int idx = tid; idx < bc * nrhs; idx += 256) {
      const int i = idx % bc, r = idx / bc, t = rel[i];
      const double v = uc[i + (int64_t)r * ulc];
      if (t < s) {
        Y[first + t + r * ldy] += v;
      } else {
        u[t - s + (int64_t)r * ul] += v;
      }
    }
    __syncthreads();
  }
  for (int k0 = 0; k0 < s; k0 += kCholNB) {
    const int w = min(kCholNB, s - k0);
    load_triangle(D, P + (int64_t)k0 * ld + k0, ld, w);
    for (int idx = tid; idx < w * nrhs; idx += 256) {
      const int k = idx % w, r = idx / w;
      yb[k * kCholMaxRhs + r] = Y[first + k0 + k + r * ldy];
    }
    __syncthreads();
    if (tid < nrhs) {
      const int r = tid;
      for (int j = 0; j < w; j++) {
        double acc = yb[j * kCholMaxRhs + r];
        for (int k = 0; k < j; k++) acc -= D[k * kLdsLd + j] * yb[k * kCholMaxRhs + r];
        acc /= D[j * kLdsLd + j];
        yb[j * kCholMaxRhs + r] = acc;
        Y[first + k0 + j + r * ldy] = acc;
      }
    }
    __syncthreads();
    const int i0 = k0 + w, nrow = m - i0;
    for (int idx = tid; idx < nrow * nrhs; idx += 256) {
      const int i = i0 + idx % nrow, r = idx / nrow;
      double acc = 0.0;
      for (int k = 0; k < w; k++) acc += P[(int64_t)(k0 + k) * ld + i] * yb[k * kCholMaxRhs + r];
      if (i < s) {
        Y[first + i + r * ldy] -= acc;
      } else {
        u[i - s + (int64_t)r * ul] -= acc;
      }
    }
    __syncthreads();
  }
}

// Backward: x_J = L11^-T (y_J - L21^T x_below); the rows below belong to ancestors, finished in earlier launches.
__global__ __launch_bounds__(256) void chol_bwd_kernel(CholDev d, const int *__restrict__ list, double *Y, int64_t ldy,
                                                       int nrhs) {
  __shared__ double D[kCholNB * kLdsLd], z[kCholNB * kCholMaxRhs];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, b = d.nb[J], m = s + b;
  const int ld = d.ld[J];
  const double *__restrict__ P = d.L + d.panel[J];
  const int *__restrict__ rows = d.below + d.rows_ptr[J];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nblk = (s + kCholNB - 1) / kCholNB;
  for (int kb = nblk - 1; kb >= 0; kb--) {
    const int k0 = kb * kCholNB, w = min(kCholNB, s - k0);
    load_triangle(D, P + (int64_t)k0 * ld + k0, ld, w);
    for (int p = wave; p < w * nrhs; p += 4) {
      const int k = p % w, r = p / w;
      const double *__restrict__ col = P + (int64_t)(k0 + k) * ld;
      double sum = 0.0;
      for (int i = k0 + w + lane; i < m; i += 64) {
        const double xv = i < s ? Y[first + i + r * ldy] : Y[rows[i - s] + r * ldy];
        sum += col[i] * xv;
      }
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      if (lane == 0) z[k * kCholMaxRhs + r] = Y[first + k0 + k + r * ldy] - sum;
    }
    __syncthreads();
    if (tid < nrhs) {
      const int r = tid;
      for (int k = w - 1; k >= 0; k--) {
        double acc = z[k * kCholMaxRhs + r];
        for (int j = k + 1; j < w; j++) acc -= D[k * kLdsLd + j] * z[j * kCholMaxRhs + r];
        acc /= D[k * kLdsLd + k];
        z[k * kCholMaxRhs + r] = acc;
        Y[first + k0 + k + r * ldy] = acc;
      }
    }
    __syncthreads();
  }
}

// ---- sweeps over a pointer table (SparseChol::sweep) ---------------------------------------------------------------
// The interior point's panels: up to kCholMaxRhs vectors a launch, each already in the elimination order, solved in
// place, forward and backward apart.  What differs from the two kernels above is the solve with the diagonal block.
// There one lane per right-hand side walks the block, so a single right-hand side -- what the interior point asks
// for several times an iteration -- leaves 255 lanes of 256 idle through every block of every front.  Here HALF A
// WAVEFRONT owns a right-hand side and lane i holds entry i of it in a register: column-oriented substitution, after
// y_j the lanes below (forward) or above (backward) it update their own entry with one LDS read each.
// LDS: D is the block's lower triangle, column-major with leading dimension 33 doubles.  Forward, the 32 lanes of a
// half read D[j * 33 + lane], consecutive doubles: one bank row, no conflict.  Backward they read D[lane * 33 + j],
// a stride of 33 doubles = 66 banks: lane l sits 2 l banks on, 32 distinct bank pairs.  rd holds the reciprocals of
// the diagonal (32 divisions in parallel once a block, none in the dependent chain); yb is [right-hand side][entry]
// with the same leading dimension, written by consecutive lanes and read as a broadcast by the L21 products.
// Every column sees the same operations in the same order whatever nv is: a column of a panel equals the column
// solved alone, bit for bit.

__device__ inline void load_triangle_rd(double *D, double *rd, const double *P, int ld, int w) {
  for (int idx = threadIdx.x; idx < w * w; idx += blockDim.x) {
    const int col = idx / w, row = idx % w;
    if (row >= col) {
      const double v = P[(int64_t)col * ld + row];
      D[col * kLdsLd + row] = v;
      if (row == col) rd[col] = 1.0 / v;
    }
  }
}

__global__ __launch_bounds__(256) void chol_fwd_panel_kernel(CholDev d, const int *__restrict__ list, CholPtrs Y,
                                                             int nv) {
  __shared__ double D[kCholNB * kLdsLd], yb[kCholMaxRhs * kLdsLd], rd[kCholNB];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, b = d.nb[J], m = s + b;
  const int ld = d.ld[J], ul = d.uld[J];
  const double *__restrict__ P = d.L + d.panel[J];
  double *u = d.arena + d.sol[J];
  const int tid = threadIdx.x, half = tid >> 5, hl = tid & 31;
  for (int idx = tid; idx < b * nv; idx += 256) u[idx % b + (int64_t)(idx / b) * ul] = 0.0;
  __syncthreads();
  for (int c = d.child_ptr[J]; c < d.child_ptr[J + 1]; c++) {
    const int C = d.child[c], bc = d.nb[C], ulc = d.uld[C];
    const int *__restrict__ rel = d.rel + d.rows_ptr[C];
    const double *__restrict__ uc = d.arena + d.sol[C];
    for (int idx = tid; idx < bc * nv; idx += 256) {
      const int i = idx % bc, r = idx / bc, t = rel[i];
      const double v = uc[i + (int64_t)r * ulc];
      if (t < s) {
        Y.p[r][first + t] += v;
      } else {
        u[t - s + (int64_t)r * ul] += v;
      }
    }
    __syncthreads();
  }
  for (int k0 = 0; k0 < s; k0 += kCholNB) {
    const int w = min(kCholNB, s - k0);
    load_triangle_rd(D, rd, P + (int64_t)k0 * ld + k0, ld, w);
    __syncthreads();
    for (int r0 = 0; r0 < nv; r0 += 8) {  // (uniform trip count: the shuffles below see whole half-wavefronts)
      const int r = r0 + half;
      const bool live = r < nv && hl < w;
      double *yr = Y.p[r < nv ? r : 0] + first + k0;
      double y = live ? yr[hl] : 0.0;
      for (int j = 0; j < w; j++) {
        const double yj = __shfl(y, j, 32) * rd[j];
        if (hl == j) y = yj;
        if (hl > j && hl < w) y -= D[j * kLdsLd + hl] * yj;
      }
      if (live) {
        yr[hl] = y;
        yb[r * kLdsLd + hl] = y;
      }
    }
    __syncthreads();
    const int i0 = k0 + w, nrow = m - i0;
    for (int idx = tid; idx < nrow * nv; idx += 256) {
      const int i = i0 + idx % nrow, r = idx / nrow;
      const double *__restrict__ yk = yb + r * kLdsLd;
      double acc = 0.0;
      for (int k = 0; k < w; k++) acc += P[(int64_t)(k0 + k) * ld + i] * yk[k];
      if (i < s) {
        Y.p[r][first + i] -= acc;
      } else {
        u[i - s + (int64_t)r * ul] -= acc;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void chol_bwd_panel_kernel(CholDev d, const int *__restrict__ list, CholPtrs Y,
                                                             int nv) {
  __shared__ double D[kCholNB * kLdsLd], z[kCholMaxRhs * kLdsLd], rd[kCholNB];
  const int J = list[blockIdx.x];
  const int first = d.first[J], s = d.first[J + 1] - first, b = d.nb[J], m = s + b;
  const int ld = d.ld[J];
  const double *__restrict__ P = d.L + d.panel[J];
  const int *__restrict__ rows = d.below + d.rows_ptr[J];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = tid >> 5, hl = tid & 31;
  const int nblk = (s + kCholNB - 1) / kCholNB;
  for (int kb = nblk - 1; kb >= 0; kb--) {
    const int k0 = kb * kCholNB, w = min(kCholNB, s - k0);
    load_triangle_rd(D, rd, P + (int64_t)k0 * ld + k0, ld, w);
    // z = y_block - L21^T x_below: a wavefront per (column, right-hand side), coalesced down the column
    for (int p = wave; p < w * nv; p += 4) {
      const int k = p % w, r = p / w;
      const double *__restrict__ col = P + (int64_t)(k0 + k) * ld;
      const double *yr = Y.p[r];
      double sum = 0.0;
      for (int i = k0 + w + lane; i < m; i += 64) sum += col[i] * (i < s ? yr[first + i] : yr[rows[i - s]]);
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      if (lane == 0) z[r * kLdsLd + k] = yr[first + k0 + k] - sum;
    }
    __syncthreads();
    for (int r0 = 0; r0 < nv; r0 += 8) {
      const int r = r0 + half;
      const bool live = r < nv && hl < w;
      double x = live ? z[r * kLdsLd + hl] : 0.0;
      for (int j = w - 1; j >= 0; j--) {
        const double xj = __shfl(x, j, 32) * rd[j];
        if (hl == j) x = xj;
        if (hl < j) x -= D[hl * kLdsLd + j] * xj;
      }
      if (live) Y.p[r][first + k0 + hl] = x;
    }
    __syncthreads();
  }
}

// workgroups of a packed sweep: one lane per (group, right-hand side)
unsigned pack_grid(int ngroup, int nrhs) { return (unsigned)(((int64_t)ngroup * nrhs + kPackLanes - 1) / kPackLanes); }

// One direction of a triangular sweep: level after level (ascending: forward), the packed groups of the level, then
// its unpacked fronts, a workgroup each.  `pack` and `front` are the kernel pair; the front kernel takes d, its
// level's list and front_args.
template <class PackKernel, class FrontKernel, class... FrontArgs>
void launch_levels(const CholSymbolic &sym, hipStream_t st, const CholDev &d, const int *glev_first,
                   const int *glev_root, const int *lev_sn, bool ascending, int nr, PackKernel pack, CholPtrs Yp,
                   double *Yb, int64_t ldy, FrontKernel front, FrontArgs... front_args) {
  for (int i = 0; i < sym.nlev; i++) {
    const int l = ascending ? i : sym.nlev - 1 - i;
    const CholLevelPlan plan = chol_level_plan(sym, l);
    if (plan.ngroup > 0) {
      hipLaunchKernelGGL(pack, dim3(pack_grid(plan.ngroup, nr)), dim3(kPackLanes), 0, st, d,
                         glev_first + sym.glev_ptr[l], glev_root + sym.glev_ptr[l], plan.ngroup, Yp, Yb, ldy, nr);
    }
    if (plan.nfront > 0) {
      hipLaunchKernelGGL(front, dim3(plan.nfront), dim3(256), 0, st, d, lev_sn + sym.lev_ptr[l], front_args...);
    }
  }
}

// ---- Schur complement (sparse_chol.hpp, "Schur complement") ---------------------------------------------------------
// The Schur supernode's fan-in is every interior subtree that touches the set -- thousands of children for a KKT
// system whose E is block-diagonal -- and chol_assemble_kernel / chol_fwd_kernel walk the children one after the other
// with a barrier each.  Here the analysis has turned the walk into a table: a lane per destination adds its sources
// in child order, which is the order and so the bits of that walk; no atomics, no barrier, nothing that depends on the
// packing cap.  Four sources are loaded ahead of their adds: the chain of a lane is the adds, not the memory latency.
__global__ __launch_bounds__(256) void chol_schur_gather_kernel(const int64_t *__restrict__ ptr,
                                                                const int64_t *__restrict__ dst,
                                                                const int64_t *__restrict__ src, int64_t ndst,
                                                                const double *__restrict__ arena, double *L) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= ndst) return;
  const int64_t at = dst[d], p1 = ptr[d + 1];
  int64_t p = ptr[d];
  double acc = L[at];
  for (; p + 4 <= p1; p += 4) {
    const double v0 = arena[src[p]], v1 = arena[src[p + 1]], v2 = arena[src[p + 2]], v3 = arena[src[p + 3]];
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; p < p1; p++) acc += arena[src[p]];
  L[at] = acc;
}

// the children's update vectors into the Schur rows of the right-hand sides: thread = (row, right-hand side)
__global__ __launch_bounds__(256) void chol_schur_fwd_kernel(const int64_t *__restrict__ vptr,
                                                             const int64_t *__restrict__ vsrc,
                                                             const int *__restrict__ vld, int ns, int first,
                                                             const double *__restrict__ arena, double *Y, int64_t ldy,
                                                             int nrhs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)ns * nrhs) return;
  const int i = (int)(idx % ns), r = (int)(idx / ns);
  double *y = Y + first + i + r * ldy;
  double acc = *y;
  for (int64_t q = vptr[i]; q < vptr[i + 1]; q++) acc += arena[vsrc[q] + (int64_t)r * vld[q]];
  *y = acc;
}

// S out of the Schur panel (lower triangle, column-major, leading dimension ld) as the full symmetric matrix
// (column-major, lds): a workgroup per 64 x 64 tile of the lower triangle, through LDS.  The panel is read down its
// columns and the lower triangle written the same way; the mirror image is written with the lanes running along the
// tile's COLUMNS, which are consecutive addresses of the upper triangle: every global access is a 512-byte run.  The
// tile's leading dimension of 65 doubles keeps both LDS access directions free of bank conflicts.
constexpr int kSchurLd = kCholTile + 1;
__global__ __launch_bounds__(256) void chol_schur_copy_kernel(const double *__restrict__ P, int ld, int ns,
                                                              double *__restrict__ S, int64_t lds) {
  __shared__ double T[kCholTile * kSchurLd];
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (tj > ti) return;
  const int R0 = ti * kCholTile, C0 = tj * kCholTile;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  for (int c = q; c < kCholTile; c += 4) {
    const int row = R0 + lane, col = C0 + c;
    const bool in = row < ns && col < ns && row >= col;
    const double v = in ? P[(int64_t)col * ld + row] : 0.0;
    T[c * kSchurLd + lane] = v;
    if (in) S[(int64_t)col * lds + row] = v;
  }
  __syncthreads();
  for (int r = q; r < kCholTile; r += 4) {
    const int row = R0 + r, col = C0 + lane;
    if (row < ns && col < ns && row > col) S[(int64_t)row * lds + col] = T[lane * kSchurLd + r];
  }
}

// ---- factored Schur complement: the dense sweeps (sparse_chol.hpp, "FACTORED SCHUR COMPLEMENT") ----------------------
// F = L2 (lower triangle, column-major, leading dimension ldF) of S~ = L2 L2^T or L2 Sigma2 L2^T, factored by the
// block-column kernels above through a one-front table.  A front of the elimination tree is swept by ONE workgroup
// (chol_fwd / chol_bwd); here the triangle is cut into panels of W columns (chol_schur_panels) and everything outside a
// panel's W x W diagonal block is spread over the device, a launch at a time.  Workgroups are ordered by launch
// boundaries only: no flags, no spin waits, no atomics.  Y is the ns Schur rows of a slab, nr <= kCholMaxRhs columns of
// leading dimension ldy, solved in place.  Every (row, right-hand side) is one chain of fused multiply-adds in a fixed
// order (plus a fixed tree in the backward gather), whatever nr or the grid: a column's bits do not depend on nr.
//   chol_schur_fwd_diag     one workgroup: the diagonal block, its 32-blocks walked in LDS as chol_fwd_panel_kernel
//                           does (stride-33 triangle, half a wavefront per right-hand side, reciprocal diagonal), the
//                           rows of the block below each 32-block updated by all 256 threads.  Latency-bound: W
//                           dependent substitution steps.
//   chol_schur_fwd_update   all rows below the panel, right-looking: a wavefront per (64 rows, 8 right-hand sides),
//                           lane = row, y -= sum over the panel's columns in ascending order; the panel's y through LDS
//                           as broadcast reads, the rows of L2 as 512-byte runs.  Reads the panel's part of L2 once per
//                           group of 8 columns (the groups of a tile share it in L2): 2 flop per 8 bytes and right-hand
//                           side, memory-bound at every nr <= 32.
//   chol_schur_bwd_gather   left-looking: a workgroup per (column of the panel, 8 right-hand sides) forms
//                           y_k - sum_{i below the panel} l_ik x_i down the contiguous column, thread t rows t, t + 256,
//                           ..., then the xor tree of a wavefront and ((w0 + w1) + (w2 + w3)).  Memory-bound like the
//                           update.
//   chol_schur_bwd_diag     one workgroup: the diagonal block from its last 32-block, chol_bwd_panel_kernel's walk.
// LDS: D and rd as in the panel kernels (no conflicts in either direction, see there); yb / z are [right-hand side][33].

// F <- lower(S) (+ lower(add)): thread = row, blockIdx.y strides the columns
__global__ __launch_bounds__(256) void chol_schur_load_kernel(const double *__restrict__ P, int ld, int ns,
                                                              const double *__restrict__ add, int64_t ldadd,
                                                              double *__restrict__ F, int ldF) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= ns) return;
  for (int col = blockIdx.y; col <= row; col += gridDim.y) {
    double v = P[(int64_t)col * ld + row];
    if (add) v += add[(int64_t)col * ldadd + row];
    F[(int64_t)col * ldF + row] = v;
  }
}

__global__ __launch_bounds__(256) void chol_schur_fwd_diag_kernel(const double *__restrict__ F, int ldF, int p0, int wp,
                                                                  double *Y, int64_t ldy, int nr) {
  __shared__ double D[kCholNB * kLdsLd], yb[kCholMaxRhs * kLdsLd], rd[kCholNB];
  const double *__restrict__ P = F + (int64_t)p0 * ldF + p0;
  double *Yp = Y + p0;
  const int tid = threadIdx.x, half = tid >> 5, hl = tid & 31;
  for (int k0 = 0; k0 < wp; k0 += kCholNB) {
    const int w = min(kCholNB, wp - k0);
    load_triangle_rd(D, rd, P + (int64_t)k0 * ldF + k0, ldF, w);
    __syncthreads();
    for (int r0 = 0; r0 < nr; r0 += 8) {  // (uniform trip count: the shuffles below see whole half-wavefronts)
      const int r = r0 + half;
      const bool live = r < nr && hl < w;
      double *yr = Yp + k0 + (int64_t)(r < nr ? r : 0) * ldy;
      double y = live ? yr[hl] : 0.0;
      for (int j = 0; j < w; j++) {
        const double yj = __shfl(y, j, 32) * rd[j];
        if (hl == j) y = yj;
        if (hl > j && hl < w) y -= D[j * kLdsLd + hl] * yj;
      }
      if (live) {
        yr[hl] = y;
        yb[r * kLdsLd + hl] = y;
      }
    }
    __syncthreads();
    const int i0 = k0 + w, nrow = wp - i0;
    for (int idx = tid; idx < nrow * nr; idx += 256) {
      const int i = i0 + idx % nrow, r = idx / nrow;
      const double *__restrict__ yk = yb + r * kLdsLd;
      double acc = 0.0;
      for (int k = 0; k < w; k++) acc = fma(P[(int64_t)(k0 + k) * ldF + i], yk[k], acc);
      Yp[i + (int64_t)r * ldy] -= acc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void chol_schur_fwd_update_kernel(const double *__restrict__ F, int ldF, int ns, int p0,
                                                                   int wp, double *Y, int64_t ldy, int nr) {
  __shared__ double yb[kCholSchurCols * kLdsLd];
  const int lane = threadIdx.x;
  const int row = p0 + wp + blockIdx.x * kCholSchurRows + lane;
  const int c0 = blockIdx.y * kCholSchurCols, ncol = min(kCholSchurCols, nr - c0);
  const bool live = row < ns;
  const double *__restrict__ Frow = F + (int64_t)p0 * ldF + (live ? row : p0);
  double acc[kCholSchurCols];
#pragma unroll
  for (int c = 0; c < kCholSchurCols; c++) acc[c] = 0.0;
  for (int k0 = 0; k0 < wp; k0 += kCholNB) {
    const int w = min(kCholNB, wp - k0);
    __syncthreads();  // (the chunk before has been read)
    for (int idx = lane; idx < ncol * w; idx += 64) {
      const int c = idx / w, k = idx % w;
      yb[c * kLdsLd + k] = Y[p0 + k0 + k + (int64_t)(c0 + c) * ldy];
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < w; k++) {
      const double f = Frow[(int64_t)(k0 + k) * ldF];
#pragma unroll
      for (int c = 0; c < kCholSchurCols; c++) {
        if (c < ncol) acc[c] = fma(f, yb[c * kLdsLd + k], acc[c]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < kCholSchurCols; c++) {
    if (c < ncol) Y[row + (int64_t)(c0 + c) * ldy] -= acc[c];
  }
}

__global__ __launch_bounds__(256) void chol_schur_bwd_gather_kernel(const double *__restrict__ F, int ldF, int ns,
                                                                    int p0, int wp, double *Y, int64_t ldy, int nr) {
  __shared__ double part[4 * kCholSchurCols];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = p0 + blockIdx.x;
  const int c0 = blockIdx.y * kCholSchurCols, ncol = min(kCholSchurCols, nr - c0);
  const double *__restrict__ Fc = F + (int64_t)col * ldF;
  const double *Yc = Y + (int64_t)c0 * ldy;
  double acc[kCholSchurCols];
#pragma unroll
  for (int c = 0; c < kCholSchurCols; c++) acc[c] = 0.0;
  for (int i = p0 + wp + tid; i < ns; i += 256) {
    const double f = Fc[i];
#pragma unroll
    for (int c = 0; c < kCholSchurCols; c++) {
      if (c < ncol) acc[c] = fma(f, Yc[i + (int64_t)c * ldy], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < kCholSchurCols; c++) {
    double sum = acc[c];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) part[wave * kCholSchurCols + c] = sum;
  }
  __syncthreads();
  if (tid < ncol) {
    const double sum = (part[tid] + part[kCholSchurCols + tid]) +
                       (part[2 * kCholSchurCols + tid] + part[3 * kCholSchurCols + tid]);
    Y[col + (int64_t)(c0 + tid) * ldy] -= sum;
  }
}

__global__ __launch_bounds__(256) void chol_schur_bwd_diag_kernel(const double *__restrict__ F, int ldF, int p0, int wp,
                                                                  double *Y, int64_t ldy, int nr) {
  __shared__ double D[kCholNB * kLdsLd], z[kCholMaxRhs * kLdsLd], rd[kCholNB];
  const double *__restrict__ P = F + (int64_t)p0 * ldF + p0;
  double *Yp = Y + p0;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = tid >> 5, hl = tid & 31;
  const int nblk = (wp + kCholNB - 1) / kCholNB;
  for (int kb = nblk - 1; kb >= 0; kb--) {
    const int k0 = kb * kCholNB, w = min(kCholNB, wp - k0);
    load_triangle_rd(D, rd, P + (int64_t)k0 * ldF + k0, ldF, w);
    // z = y_block - L21^T x over the later 32-blocks of the panel: a wavefront per (column, right-hand side)
    for (int p = wave; p < w * nr; p += 4) {
      const int k = p % w, r = p / w;
      const double *__restrict__ col = P + (int64_t)(k0 + k) * ldF;
      const double *yr = Yp + (int64_t)r * ldy;
      double sum = 0.0;
      for (int i = k0 + w + lane; i < wp; i += 64) sum = fma(col[i], yr[i], sum);
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      if (lane == 0) z[r * kLdsLd + k] = yr[k0 + k] - sum;
    }
    __syncthreads();
    for (int r0 = 0; r0 < nr; r0 += 8) {
      const int r = r0 + half;
      const bool live = r < nr && hl < w;
      double x = live ? z[r * kLdsLd + hl] : 0.0;
      for (int j = w - 1; j >= 0; j--) {
        const double xj = __shfl(x, j, 32) * rd[j];
        if (hl == j) x = xj;
        if (hl < j) x -= D[hl * kLdsLd + j] * xj;
      }
      if (live) Yp[k0 + hl + (int64_t)r * ldy] = x;
    }
    __syncthreads();
  }
}

// ---- retained matrix: value compaction, diagonal shift, product, residual, norms -------------------------------------
// (sparse_chol.hpp, "RETAINED MATRIX").  All panels are in elimination order, column-major, leading dimension ld.
//
// Product and residual.  A row of at most kCholLongRow entries belongs to one lane (chol_mat_rows_kernel: consecutive
// lanes take consecutive rows, so the stores and the loads of B are full runs and the gathers of X stay near the
// diagonal for the orderings used here); a longer row belongs to one wavefront (chol_mat_long_kernel: lane l sums
// entries l, l + 64, ..., then a fixed xor tree).  Which of the two a row gets depends on its length alone, and either
// way an output element is one chain of fma in entry order (plus the tree), whatever nr, the slab or the grid: column
// j has the same bits whatever other columns are in the panel.  A thread carries kMatCols columns so that the indices
// and values of its row are read once for them; the columns of a partial group are clamped to the last one, computed
// again and not stored.  No floating-point atomics: the column maxima go through an integer atomicMax on the bit
// pattern of |v| (order-independent; a NaN's pattern is above every finite one's, so it shows).
struct CholMat {
  const int *rowp, *col, *vidx;
  const double *aval;
};
constexpr int kMatCols = 4;
enum { MAT_PRODUCT, MAT_RESIDUAL, MAT_NORM };
// slots of the statistics array (bit patterns of non-negative doubles)
constexpr int kStatR = 0, kStatX = kCholMaxRhs, kStatB = 2 * kCholMaxRhs, kStatA = 3 * kCholMaxRhs;
constexpr int kStatCount = 3 * kCholMaxRhs + 4;

__device__ inline unsigned long long abs_bits(double v) { return (unsigned long long)__double_as_longlong(fabs(v)); }
__device__ inline unsigned long long wave_max_bits(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

__global__ void chol_compact_kernel(const int *__restrict__ ptr, const int *__restrict__ src, int64_t ndst,
                                    const double *__restrict__ vals, double *__restrict__ aval) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndst) return;
  double sum = 0.0;  // (the sum chol_scatter_kernel writes into L, bit for bit)
  for (int p = ptr[d]; p < ptr[d + 1]; p++) sum += vals[src[p]];
  aval[d] = sum;
}

// L_kk += shift_k (elimination order) after the scatter
__global__ void chol_shift_kernel(CholDev d, const int *__restrict__ sn_of, const double *__restrict__ shift, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int J = sn_of[k], c = k - d.first[J];
  d.L[d.panel[J] + (int64_t)c * (d.ld[J] + 1)] += shift[k];
}

template <int kMode>
__device__ inline void mat_finish(int i, int j0, int nr, const double acc[kMatCols], const double *__restrict__ X,
                                  const double *__restrict__ B, double *__restrict__ R, int64_t ld,
                                  unsigned long long rb[kMatCols], unsigned long long xb[kMatCols]) {
#pragma unroll
  for (int k = 0; k < kMatCols; k++) {
    if (j0 + k >= nr) continue;
    const int64_t at = i + (int64_t)(j0 + k) * ld;
    if (kMode == MAT_PRODUCT) {
      R[at] = acc[k];
    } else {
      const double r = B[at] - acc[k];
      R[at] = r;
      rb[k] = abs_bits(r);
      xb[k] = abs_bits(X[at]);
    }
  }
}

template <int kMode>
__global__ __launch_bounds__(256) void chol_mat_rows_kernel(CholMat m, int n, const double *__restrict__ X,
                                                            const double *__restrict__ B, double *__restrict__ R,
                                                            int64_t ld, int nr, unsigned long long *stats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int j0 = blockIdx.y * kMatCols;
  int beg = 0, end = 0;
  if (i < n) beg = m.rowp[i], end = m.rowp[i + 1];
  const bool mine = i < n && end - beg <= kCholLongRow;
  if (!mine) end = beg;
  double acc[kMatCols] = {0.0, 0.0, 0.0, 0.0};
  int64_t colat[kMatCols];
#pragma unroll
  for (int k = 0; k < kMatCols; k++) colat[k] = (int64_t)(j0 + k < nr ? j0 + k : nr - 1) * ld;
  for (int p = beg; p < end; p++) {
    const double a = m.aval[m.vidx[p]];
    if (kMode == MAT_NORM) {
      acc[0] += fabs(a);
    } else {
      const int c = m.col[p];
#pragma unroll
      for (int k = 0; k < kMatCols; k++) acc[k] = fma(a, X[c + colat[k]], acc[k]);
    }
  }
  if (kMode == MAT_NORM) {
    const unsigned long long top = wave_max_bits(abs_bits(acc[0]));
    if ((threadIdx.x & 63) == 0 && top != 0) atomicMax(&stats[kStatA], top);
    return;
  }
  unsigned long long rb[kMatCols] = {0, 0, 0, 0}, xb[kMatCols] = {0, 0, 0, 0};
  if (mine) mat_finish<kMode>(i, j0, nr, acc, X, B, R, ld, rb, xb);
  if (kMode == MAT_RESIDUAL) {
#pragma unroll
    for (int k = 0; k < kMatCols; k++) {
      if (j0 + k >= nr) continue;  // (uniform)
      const unsigned long long rtop = wave_max_bits(rb[k]), xtop = wave_max_bits(xb[k]);
      if ((threadIdx.x & 63) == 0) {
        if (rtop != 0) atomicMax(&stats[kStatR + j0 + k], rtop);
        if (xtop != 0) atomicMax(&stats[kStatX + j0 + k], xtop);
      }
    }
  }
}

template <int kMode>
__global__ __launch_bounds__(256) void chol_mat_long_kernel(CholMat m, const int *__restrict__ long_rows, int nlong,
                                                            const double *__restrict__ X, const double *__restrict__ B,
                                                            double *__restrict__ R, int64_t ld, int nr,
                                                            unsigned long long *stats) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j0 = blockIdx.y * kMatCols;
  if (w >= nlong) return;  // (the whole wavefront)
  const int i = long_rows[w];
  const int beg = m.rowp[i], end = m.rowp[i + 1];
  double acc[kMatCols] = {0.0, 0.0, 0.0, 0.0};
  int64_t colat[kMatCols];
#pragma unroll
  for (int k = 0; k < kMatCols; k++) colat[k] = (int64_t)(j0 + k < nr ? j0 + k : nr - 1) * ld;
  for (int p = beg + lane; p < end; p += 64) {
    const double a = m.aval[m.vidx[p]];
    if (kMode == MAT_NORM) {
      acc[0] += fabs(a);
    } else {
      const int c = m.col[p];
#pragma unroll
      for (int k = 0; k < kMatCols; k++) acc[k] = fma(a, X[c + colat[k]], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < (kMode == MAT_NORM ? 1 : kMatCols); k++) {
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
  }
  if (lane != 0) return;
  if (kMode == MAT_NORM) {
    atomicMax(&stats[kStatA], abs_bits(acc[0]));
    return;
  }
  unsigned long long rb[kMatCols] = {0, 0, 0, 0}, xb[kMatCols] = {0, 0, 0, 0};
  mat_finish<kMode>(i, j0, nr, acc, X, B, R, ld, rb, xb);
  if (kMode == MAT_RESIDUAL) {
#pragma unroll
    for (int k = 0; k < kMatCols; k++) {
      if (j0 + k >= nr) continue;
      atomicMax(&stats[kStatR + j0 + k], rb[k]);
      atomicMax(&stats[kStatX + j0 + k], xb[k]);
    }
  }
}

// max |b| of every column of a panel: grid (row blocks, columns)
__global__ __launch_bounds__(256) void chol_colmax_kernel(const double *__restrict__ P, int64_t ld, int n,
                                                          unsigned long long *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long top = wave_max_bits(i < n ? abs_bits(P[i + (int64_t)blockIdx.y * ld]) : 0ull);
  if ((threadIdx.x & 63) == 0 && top != 0) atomicMax(&out[blockIdx.y], top);
}

// X_j += D_j for the columns whose bit is set in mask (a slab has at most 32 columns)
__global__ void chol_update_masked_kernel(double *__restrict__ X, const double *__restrict__ D, int64_t ld, int n,
                                          int nr, uint32_t mask) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * nr) return;
  const int p = (int)(idx % n), r = (int)(idx / n);
  if ((mask >> r) & 1u) X[p + r * ld] += D[p + r * ld];
}

inline double bits_double(unsigned long long b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

}  // namespace

// the anonymous namespace's CholDev under a name the header can declare
struct SparseChol::DevTables : CholDev {};
SparseChol::DevTables SparseChol::dev() const {
  return {{d_first, d_b, d_ld, d_uld, d_panel, d_upd, d_sol, d_rows_ptr, d_below, d_rel, d_child_ptr, d_child, L,
           arena}};
}

int SparseChol::upload(bool embedded) {
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t arena_doubles = std::max(sym.arena, sym.sol_arena) + 4;
  const int64_t y_doubles = embedded ? 4 : sym.ldy() * kCholMaxRhs;
  if (arena.alloc((size_t)arena_doubles, true) != PO_OK || Y.alloc((size_t)y_doubles, true) != PO_OK ||
      L.alloc((size_t)sym.Lsize + 4, true) != PO_OK) {
    (void)hipGetLastError();
    set_error("sparse Cholesky: cannot allocate the factor (%lld bytes) and its work space (%lld bytes)",
              (long long)(8 * sym.Lsize), (long long)sym.work_bytes);
    return PO_ERR_ARG;
  }
  if (!embedded) PO_TRY(avals.alloc(sym.rows.size() + 4, false));
  PO_TRY(d_flag.alloc(4, false));
  PO_TRY(d_perm.upload(sym.perm));
  PO_TRY(d_first.upload(sym.sn_first));
  PO_TRY(d_b.upload(sym.sn_b));
  PO_TRY(d_ld.upload(sym.sn_ld));
  PO_TRY(d_uld.upload(sym.upd_ld));
  PO_TRY(d_below.upload(sym.below_rows));
  PO_TRY(d_rel.upload(sym.rel));
  PO_TRY(d_child_ptr.upload(sym.child_ptr));
  PO_TRY(d_child.upload(sym.child));
  PO_TRY(d_rows_ptr.upload(sym.rows_ptr));
  PO_TRY(d_panel.upload(sym.panel_off));
  PO_TRY(d_upd.upload(sym.upd_off));
  PO_TRY(d_sol.upload(sym.sol_off));
  PO_TRY(d_glev_first.upload(sym.glev_first));
  PO_TRY(d_glev_root.upload(sym.glev_root));
  PO_TRY(d_lev_sn.upload(sym.lev_sn));
  PO_TRY(d_chunk_sn.upload(sym.chunk_sn));
  PO_TRY(d_chunk_c0.upload(sym.chunk_c0));
  PO_TRY(d_tab.upload(sym.tab));
  if (!embedded) {
    PO_TRY(d_asm_ptr.upload(sym.asm_ptr));
    PO_TRY(d_asm_src.upload(sym.asm_src));
    PO_TRY(d_asm_dst.upload(sym.asm_dst));
  }
  if (sym.ns > 0) {
    PO_TRY(d_schur_ptr.upload(sym.schur_ptr));
    PO_TRY(d_schur_src.upload(sym.schur_src));
    PO_TRY(d_schur_dst.upload(sym.schur_dst));
    PO_TRY(d_schur_vptr.upload(sym.schur_vptr));
    PO_TRY(d_schur_vsrc.upload(sym.schur_vsrc));
    PO_TRY(d_schur_vld.upload(sym.schur_vld));
  }
  PO_HIP(hipDeviceSynchronize());
  return PO_OK;
}

int SparseChol::scatter(const int *ptr, const int64_t *dst, const int *src, int64_t ndst, const double *dvals) {
  PO_HIP(hipMemsetAsync(L, 0, ((size_t)sym.Lsize + 4) * sizeof(double), ctx->stream));
  if (ndst > 0) {
    hipLaunchKernelGGL(chol_scatter_kernel, dim3((unsigned)((ndst + 255) / 256)), dim3(256), 0, ctx->stream, ptr, dst,
                       src, ndst, dvals, L);
    PO_HIP(hipGetLastError());
  }
  if (d_shift && sym.n > 0) {
    hipLaunchKernelGGL(chol_shift_kernel, dim3((unsigned)((sym.n + 255) / 256)), dim3(256), 0, ctx->stream, dev(),
                       (const int *)d_sn_of, (const double *)d_shift, sym.n);
    PO_HIP(hipGetLastError());
  }
  have_values = true;
  factored = false;
  schur_ready = schur_factored = false;
  return PO_OK;
}

int SparseChol::setValuesDevice(const double *dvals) {
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t ndst = (int64_t)sym.asm_dst.size();
  if (keep) {
    if (ndst > 0) {
      hipLaunchKernelGGL(chol_compact_kernel, dim3((unsigned)((ndst + 255) / 256)), dim3(256), 0, ctx->stream,
                         (const int *)d_asm_ptr, (const int *)d_asm_src, ndst, dvals, aval.get());
      PO_HIP(hipGetLastError());
    }
    have_aval = true;
    have_anorm = false;
  }
  return scatter(d_asm_ptr, d_asm_dst, d_asm_src, ndst, dvals);
}

int SparseChol::setValuesHost(int64_t n, const int *colp, const int *rows, const double *vals) {
  PO_HIP(hipSetDevice(ctx->device));
  const bool same = n == sym.n && memcmp(colp, sym.colp.data(), ((size_t)n + 1) * sizeof(int)) == 0 &&
                    (sym.rows.empty() || memcmp(rows, sym.rows.data(), sym.rows.size() * sizeof(int)) == 0);
  if (same) {
    if (!sym.rows.empty())
      PO_HIP(hipMemcpyAsync(avals, vals, sym.rows.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PO_TRY(setValuesDevice(avals));
    PO_HIP(hipStreamSynchronize(ctx->stream));  // (the caller's array may go away)
    return PO_OK;
  }
  if (keep) {
    set_error("sparse Cholesky: while the matrix is kept, set_values takes the creation pattern only (the one-off "
              "table of another pattern has no place in the retained values)");
    return PO_ERR_ARG;
  }
  // another pattern: its own table, built on the host and used once
  std::vector<int> ptr, src;
  std::vector<int64_t> dst;
  PO_TRY(chol_scatter_table(sym, n, colp, rows, &ptr, &dst, &src));
  DevArray<int> tp, ts;
  DevArray<int64_t> td;
  DevArray<double> tv;
  PO_TRY(tp.upload(ptr));
  PO_TRY(ts.upload(src));
  PO_TRY(td.upload(dst));
  PO_TRY(tv.upload(std::vector<double>(vals, vals + colp[n])));
  const int rc = scatter(tp, td, ts, (int64_t)dst.size(), tv);
  (void)hipStreamSynchronize(ctx->stream);  // (the tables go away with this scope)
  return rc;
}

int SparseChol::beginAssembly(double **Lout) {
  PO_HIP(hipSetDevice(ctx->device));
  PO_HIP(hipMemsetAsync(L, 0, ((size_t)sym.Lsize + 4) * sizeof(double), ctx->stream));
  have_values = true;
  factored = false;
  *Lout = L;
  return PO_OK;
}

int SparseChol::factorAssembled(int *flag) {
  if (!have_values) {
    set_error("sparse Cholesky: factorAssembled() needs beginAssembly() since the last factorization");
    return PO_ERR_ARG;
  }
  PO_HIP(hipSetDevice(ctx->device));
  PO_TRY(launchFactor<false>(flag));
  have_values = false;
  factored = true;
  factored_kind = PO_CHOL_LLT;
  have_inertia = uncounted = false;
  return PO_OK;
}

int SparseChol::setFactorization(int k) {
  if (k != PO_CHOL_LLT && k != PO_CHOL_LDLT) {
    set_error("sparse Cholesky: unknown factorization kind %d (PO_CHOL_LLT = 0, PO_CHOL_LDLT = 1)", k);
    return PO_ERR_ARG;
  }
  if (k == PO_CHOL_LDLT && ctx && !d_sign) {
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(d_sign.alloc((size_t)sym.n + 4, false));
  }
  kind = k;
  return PO_OK;
}

int SparseChol::inertia(int64_t out[3]) const {
  if (!have_inertia) {
    set_error(uncounted ? "sparse Cholesky: the last L L^T factorization replaced non-positive pivots and does not "
                          "count them (factor() reported the first); PO_CHOL_LDLT gives the inertia of such a matrix"
                        : "sparse Cholesky: inertia() before factor()");
    return PO_ERR_ARG;
  }
  for (int i = 0; i < 3; i++) out[i] = inertia_[i];
  return PO_OK;
}

// every level of the numeric factorization, queued on the stream; pivots are flagged in `flag` (device)
template <bool kSigned>
int SparseChol::launchFactor(int *flag) {
  hipStream_t st = ctx->stream;
  int *const d_flag = flag;
  double *const sgn = kSigned ? d_sign : nullptr;
  const CholDev d = dev();
  for (int l = 0; l < sym.nlev; l++) {
    const CholLevelPlan plan = chol_level_plan(sym, l);
    if (plan.ngroup > 0) {  // (independent of the level's unpacked fronts)
      hipLaunchKernelGGL(chol_pack_factor_kernel<kSigned>, dim3((plan.ngroup + kPackLanes - 1) / kPackLanes),
                         dim3(kPackLanes), 0, st, d, d_glev_first + sym.glev_ptr[l], d_glev_root + sym.glev_ptr[l],
                         plan.ngroup, d_flag, sgn);
    }
    if (plan.nchunk > 0) {
      hipLaunchKernelGGL(chol_assemble_kernel, dim3(plan.nchunk), dim3(128), 0, st, d, d_chunk_sn + sym.chunk_ptr[l],
                         d_chunk_c0 + sym.chunk_ptr[l]);
    }
    if (plan.nschur > 0) launchSchurGather(1);  // (its children are below this level; the front is then left alone)
    const int nsmall = plan.nsmall;
    if (nsmall > 0) {
      hipLaunchKernelGGL(chol_small_kernel<kSigned>, dim3(nsmall), dim3(64), 0, st, d, d_lev_sn + sym.lev_ptr[l],
                         d_flag, sgn);
    }
    const int *big = d_lev_sn + sym.lev_ptr[l] + nsmall;
    for (int step = sym.step_ptr[l]; step < sym.step_ptr[l + 1]; step++) {
      const int kb = step - sym.step_ptr[l], nact = sym.step_nact[step];
      const int *htab = &sym.tab[sym.step_tab[step]];
      const int *dtab = d_tab + sym.step_tab[step];
      hipLaunchKernelGGL(chol_diag_kernel<kSigned>, dim3(nact), dim3(64), 0, st, d, big, kb, d_flag, sgn);
      const int total = htab[nact];
      if (total > 0) {
        int most = 0;
        for (int a = 0; a < nact; a++) most = std::max(most, htab[a + 1] - htab[a]);
        hipLaunchKernelGGL(chol_trsm_kernel<kSigned>, dim3(total), dim3(kCholTile), 0, st, d, big, dtab, nact, kb,
                           (const double *)sgn);
        hipLaunchKernelGGL(chol_update_kernel<kSigned>, dim3(total, most), dim3(256), 0, st, d, big, dtab, nact, kb,
                           (const double *)sgn);
      }
    }
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::factor(int *info) {
  if (info) *info = 0;
  if (!have_values) {
    set_error("sparse Cholesky: factor() needs values set since the last factorization");
    return PO_ERR_ARG;
  }
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // flag[0] = 0, flag[1] = 0x7f7f7f7f (above every index), the counts flag[2] = flag[3] = 0
  PO_HIP(hipMemsetAsync(d_flag, 0, 4 * sizeof(int), st));
  PO_HIP(hipMemsetAsync(d_flag + 1, 0x7f, sizeof(int), st));
  const bool ldlt = kind == PO_CHOL_LDLT;
  PO_TRY(ldlt ? launchFactor<true>(d_flag) : launchFactor<false>(d_flag));
  const int npiv = sym.n - sym.ns;  // the Schur supernode is not eliminated: the pivots are the interior's
  if (ldlt && npiv > 0) {
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)npiv + 1023) / 1024, 1024);
    hipLaunchKernelGGL(chol_count_negative_kernel, dim3(blocks), dim3(256), 0, st, (const double *)d_sign, npiv,
                       d_flag);
    PO_HIP(hipGetLastError());
  }
  int flag[4] = {0, 0, 0, 0};
  PO_HIP(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, st));
  PO_HIP(hipStreamSynchronize(st));
  have_values = false;
  factored = true;
  factored_kind = kind;
  schur_ready = sym.ns > 0;
  schur_factored = false;
  // (the counts came with the flag read: nothing of size n goes to the host).  The unsigned kernels count nothing:
  // a Cholesky factorization that replaced no pivot has n positive ones, one that did has no inertia to report.
  inertia_[1] = ldlt ? flag[2] : 0;
  inertia_[2] = ldlt ? flag[3] : 0;
  inertia_[0] = (int64_t)npiv - inertia_[1] - inertia_[2];
  have_inertia = ldlt || flag[0] == 0;
  uncounted = !have_inertia;
  if (flag[0] != 0) {
    // like LAPACK's info behind the reference's factor() (src/ParOptSparseCholesky.cpp:631): the pivot was
    // replaced by 1 and the factorization finished, the caller decides
    set_error(ldlt ? "sparse Cholesky (LDLT): zero or NaN pivot at permuted index %d"
                   : "sparse Cholesky: non-positive pivot at permuted index %d",
              flag[1]);
    if (info) *info = 1 + flag[1];
  }
  return PO_OK;
}

void SparseChol::solvePanel(double *P, int nr) {
  hipStream_t st = ctx->stream;
  const CholDev d = dev();
  const int64_t ldy = sym.ldy();
  const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
  const CholPtrs none = {};
  launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, true, nr, chol_pack_fwd_kernel<false>, none, P, ldy,
                chol_fwd_kernel, P, ldy, nr);
  double *P2 = P + (sym.n - sym.ns);  // the Schur rows (a handle with a factored S~ only: refuseWholeSolve)
  if (sym.ns > 0) {
    launchSchurFwd(P, nr);
    schurSweep(P2, ldy, nr, true);
  }
  if (factored_kind == PO_CHOL_LDLT) {  // (the interior's signs and, behind them, those of S~)
    hipLaunchKernelGGL(chol_sign_kernel, dim3(pg), dim3(256), 0, st, P, ldy, (const double *)d_sign, sym.n, nr);
  }
  if (sym.ns > 0) schurSweep(P2, ldy, nr, false);
  launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, false, nr, chol_pack_bwd_kernel<false>, none, P, ldy,
                chol_bwd_kernel, P, ldy, nr);
}

int SparseChol::refuseWholeSolve(const char *who) const {
  if (sym.ns == 0 || schur_factored) return PO_OK;
  set_error("sparse Cholesky: %s on a handle with a Schur set: the Schur supernode is not eliminated, the solve is its "
            "two halves solve_condense() and solve_expand() around the caller's own solve with S (get_schur()), or "
            "schur_factor() first: the handle then factors and solves with S itself", who);
  return PO_ERR_ARG;
}

int SparseChol::solveDevice(double *dx, int nrhs, int64_t ldx) {
  PO_TRY(refuseWholeSolve("solve()"));
  if (!factored) {
    set_error("sparse Cholesky: solve() before factor()");
    return PO_ERR_ARG;
  }
  if (nrhs < 0 || (nrhs > 1 && ldx < sym.n)) {
    set_error("sparse Cholesky: solve with nrhs %d, ldx %lld (size %d)", nrhs, (long long)ldx, sym.n);
    return PO_ERR_ARG;
  }
  if (sym.n == 0 || nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ldy = sym.ldy();
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    double *x = dx + (int64_t)r0 * ldx;
    const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Y, ldy, x, ldx, d_perm, sym.n, nr, 0);
    solvePanel(Y, nr);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Y, ldy, x, ldx, d_perm, sym.n, nr, 1);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::sweep(double *const *Yh, int nv, bool forward, bool backward) {
  if (!factored) {
    set_error("sparse Cholesky: sweep() before the factorization");
    return PO_ERR_ARG;
  }
  if (sym.n == 0 || nv <= 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const CholDev d = dev();
  for (int r0 = 0; r0 < nv; r0 += kCholMaxRhs) {  // (sol_off lays the update vectors out for kCholMaxRhs columns)
    const int nr = std::min(kCholMaxRhs, nv - r0);
    CholPtrs t;
    for (int j = 0; j < kCholMaxRhs; j++) t.p[j] = Yh[r0 + (j < nr ? j : 0)];
    if (forward) {
      launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, true, nr, chol_pack_fwd_kernel<true>, t, nullptr,
                    (int64_t)0, chol_fwd_panel_kernel, t, nr);
    }
    if (backward) {
      launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, false, nr, chol_pack_bwd_kernel<true>, t, nullptr,
                    (int64_t)0, chol_bwd_panel_kernel, t, nr);
    }
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::solveHost(double *x, int nrhs, int64_t ldx) {
  PO_TRY(refuseWholeSolve("solve()"));
  if (sym.n == 0 || nrhs <= 0) return solveDevice(nullptr, nrhs, ldx);
  if (nrhs > 1 && ldx < sym.n) return solveDevice(nullptr, nrhs, ldx);
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t count = (int64_t)(nrhs - 1) * ldx + sym.n;
  PO_TRY(hostBuffer(count));
  PO_HIP(hipMemcpyAsync(xbuf, x, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PO_TRY(solveDevice(xbuf, nrhs, ldx));
  PO_HIP(hipMemcpyAsync(x, xbuf, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}

// ---- Schur complement: reading S, the two halves of the solve ------------------------------------------------------
void SparseChol::launchSchurGather(int reps) {
  const int64_t ndst = (int64_t)sym.schur_dst.size();
  for (int k = 0; k < reps && ndst > 0; k++) {
    hipLaunchKernelGGL(chol_schur_gather_kernel, dim3((unsigned)((ndst + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const int64_t *)d_schur_ptr, (const int64_t *)d_schur_dst, (const int64_t *)d_schur_src, ndst,
                       (const double *)arena, L.get());
  }
}

int SparseChol::schurAssemblyProbe(bool chunked, int reps) {
  if (sym.ns == 0 || reps < 0) {
    set_error("sparse Cholesky: the assembly probe needs a handle with a Schur set and reps >= 0");
    return PO_ERR_ARG;
  }
  PO_HIP(hipSetDevice(ctx->device));
  if (!chunked) {
    launchSchurGather(reps);
  } else {
    const int nchunk = (sym.ns + kCholChunk - 1) / kCholChunk;
    if (!d_probe_sn) {
      std::vector<int> sn((size_t)nchunk, sym.schur_sn), c0((size_t)nchunk);
      for (int k = 0; k < nchunk; k++) c0[k] = k * kCholChunk;
      PO_TRY(d_probe_sn.upload(sn));
      PO_TRY(d_probe_c0.upload(c0));
    }
    const CholDev d = dev();
    for (int k = 0; k < reps; k++) {
      hipLaunchKernelGGL(chol_assemble_kernel, dim3(nchunk), dim3(128), 0, ctx->stream, d, (const int *)d_probe_sn,
                         (const int *)d_probe_c0);
    }
  }
  PO_HIP(hipGetLastError());
  return PO_OK;
}

int SparseChol::getSchurDevice(double *dS, int64_t lds) {
  if (sym.ns == 0) {
    set_error("sparse Cholesky: get_schur() needs a handle created with a Schur set");
    return PO_ERR_ARG;
  }
  if (!schur_ready) {
    set_error("sparse Cholesky: get_schur() is valid after factor() until the next set_values");
    return PO_ERR_ARG;
  }
  if (lds < sym.ns) {
    set_error("sparse Cholesky: get_schur() with lds %lld for a Schur set of %d", (long long)lds, sym.ns);
    return PO_ERR_ARG;
  }
  PO_HIP(hipSetDevice(ctx->device));
  const int S = sym.schur_sn;
  const unsigned nt = (unsigned)((sym.ns + kCholTile - 1) / kCholTile);
  hipLaunchKernelGGL(chol_schur_copy_kernel, dim3(nt, nt), dim3(256), 0, ctx->stream,
                     (const double *)(L.get() + sym.panel_off[S]), sym.sn_ld[S], sym.ns, dS, lds);
  PO_HIP(hipGetLastError());
  return PO_OK;
}

int SparseChol::getSchurHost(double *S, int64_t lds) {
  const int64_t count = (int64_t)sym.ns * sym.ns;
  if (sym.ns > 0 && schur_ready && lds >= sym.ns && count > sbuf_cap) {
    PO_HIP(hipSetDevice(ctx->device));
    sbuf_cap = 0;
    PO_TRY(sbuf.alloc((size_t)count, false));
    sbuf_cap = count;
  }
  PO_TRY(getSchurDevice(sbuf, lds < sym.ns ? lds : sym.ns));  // (it refuses what this entry refuses)
  const size_t width = (size_t)sym.ns * sizeof(double);
  PO_HIP(hipMemcpy2DAsync(S, (size_t)lds * sizeof(double), sbuf, width, width, (size_t)sym.ns, hipMemcpyDeviceToHost,
                          ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}

int SparseChol::halfSolveCheck(const char *who, int nrhs, int64_t ldx) {
  if (sym.ns == 0) {
    set_error("sparse Cholesky: %s needs a handle created with a Schur set", who);
    return PO_ERR_ARG;
  }
  if (!factored) {
    set_error("sparse Cholesky: %s before factor()", who);
    return PO_ERR_ARG;
  }
  if (nrhs < 0 || (nrhs > 1 && ldx < sym.n)) {
    set_error("sparse Cholesky: %s with nrhs %d, ldx %lld (size %d)", who, nrhs, (long long)ldx, sym.n);
    return PO_ERR_ARG;
  }
  return PO_OK;
}

// the children's update vectors into the Schur rows of the panel P (after the interior's forward levels)
void SparseChol::launchSchurFwd(double *P, int nr) {
  for (int l = 0; l < sym.nlev; l++) {
    if (chol_level_plan(sym, l).nschur == 0) continue;
    hipLaunchKernelGGL(chol_schur_fwd_kernel, dim3((unsigned)(((int64_t)sym.ns * nr + 255) / 256)), dim3(256), 0,
                       ctx->stream, (const int64_t *)d_schur_vptr, (const int64_t *)d_schur_vsrc,
                       (const int *)d_schur_vld, sym.ns, sym.n - sym.ns, (const double *)arena, P, sym.ldy(), nr);
  }
}

// Schur entries: g = b2 - A21 A11^-1 b1; interior entries: the forward-swept intermediate, which expand reads
int SparseChol::condenseDevice(double *dx, int nrhs, int64_t ldx) {
  PO_TRY(halfSolveCheck("solve_condense()", nrhs, ldx));
  if (nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const CholDev d = dev();
  const int64_t ldy = sym.ldy();
  const CholPtrs none = {};
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    double *x = dx + (int64_t)r0 * ldx, *P = Y;
    const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, P, ldy, x, ldx, d_perm, sym.n, nr, 0);
    launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, true, nr, chol_pack_fwd_kernel<false>, none, P, ldy,
                  chol_fwd_kernel, P, ldy, nr);
    launchSchurFwd(P, nr);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, P, ldy, x, ldx, d_perm, sym.n, nr, 1);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

// x2 in the Schur entries, the intermediate of condense in the interior ones: x1 = A11^-1 (b1 - A12 x2)
int SparseChol::expandDevice(double *dx, int nrhs, int64_t ldx) {
  PO_TRY(halfSolveCheck("solve_expand()", nrhs, ldx));
  if (nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const CholDev d = dev();
  const int64_t ldy = sym.ldy();
  const int ni = sym.n - sym.ns;
  const CholPtrs none = {};
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    double *x = dx + (int64_t)r0 * ldx, *P = Y;
    const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, P, ldy, x, ldx, d_perm, sym.n, nr, 0);
    if (factored_kind == PO_CHOL_LDLT && ni > 0) {  // (the interior's signs; the Schur columns have none)
      hipLaunchKernelGGL(chol_sign_kernel, dim3((unsigned)(((int64_t)ni * nr + 255) / 256)), dim3(256), 0, st, P, ldy,
                         (const double *)d_sign, ni, nr);
    }
    launch_levels(sym, st, d, d_glev_first, d_glev_root, d_lev_sn, false, nr, chol_pack_bwd_kernel<false>, none, P, ldy,
                  chol_bwd_kernel, P, ldy, nr);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, P, ldy, x, ldx, d_perm, sym.n, nr, 1);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::halfSolveHost(bool condense, double *x, int nrhs, int64_t ldx) {
  PO_TRY(halfSolveCheck(condense ? "solve_condense()" : "solve_expand()", nrhs, ldx));
  if (nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t count = (int64_t)(nrhs - 1) * ldx + sym.n;
  PO_TRY(hostBuffer(count));
  PO_HIP(hipMemcpyAsync(xbuf, x, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PO_TRY(condense ? condenseDevice(xbuf, nrhs, ldx) : expandDevice(xbuf, nrhs, ldx));
  PO_HIP(hipMemcpyAsync(x, xbuf, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}
int SparseChol::condenseHost(double *x, int nrhs, int64_t ldx) { return halfSolveHost(true, x, nrhs, ldx); }
int SparseChol::expandHost(double *x, int nrhs, int64_t ldx) { return halfSolveHost(false, x, nrhs, ldx); }

// ---- factored Schur complement: S~ = S + add in a buffer of its own, the dense sweeps --------------------------------
int SparseChol::schurFactorCheck(const char *who, int64_t ldadd) {
  if (sym.ns == 0) {
    set_error("sparse Cholesky: %s needs a handle created with a Schur set", who);
    return PO_ERR_ARG;
  }
  if (!schur_ready) {
    set_error("sparse Cholesky: %s is valid after factor() until the next set_values", who);
    return PO_ERR_ARG;
  }
  if (ldadd < sym.ns) {
    set_error("sparse Cholesky: %s with ldadd %lld for a Schur set of %d", who, (long long)ldadd, sym.ns);
    return PO_ERR_ARG;
  }
  return PO_OK;
}

// the block-column kernels of launchFactor on the one front F (first = {n - ns, n}, nb = 0)
template <bool kSigned>
void SparseChol::launchSchurFactor(int *flag) {
  hipStream_t st = ctx->stream;
  double *const sgn = kSigned ? d_sign : nullptr;
  const int ns = sym.ns;
  const int *ti = ftab_i;
  const int64_t *tl = ftab_l;
  const CholDev d = {ti, ti + 2, ti + 3, ti + 4, tl, tl + 1, tl, tl, nullptr, nullptr, nullptr, nullptr, F, F};
  const int *list = ti + 5;
  if (ns <= kCholSmall) {
    hipLaunchKernelGGL(chol_small_kernel<kSigned>, dim3(1), dim3(64), 0, st, d, list, flag, sgn);
    return;
  }
  const int steps = (ns + kCholNB - 1) / kCholNB;
  for (int kb = 0; kb < steps; kb++) {
    hipLaunchKernelGGL(chol_diag_kernel<kSigned>, dim3(1), dim3(64), 0, st, d, list, kb, flag, sgn);
    const int total = chol_row_tiles(ns, ns, kb);
    if (total > 0) {
      const int *dtab = ti + 6 + 2 * kb;  // {0, total}
      hipLaunchKernelGGL(chol_trsm_kernel<kSigned>, dim3(total), dim3(kCholTile), 0, st, d, list, dtab, 1, kb,
                         (const double *)sgn);
      hipLaunchKernelGGL(chol_update_kernel<kSigned>, dim3(total, total), dim3(256), 0, st, d, list, dtab, 1, kb,
                         (const double *)sgn);
    }
  }
}

int SparseChol::schurFactorDevice(const double *dadd, int64_t ldadd, int *info) {
  if (info) *info = 0;
  PO_TRY(schurFactorCheck("schur_factor()", dadd ? ldadd : (int64_t)sym.ns));
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int ns = sym.ns, S = sym.schur_sn;
  if (!F) {
    ldF = (ns + 1) / 2 * 2;
    const size_t count = (size_t)ldF * ns + 4;
    if (F.alloc(count, true) != PO_OK) {
      (void)hipGetLastError();
      set_error("sparse Cholesky: cannot allocate the factor of the Schur complement (%lld bytes)",
                (long long)(count * sizeof(double)));
      return PO_ERR_ARG;
    }
    fbytes = (int64_t)(count * sizeof(double));
    std::vector<int> ti = {sym.n - ns, sym.n, 0, ldF, 0, 0};
    for (int kb = 0; kb < (ns + kCholNB - 1) / kCholNB; kb++) {
      ti.push_back(0);
      ti.push_back(chol_row_tiles(ns, ns, kb));
    }
    PO_TRY(ftab_i.upload(ti));
    PO_TRY(ftab_l.upload(std::vector<int64_t>{0, 0}));
    PO_TRY(d_sflag.alloc(4, false));
  }
  schur_factored = false;
  hipLaunchKernelGGL(chol_schur_load_kernel, dim3((unsigned)((ns + 255) / 256), (unsigned)std::min(ns, 65535)),
                     dim3(256), 0, st, (const double *)(L.get() + sym.panel_off[S]), sym.sn_ld[S], ns, dadd, ldadd,
                     F.get(), ldF);
  PO_HIP(hipMemsetAsync(d_sflag, 0, 4 * sizeof(int), st));
  PO_HIP(hipMemsetAsync(d_sflag + 1, 0x7f, sizeof(int), st));
  const bool ldlt = factored_kind == PO_CHOL_LDLT;
  if (ldlt) {
    launchSchurFactor<true>(d_sflag);
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)ns + 1023) / 1024, 1024);
    hipLaunchKernelGGL(chol_count_negative_kernel, dim3(blocks), dim3(256), 0, st,
                       (const double *)(d_sign.get() + (sym.n - ns)), ns, d_sflag.get());
  } else {
    launchSchurFactor<false>(d_sflag);
  }
  PO_HIP(hipGetLastError());
  int flag[4] = {0, 0, 0, 0};
  PO_HIP(hipMemcpyAsync(flag, d_sflag, sizeof(flag), hipMemcpyDeviceToHost, st));
  PO_HIP(hipStreamSynchronize(st));
  schur_factored = true;
  schur_added = dadd != nullptr;
  schur_inertia_[1] = ldlt ? flag[2] : 0;
  schur_inertia_[2] = ldlt ? flag[3] : 0;
  schur_inertia_[0] = (int64_t)ns - schur_inertia_[1] - schur_inertia_[2];
  schur_have_inertia = ldlt || flag[0] == 0;
  if (flag[0] != 0) {
    set_error(ldlt ? "sparse Cholesky (LDLT): zero or NaN pivot of the Schur complement at permuted index %d"
                   : "sparse Cholesky: non-positive pivot of the Schur complement at permuted index %d",
              flag[1]);
    if (info) *info = 1 + flag[1];
  }
  return PO_OK;
}

int SparseChol::schurFactorHost(const double *add, int64_t ldadd, int *info) {
  if (!add) return schurFactorDevice(nullptr, ldadd, info);
  if (info) *info = 0;
  PO_TRY(schurFactorCheck("schur_factor()", ldadd));
  PO_HIP(hipSetDevice(ctx->device));
  const size_t count = (size_t)sym.ns * sym.ns, width = (size_t)sym.ns * sizeof(double);
  if (addbuf.size() < count) PO_TRY(addbuf.alloc(count, false));
  PO_HIP(hipMemcpy2DAsync(addbuf, width, add, (size_t)ldadd * sizeof(double), width, (size_t)sym.ns,
                          hipMemcpyHostToDevice, ctx->stream));
  return schurFactorDevice(addbuf, sym.ns, info);  // (it synchronises: the caller's array may go away)
}

int SparseChol::schurInertia(int64_t out[3]) const {
  if (!schur_factored || !schur_have_inertia) {
    set_error(schur_factored ? "sparse Cholesky: the last L L^T factorization of the Schur complement replaced "
                               "non-positive pivots and does not count them (schur_factor() reported the first)"
                             : "sparse Cholesky: schur_inertia() before schur_factor()");
    return PO_ERR_ARG;
  }
  for (int i = 0; i < 3; i++) out[i] = schur_inertia_[i];
  return PO_OK;
}

void SparseChol::schurSweep(double *Yb, int64_t ld, int nr, bool forward) {
  hipStream_t st = ctx->stream;
  const int ns = sym.ns;
  const double *Fp = F;
  const int ldf = ldF;
  const unsigned groups = (unsigned)((nr + kCholSchurCols - 1) / kCholSchurCols);
  if (forward) {
    chol_schur_panels(
        ns, sym.schur_w, true,
        [&](int p0, int w) {
          hipLaunchKernelGGL(chol_schur_fwd_diag_kernel, dim3(1), dim3(256), 0, st, Fp, ldf, p0, w, Yb, ld, nr);
        },
        [&](int p0, int w) {
          const unsigned tiles = (unsigned)((ns - p0 - w + kCholSchurRows - 1) / kCholSchurRows);
          hipLaunchKernelGGL(chol_schur_fwd_update_kernel, dim3(tiles, groups), dim3(64), 0, st, Fp, ldf, ns, p0, w, Yb,
                             ld, nr);
        });
  } else {
    chol_schur_panels(
        ns, sym.schur_w, false,
        [&](int p0, int w) {
          hipLaunchKernelGGL(chol_schur_bwd_diag_kernel, dim3(1), dim3(256), 0, st, Fp, ldf, p0, w, Yb, ld, nr);
        },
        [&](int p0, int w) {
          hipLaunchKernelGGL(chol_schur_bwd_gather_kernel, dim3((unsigned)w, groups), dim3(256), 0, st, Fp, ldf, ns, p0,
                             w, Yb, ld, nr);
        });
  }
}

int SparseChol::schurSolveDevice(double *dx2, int nrhs, int64_t ldx2) {
  if (sym.ns == 0) {
    set_error("sparse Cholesky: schur_solve() needs a handle created with a Schur set");
    return PO_ERR_ARG;
  }
  if (!schur_factored) {
    set_error("sparse Cholesky: schur_solve() is valid after schur_factor() until the next set_values or factor()");
    return PO_ERR_ARG;
  }
  if (nrhs < 0 || (nrhs > 1 && ldx2 < sym.ns)) {
    set_error("sparse Cholesky: schur_solve with nrhs %d, ldx2 %lld (Schur set of %d)", nrhs, (long long)ldx2, sym.ns);
    return PO_ERR_ARG;
  }
  if (nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int ns = sym.ns;
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    double *x = dx2 + (int64_t)r0 * ldx2;
    schurSweep(x, ldx2, nr, true);
    if (factored_kind == PO_CHOL_LDLT) {
      hipLaunchKernelGGL(chol_sign_kernel, dim3((unsigned)(((int64_t)ns * nr + 255) / 256)), dim3(256), 0, st, x, ldx2,
                         (const double *)(d_sign.get() + (sym.n - ns)), ns, nr);
    }
    schurSweep(x, ldx2, nr, false);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::schurSolveHost(double *x2, int nrhs, int64_t ldx2) {
  if (sym.ns == 0 || !schur_factored || nrhs <= 0 || (nrhs > 1 && ldx2 < sym.ns)) {
    return schurSolveDevice(nullptr, nrhs, ldx2);  // (it refuses what this entry refuses)
  }
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t count = (int64_t)(nrhs - 1) * ldx2 + sym.ns;
  PO_TRY(hostBuffer(count));
  PO_HIP(hipMemcpyAsync(xbuf, x2, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PO_TRY(schurSolveDevice(xbuf, nrhs, ldx2));
  PO_HIP(hipMemcpyAsync(x2, xbuf, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}

// ---- retained matrix, diagonal shift, refined solve ----------------------------------------------------------------
int SparseChol::setKeepMatrix(bool on) {
  if (!on) {
    keep = have_aval = have_anorm = false;
    for (DevArray<int> *a : {&d_mrowp, &d_mcol, &d_mvidx, &d_mlong}) a->reset();
    for (DevArray<double> *a : {&aval, &Bp, &Xp}) a->reset();
    d_stats.reset();
    return PO_OK;
  }
  if (keep) return PO_OK;
  if (2 * (int64_t)sym.asm_dst.size() > 2000000000LL) {
    set_error("sparse Cholesky: the retained matrix would have more than 2e9 entries");
    return PO_ERR_ARG;
  }
  chol_matrix_table(&sym);
  if (ctx) {
    if (!d_asm_ptr) {
      set_error("sparse Cholesky: an embedded factorization keeps no matrix");
      return PO_ERR_ARG;
    }
    PO_HIP(hipSetDevice(ctx->device));
    PO_TRY(d_mrowp.upload(sym.mat_rowp));
    PO_TRY(d_mcol.upload(sym.mat_col));
    PO_TRY(d_mvidx.upload(sym.mat_vidx));
    PO_TRY(d_mlong.upload(sym.mat_long));
    PO_TRY(aval.alloc(sym.asm_dst.size() + 4, true));
    PO_TRY(d_stats.alloc(kStatCount, true));
  }
  keep = true;
  have_aval = have_anorm = false;  // (values set before this call went into L only)
  return PO_OK;
}

int SparseChol::setDiagonalShift(const double *shift) {
  if (!shift) {
    d_shift.reset();
    d_sn_of.reset();
    return PO_OK;
  }
  PO_HIP(hipSetDevice(ctx->device));
  std::vector<double> permuted((size_t)sym.n);
  for (int k = 0; k < sym.n; k++) permuted[k] = shift[sym.perm[k]];
  PO_HIP(hipStreamSynchronize(ctx->stream));  // (a scatter that reads the previous shift may still be queued)
  PO_TRY(d_shift.upload(permuted));
  if (!d_sn_of) PO_TRY(d_sn_of.upload(sym.sn_of));
  return PO_OK;
}

int SparseChol::needMatrix(const char *who) {
  if (!keep) {
    set_error("sparse Cholesky: %s needs the retained matrix (keep_matrix is off)", who);
    return PO_ERR_ARG;
  }
  if (!have_aval) {
    set_error("sparse Cholesky: %s needs values set since keep_matrix was switched on", who);
    return PO_ERR_ARG;
  }
  return PO_OK;
}

void SparseChol::productPanel(const double *X, const double *B, double *R, int nr, unsigned long long *stats) {
  const CholMat m = {d_mrowp, d_mcol, d_mvidx, aval};
  const int64_t ld = sym.ldy();
  const int nlong = (int)sym.mat_long.size();
  const dim3 rows_grid((unsigned)((sym.n + 255) / 256), (unsigned)((nr + kMatCols - 1) / kMatCols));
  const dim3 long_grid((unsigned)((nlong + 3) / 4), rows_grid.y);
  hipStream_t st = ctx->stream;
  if (B) {
    hipLaunchKernelGGL(chol_mat_rows_kernel<MAT_RESIDUAL>, rows_grid, dim3(256), 0, st, m, sym.n, X, B, R, ld, nr,
                       stats);
    if (nlong > 0) {
      hipLaunchKernelGGL(chol_mat_long_kernel<MAT_RESIDUAL>, long_grid, dim3(256), 0, st, m, (const int *)d_mlong,
                         nlong, X, B, R, ld, nr, stats);
    }
  } else {
    hipLaunchKernelGGL(chol_mat_rows_kernel<MAT_PRODUCT>, rows_grid, dim3(256), 0, st, m, sym.n, X, B, R, ld, nr,
                       stats);
    if (nlong > 0) {
      hipLaunchKernelGGL(chol_mat_long_kernel<MAT_PRODUCT>, long_grid, dim3(256), 0, st, m, (const int *)d_mlong,
                         nlong, X, B, R, ld, nr, stats);
    }
  }
}

// ||A||_inf, once per set of values
int SparseChol::matrixNorm() {
  if (have_anorm) return PO_OK;
  hipStream_t st = ctx->stream;
  const CholMat m = {d_mrowp, d_mcol, d_mvidx, aval};
  const int nlong = (int)sym.mat_long.size();
  PO_HIP(hipMemsetAsync(d_stats + kStatA, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(chol_mat_rows_kernel<MAT_NORM>, dim3((unsigned)((sym.n + 255) / 256)), dim3(256), 0, st, m, sym.n,
                     (const double *)nullptr, (const double *)nullptr, (double *)nullptr, (int64_t)0, 1, d_stats.get());
  if (nlong > 0) {
    hipLaunchKernelGGL(chol_mat_long_kernel<MAT_NORM>, dim3((unsigned)((nlong + 3) / 4)), dim3(256), 0, st, m,
                       (const int *)d_mlong, nlong, (const double *)nullptr, (const double *)nullptr,
                       (double *)nullptr, (int64_t)0, 1, d_stats.get());
  }
  PO_HIP(hipGetLastError());
  unsigned long long bits = 0;
  PO_HIP(hipMemcpyAsync(&bits, d_stats + kStatA, sizeof(bits), hipMemcpyDeviceToHost, st));
  PO_HIP(hipStreamSynchronize(st));
  anorm = bits_double(bits);
  have_anorm = true;
  return PO_OK;
}

int SparseChol::matvecDevice(const double *dx, int64_t ldx, double *dy, int64_t ldy_user, int nrhs) {
  PO_TRY(needMatrix("matvec()"));
  if (nrhs < 0 || (nrhs > 1 && (ldx < sym.n || ldy_user < sym.n))) {
    set_error("sparse Cholesky: matvec with nrhs %d, ldx %lld, ldy %lld (size %d)", nrhs, (long long)ldx,
              (long long)ldy_user, sym.n);
    return PO_ERR_ARG;
  }
  if (sym.n == 0 || nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ldy = sym.ldy();
  if (!Xp) PO_TRY(Xp.alloc((size_t)(ldy * kCholMaxRhs), true));
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Xp.get(), ldy,
                       const_cast<double *>(dx) + (int64_t)r0 * ldx, ldx, d_perm.get(), sym.n, nr, 0);
    productPanel(Xp, nullptr, Y, nr, nullptr);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Y.get(), ldy, dy + (int64_t)r0 * ldy_user,
                       ldy_user, d_perm.get(), sym.n, nr, 1);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::hostBuffer(int64_t count) {
  if (count > xbuf_cap) {
    xbuf_cap = 0;
    PO_TRY(xbuf.alloc((size_t)count, false));
    xbuf_cap = count;
  }
  return PO_OK;
}

int SparseChol::matvecHost(const double *x, int64_t ldx, double *y, int64_t ldy_user, int nrhs) {
  if (sym.n == 0 || nrhs <= 0 || (nrhs > 1 && (ldx < sym.n || ldy_user < sym.n))) {
    return matvecDevice(nullptr, ldx, nullptr, ldy_user, nrhs);
  }
  PO_TRY(needMatrix("matvec()"));
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t xcount = (int64_t)(nrhs - 1) * ldx + sym.n, ycount = (int64_t)(nrhs - 1) * ldy_user + sym.n;
  PO_TRY(hostBuffer(xcount));
  if (ycount > ybuf_cap) {
    ybuf_cap = 0;
    PO_TRY(ybuf.alloc((size_t)ycount, true));
    ybuf_cap = ycount;
  }
  PO_HIP(hipMemcpyAsync(xbuf, x, (size_t)xcount * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PO_TRY(matvecDevice(xbuf, ldx, ybuf, ldy_user, nrhs));
  // (column by column: what lies between the columns of y is the caller's)
  const size_t pitch = (size_t)(nrhs > 1 ? ldy_user : sym.n) * sizeof(double);
  PO_HIP(hipMemcpy2DAsync(y, pitch, ybuf, pitch, (size_t)sym.n * sizeof(double), (size_t)nrhs, hipMemcpyDeviceToHost,
                          ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}

// Refined solve, slab by slab.  B, X and Y are panels in elimination order:
//   X = solve(B); k = 0
//   loop: R = B - A X into Y with max|r|_j and max|x|_j (one small copy to the host and one synchronisation a step);
//         eta_j = max|r|_j / (||A||_inf max|x|_j + max|b|_j);
//         column j stops when !(eta_j > tol) -- so a NaN stops --, or k == max_steps, or k > 0 and
//         !(eta_j <= eta_j_prev / 2) (LAPACK's xGERFS rule; no roll-back, the eta reported is the iterate's);
//         all stopped: done.  D = solve(R) in Y; X_j += D_j for the columns still running; k += 1
// A column that has stopped is swept along with the others and never updated: its result and its statistics are the
// ones it would have alone.
int SparseChol::solveRefinedDevice(double *dx, int nrhs, int64_t ldx, int max_steps, double tol, int *steps,
                                   double *eta0, double *eta) {
  PO_TRY(refuseWholeSolve("solve_refined()"));
  if (sym.ns > 0 && schur_added) {
    set_error("sparse Cholesky: solve_refined() after schur_factor() with an add: the retained A is not the matrix "
              "being solved (A22 + add is); call schur_factor() without one, or solve()");
    return PO_ERR_ARG;
  }
  PO_TRY(needMatrix("solve_refined()"));
  if (!factored) {
    set_error("sparse Cholesky: solve_refined() before factor()");
    return PO_ERR_ARG;
  }
  if (nrhs < 0 || (nrhs > 1 && ldx < sym.n)) {
    set_error("sparse Cholesky: solve_refined with nrhs %d, ldx %lld (size %d)", nrhs, (long long)ldx, sym.n);
    return PO_ERR_ARG;
  }
  if (max_steps < 0) max_steps = 5;                 // ITMAX of xGERFS
  if (!(tol >= 0.0)) tol = 2.220446049250313e-16;   // eps: a residual formed in fp64 is not known better
  if (sym.n == 0 || nrhs == 0) return PO_OK;
  PO_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ldy = sym.ldy();
  const size_t panel = (size_t)(ldy * kCholMaxRhs);
  if (!Xp) PO_TRY(Xp.alloc(panel, true));
  if (!Bp) PO_TRY(Bp.alloc(panel, true));
  PO_TRY(matrixNorm());
  for (int r0 = 0; r0 < nrhs; r0 += kCholMaxRhs) {
    const int nr = std::min(kCholMaxRhs, nrhs - r0);
    double *x = dx + (int64_t)r0 * ldx;
    const unsigned pg = (unsigned)(((int64_t)sym.n * nr + 255) / 256);
    const size_t bytes = (size_t)(ldy * nr) * sizeof(double);
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Bp.get(), ldy, x, ldx, d_perm.get(), sym.n, nr,
                       0);
    PO_HIP(hipMemsetAsync(d_stats, 0, kStatA * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(chol_colmax_kernel, dim3((unsigned)((sym.n + 255) / 256), (unsigned)nr), dim3(256), 0, st,
                       (const double *)Bp, ldy, sym.n, d_stats + kStatB);
    PO_HIP(hipMemcpyAsync(Y, Bp, bytes, hipMemcpyDeviceToDevice, st));
    solvePanel(Y, nr);
    PO_HIP(hipMemcpyAsync(Xp, Y, bytes, hipMemcpyDeviceToDevice, st));
    uint32_t running = nr == 32 ? 0xffffffffu : ((1u << nr) - 1u);
    double prev[kCholMaxRhs];
    for (int k = 0;; k++) {
      if (k > 0) PO_HIP(hipMemsetAsync(d_stats, 0, kStatB * sizeof(unsigned long long), st));
      productPanel(Xp, Bp, Y, nr, d_stats);
      PO_HIP(hipGetLastError());
      unsigned long long h[kStatA];
      PO_HIP(hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, st));
      PO_HIP(hipStreamSynchronize(st));
      for (int j = 0; j < nr; j++) {
        if (!((running >> j) & 1u)) continue;
        const double e = bits_double(h[kStatR + j]) / (anorm * bits_double(h[kStatX + j]) + bits_double(h[kStatB + j]));
        if (k == 0 && eta0) eta0[r0 + j] = e;
        if (eta) eta[r0 + j] = e;
        if (!(e > tol) || k == max_steps || (k > 0 && !(e <= 0.5 * prev[j]))) {
          running &= ~(1u << j);
          if (steps) steps[r0 + j] = k;
        }
        prev[j] = e;
      }
      if (running == 0) break;
      solvePanel(Y, nr);
      hipLaunchKernelGGL(chol_update_masked_kernel, dim3(pg), dim3(256), 0, st, Xp.get(), (const double *)Y, ldy,
                         sym.n, nr, running);
    }
    hipLaunchKernelGGL(chol_permute_kernel, dim3(pg), dim3(256), 0, st, Xp.get(), ldy, x, ldx, d_perm.get(), sym.n, nr,
                       1);
    PO_HIP(hipGetLastError());
  }
  return PO_OK;
}

int SparseChol::solveRefinedHost(double *x, int nrhs, int64_t ldx, int max_steps, double tol, int *steps, double *eta0,
                                 double *eta) {
  PO_TRY(refuseWholeSolve("solve_refined()"));
  if (sym.n == 0 || nrhs <= 0 || (nrhs > 1 && ldx < sym.n)) {
    return solveRefinedDevice(nullptr, nrhs, ldx, max_steps, tol, steps, eta0, eta);
  }
  PO_TRY(needMatrix("solve_refined()"));
  PO_HIP(hipSetDevice(ctx->device));
  const int64_t count = (int64_t)(nrhs - 1) * ldx + sym.n;
  PO_TRY(hostBuffer(count));
  PO_HIP(hipMemcpyAsync(xbuf, x, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PO_TRY(solveRefinedDevice(xbuf, nrhs, ldx, max_steps, tol, steps, eta0, eta));
  PO_HIP(hipMemcpyAsync(x, xbuf, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  return PO_OK;
}

}  // namespace po
