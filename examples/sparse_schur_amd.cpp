// ParOptSparseCholesky as a PARTIAL factorization: the saddle-point system of sparse_kkt_amd.cpp with a regularised
// corner,
//
//       K = [ M   B^T      ]      M: the bilinear mass matrix of an nx x nx mesh, two unknowns per node
//           [ B   -delta I ]      B: one constraint row per 2 x 2 patch of nodes, the weight 1/4 on its unknowns
//
// reduced onto the constraint block.
//
//   sparse_schur_amd [nx] [ND|AMD|NATURAL]
//
// The constraint unknowns are the Schur set (the constructor with nschur, schur_vars).  In L S L^T mode factor()
// eliminates the unknowns of M only and leaves S = -delta I - B M^-1 B^T on the device; the ordering type applies to
// M's graph.  The solve of K x = b, b = K 1, is then condense() (the constraint entries become g = b2 - B M^-1 b1),
// the caller's own solve S x2 = g -- here a few lines of host Cholesky on -S, which is SPD -- and expand()
// (x1 = M^-1 (b1 - B^T x2)).  Prints one JSON line: n, ns, the inertia of the interior pivots and the backward error
// eta = max|b - K x| / (||K||_inf max|x| + max|b|).  The inertia must be (rows of M, 0, 0), anything else ends with a
// non-zero exit status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ParOptAMD.hpp"

namespace {

const double kElement[4][4] = {{4.0, 2.0, 2.0, 1.0}, {2.0, 4.0, 1.0, 2.0}, {2.0, 1.0, 4.0, 2.0}, {1.0, 2.0, 2.0, 4.0}};
const int kPatch = 2;          // nodes per side of a patch
const double kWeight = 0.25;   // entries of B
const double kDelta = 1.0;     // the regularised corner: -kDelta I

struct Triplet {
  int row, col;
  double val;
};

// compressed columns of K from the element loop, the patch loop and the corner: count, prefix sum, fill.  Returns the
// rows of M.
int assemble(int nx, std::vector<int> *colp, std::vector<int> *rows, std::vector<double> *vals) {
  const int nodes_per_side = nx + 1, nm = 2 * nodes_per_side * nodes_per_side;
  const int patches_per_side = (nodes_per_side + kPatch - 1) / kPatch;
  const int size = nm + patches_per_side * patches_per_side;
  std::vector<Triplet> ent;
  ent.reserve((size_t)nx * nx * 32 + (size_t)nm * 2);
  for (int ey = 0; ey < nx; ey++) {
    for (int ex = 0; ex < nx; ex++) {
      const int node[4] = {ex + ey * nodes_per_side, ex + 1 + ey * nodes_per_side, ex + (ey + 1) * nodes_per_side,
                           ex + 1 + (ey + 1) * nodes_per_side};
      for (int dof = 0; dof < 2; dof++) {
        for (int a = 0; a < 4; a++) {
          for (int b = 0; b < 4; b++) ent.push_back({2 * node[a] + dof, 2 * node[b] + dof, kElement[a][b] / 9.0});
        }
      }
    }
  }
  for (int ny = 0; ny < nodes_per_side; ny++) {
    for (int nxi = 0; nxi < nodes_per_side; nxi++) {
      const int con = nm + (nxi / kPatch) + (ny / kPatch) * patches_per_side;
      for (int dof = 0; dof < 2; dof++) {
        const int u = 2 * (nxi + ny * nodes_per_side) + dof;
        ent.push_back({con, u, kWeight});  // B
        ent.push_back({u, con, kWeight});  // B^T
      }
    }
  }
  for (int con = nm; con < size; con++) ent.push_back({con, con, -kDelta});
  colp->assign((size_t)size + 1, 0);
  for (const Triplet &t : ent) (*colp)[t.col + 1]++;
  for (int j = 0; j < size; j++) (*colp)[j + 1] += (*colp)[j];
  rows->resize(ent.size());
  vals->resize(ent.size());
  std::vector<int> next(colp->begin(), colp->end() - 1);
  for (const Triplet &t : ent) {
    const int p = next[t.col]++;
    (*rows)[p] = t.row;
    (*vals)[p] = t.val;
  }
  return nm;
}


// x <- (-S)^-1 x by an unblocked Cholesky of the SPD matrix -S (column-major, order ns); false at a bad pivot
bool solve_negated_spd(std::vector<double> &S, int ns, double *x) {
  for (double &v : S) v = -v;
  for (int k = 0; k < ns; k++) {
    double piv = S[(size_t)k * ns + k];
    for (int j = 0; j < k; j++) piv -= S[(size_t)j * ns + k] * S[(size_t)j * ns + k];
    if (!(piv > 0.0)) return false;
    const double lkk = sqrt(piv);
    S[(size_t)k * ns + k] = lkk;
    for (int i = k + 1; i < ns; i++) {
      double v = S[(size_t)k * ns + i];
      for (int j = 0; j < k; j++) v -= S[(size_t)j * ns + i] * S[(size_t)j * ns + k];
      S[(size_t)k * ns + i] = v / lkk;
    }
  }
  for (int i = 0; i < ns; i++) {  // L y = x
    double v = x[i];
    for (int j = 0; j < i; j++) v -= S[(size_t)j * ns + i] * x[j];
    x[i] = v / S[(size_t)i * ns + i];
  }
  for (int i = ns - 1; i >= 0; i--) {  // L^T z = y
    double v = x[i];
    for (int j = i + 1; j < ns; j++) v -= S[(size_t)i * ns + j] * x[j];
    x[i] = v / S[(size_t)i * ns + i];
  }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  int nx = 64;
  ParOptOrderingType order = PAROPT_ND_ORDER;
  for (int k = 1; k < argc; k++) {
    if (strcmp(argv[k], "ND") == 0) {
      order = PAROPT_ND_ORDER;
    } else if (strcmp(argv[k], "AMD") == 0) {
      order = PAROPT_AMD_ORDER;
    } else if (strcmp(argv[k], "NATURAL") == 0) {
      order = PAROPT_NATURAL_ORDER;
    } else if (atoi(argv[k]) > 0) {
      nx = atoi(argv[k]);
    } else {
      fprintf(stderr, "usage: %s [nx] [ND|AMD|NATURAL]\n", argv[0]);
      return 1;
    }
  }
  po_ctx ctx = NULL;
  if (po_ctx_create(0, &ctx) != 0) {
    fprintf(stderr, "no MI355X available: %s\n", po_last_error());
    return 2;
  }
  std::vector<int> colp, rows;
  std::vector<double> vals;
  const int nm = assemble(nx, &colp, &rows, &vals);
  const int size = (int)colp.size() - 1, ns = size - nm;
  std::vector<double> b((size_t)size, 0.0);
  double knorm = 0.0;
  {
    std::vector<double> rowsum((size_t)size, 0.0);
    for (int j = 0; j < size; j++) {
      for (int p = colp[j]; p < colp[j + 1]; p++) b[rows[p]] += vals[p];  // b = K 1
    }
    // ||K||_inf of the assembled matrix: repeated entries add up first
    std::vector<double> col((size_t)size, 0.0);
    for (int j = 0; j < size; j++) {
      for (int p = colp[j]; p < colp[j + 1]; p++) col[rows[p]] += vals[p];
      for (int p = colp[j]; p < colp[j + 1]; p++) {
        rowsum[rows[p]] += fabs(col[rows[p]]);
        col[rows[p]] = 0.0;
      }
    }
    for (int i = 0; i < size; i++) knorm = rowsum[i] > knorm ? rowsum[i] : knorm;
  }
  std::vector<int> schur((size_t)ns);
  for (int k = 0; k < ns; k++) schur[k] = nm + k;
  ParOptSparseCholesky *kkt =
      new ParOptSparseCholesky(ctx, size, colp.data(), rows.data(), order, NULL, ns, schur.data());
  if (!kkt->handle() || kkt->getNumSchur() != ns) return 3;
  if (kkt->setFactorization(PAROPT_CHOLESKY_LDLT) != 0) return 3;
  kkt->setValues(size, colp.data(), rows.data(), vals.data());
  const int info = kkt->factor();
  int pos = 0, neg = 0, replaced = 0;
  const int have = kkt->getInertia(&pos, &neg, &replaced);
  std::vector<double> S((size_t)ns * ns), x(b);
  int failed = kkt->getSchur(S.data());
  failed |= kkt->condense(x.data());
  const bool spd = solve_negated_spd(S, ns, x.data() + nm);  // S x2 = g: (-S) x2 = -g
  for (int k = 0; k < ns; k++) x[nm + k] = -x[nm + k];
  failed |= kkt->expand(x.data());
  std::vector<double> r(b);
  for (int j = 0; j < size; j++) {
    for (int p = colp[j]; p < colp[j + 1]; p++) r[rows[p]] -= vals[p] * x[j];
  }
  double rmax = 0.0, xmax = 0.0, bmax = 0.0, errinf = 0.0;
  for (int i = 0; i < size; i++) {
    if (!(fabs(r[i]) <= rmax)) rmax = fabs(r[i]);
    if (!(fabs(x[i]) <= xmax)) xmax = fabs(x[i]);
    if (!(fabs(b[i]) <= bmax)) bmax = fabs(b[i]);
    if (!(fabs(1.0 - x[i]) <= errinf)) errinf = fabs(1.0 - x[i]);
  }
  const double eta = rmax / (knorm * xmax + bmax);
  printf("{\"n\": %d, \"ns\": %d, \"inertia\": [%d, %d, %d], \"eta\": %.17g, \"x_err_inf\": %.17g, "
         "\"factor_info\": %d}\n",
         size, ns, pos, neg, replaced, eta, errinf, info);
  delete kkt;
  po_ctx_destroy(ctx);
  if (failed != 0 || !spd) return 6;
  if (have != 0 || pos != nm || neg != 0 || replaced != 0) {
    fprintf(stderr, "interior inertia (%d, %d, %d) is not (%d, 0, 0)\n", pos, neg, replaced, nm);
    return 5;
  }
  return info == 0 ? 0 : 4;
}
