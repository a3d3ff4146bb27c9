// ParOptSparseCholesky factoring and solving with its own Schur complement: the KKT system of sparse_kkt_amd.cpp,
//
//       K = [ M   B^T ]      M: the bilinear mass matrix of an nx x nx mesh, two unknowns per node
//           [ B   0   ]      B: one constraint row per 2 x 2 patch of nodes, the weight 1/4 on its unknowns
//
// reduced onto its constraint block as in sparse_schur_amd.cpp, and solved entirely on the device.
//
//   sparse_schur_solve_amd [nx] [ND|AMD|NATURAL]
//
// The constraint unknowns are the Schur set.  K has a zero corner, so the factorization is that of the REGULARISED
// matrix K + diag(shift), shift = -delta on the constraint rows (setDiagonalShift), with K itself kept beside the
// factor (setKeepMatrix).  factor() eliminates the unknowns of M and leaves S = -delta I - B M^-1 B^T on the device;
// factorSchur() factors it there (L2 Sigma2 L2^T, every sign negative); solveRefined() then runs the whole solve --
// interior forward sweep, dense sweeps with S, interior backward sweep -- and refines against K until the backward
// error eta = max|b - K x| / (||K||_inf max|x| + max|b|) of the UNREGULARISED system stops improving.  b = K 1.
// Prints one JSON line: n, ns, the inertia of the interior pivots and of S, the corrections applied, eta before the
// first and of the solution returned.  The inertias must be (rows of M, 0, 0) and (0, rows of B, 0), anything else ends
// with a non-zero exit status.
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
const double kDelta = 1e-6;    // the shift on the constraint rows

struct Triplet {
  int row, col;
  double val;
};

// compressed columns of K from the element loop and the patch loop: count, prefix sum, fill.  Returns the rows of M.
// The corner has no entries at all: the Schur set is a clique of the analysis, the shift fills its diagonal.
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
  std::vector<double> x((size_t)size, 0.0), shift((size_t)size, 0.0);
  for (int j = 0; j < size; j++) {
    for (int p = colp[j]; p < colp[j + 1]; p++) x[rows[p]] += vals[p];  // b = K 1
  }
  for (int i = nm; i < size; i++) shift[i] = -kDelta;
  std::vector<int> schur((size_t)ns);
  for (int k = 0; k < ns; k++) schur[k] = nm + k;
  ParOptSparseCholesky *kkt =
      new ParOptSparseCholesky(ctx, size, colp.data(), rows.data(), order, NULL, ns, schur.data());
  if (!kkt->handle() || kkt->getNumSchur() != ns) return 3;
  if (kkt->setFactorization(PAROPT_CHOLESKY_LDLT) != 0 || kkt->setKeepMatrix(true) != 0 ||
      kkt->setDiagonalShift(shift.data()) != 0) {
    return 3;
  }
  kkt->setValues(size, colp.data(), rows.data(), vals.data());
  const int info = kkt->factor();
  const int schur_info = kkt->factorSchur();
  int steps = -1, pos = 0, neg = 0, replaced = 0, spos = 0, sneg = 0, sreplaced = 0;
  double eta0 = 0.0, eta = 0.0;
  const int solved = kkt->solveRefined(x.data(), 1, -1, -1.0, &steps, &eta0, &eta);
  const int have = kkt->getInertia(&pos, &neg, &replaced) | kkt->getSchurInertia(&spos, &sneg, &sreplaced);
  double errinf = 0.0;
  for (int i = 0; i < size; i++) {
    const double e = fabs(1.0 - x[i]);
    if (!(e <= errinf)) errinf = e;
  }
  printf("{\"n\": %d, \"ns\": %d, \"inertia\": [%d, %d, %d], \"schur_inertia\": [%d, %d, %d], \"steps\": %d, "
         "\"eta0\": %.17g, \"eta\": %.17g, \"x_err_inf\": %.17g, \"factor_info\": %d, \"schur_factor_info\": %d}\n",
         size, ns, pos, neg, replaced, spos, sneg, sreplaced, steps, eta0, eta, errinf, info, schur_info);
  delete kkt;
  po_ctx_destroy(ctx);
  if (solved != 0) return 6;
  if (have != 0 || pos != nm || neg != 0 || replaced != 0 || spos != 0 || sneg != ns || sreplaced != 0) {
    fprintf(stderr, "inertia (%d, %d, %d) + (%d, %d, %d) is not (%d, 0, 0) + (0, %d, 0)\n", pos, neg, replaced, spos,
            sneg, sreplaced, nm, ns);
    return 5;
  }
  return info == 0 && schur_info == 0 ? 0 : 4;
}
