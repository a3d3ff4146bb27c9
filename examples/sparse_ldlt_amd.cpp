// ParOptSparseCholesky in LDLT mode on a saddle-point system of the user's own: the bilinear mass matrix M of
// sparse_cholesky_amd.cpp (an nx x nx mesh of four-node elements, two unknowns per node), bordered by one constraint
// row per 2 x 2 patch of nodes (B: the weight 1/4 on every unknown of the patch) and a regularised corner,
//
//       K = [ M   B^T     ]
//           [ B  -delta I ],   delta = 1.
//
//   sparse_ldlt_amd [nx] [ND|AMD|NATURAL]
//
// K is symmetric quasi-definite, so P K P^T = L S L^T exists with S = diag(+-1) under every ordering and no pivoting
// is needed (ParOptSparseCholesky::setFactorization(PAROPT_CHOLESKY_LDLT)).  b = K 1, so the solution is the vector of
// ones; the inertia must be (rows of M, rows of B, 0), anything else ends with a non-zero exit status.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ParOptAMD.hpp"

namespace {

double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

const double kElement[4][4] = {{4.0, 2.0, 2.0, 1.0}, {2.0, 4.0, 1.0, 2.0}, {2.0, 1.0, 4.0, 2.0}, {1.0, 2.0, 2.0, 4.0}};
const int kPatch = 2;          // nodes per side of a patch
const double kWeight = 0.25;   // entries of B
const double kDelta = 1.0;

struct Triplet {
  int row, col;
  double val;
};

// compressed columns of K from the element loop and the patch loop: count, prefix sum, fill.  Returns the rows of M.
int assemble(int nx, std::vector<int> *colp, std::vector<int> *rows, std::vector<double> *vals) {
  const int nodes_per_side = nx + 1, nm = 2 * nodes_per_side * nodes_per_side;
  const int patches_per_side = (nodes_per_side + kPatch - 1) / kPatch;
  const int size = nm + patches_per_side * patches_per_side;
  std::vector<Triplet> ent;
  ent.reserve((size_t)nx * nx * 32 + (size_t)nm * 2 + (size_t)(size - nm));
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
  const int size = (int)colp.size() - 1, nb = size - nm;
  std::vector<double> x((size_t)size, 0.0);
  for (int j = 0; j < size; j++) {
    for (int p = colp[j]; p < colp[j + 1]; p++) x[rows[p]] += vals[p];  // b = K 1
  }
  printf("size = %d  (M: %d, B: %d rows)\n", size, nm, nb);
  const double t0 = now();
  ParOptSparseCholesky *ldlt = new ParOptSparseCholesky(ctx, size, colp.data(), rows.data(), order);
  if (!ldlt->handle()) return 3;
  if (ldlt->setFactorization(PAROPT_CHOLESKY_LDLT) != 0) return 3;
  const double t1 = now();
  ldlt->setValues(size, colp.data(), rows.data(), vals.data());
  const double t2 = now();
  const int info = ldlt->factor();
  const double t3 = now();
  ldlt->solve(x.data());
  const double t4 = now();
  int n = 0, num_snodes = 0, nnzL = 0, pos = 0, neg = 0, replaced = 0;
  ldlt->getInfo(&n, &num_snodes, &nnzL);
  const int have = ldlt->getInertia(&pos, &neg, &replaced);
  printf("supernodes = %d  nnz(L) = %d  factor info = %d\n", num_snodes, nnzL, info);
  printf("inertia: %d %d %d\n", pos, neg, replaced);
  printf("Setup/order time: %12.5e\n", t1 - t0);
  printf("Set values  time: %12.5e\n", t2 - t1);
  printf("Factor time:      %12.5e\n", t3 - t2);
  printf("Solve time:       %12.5e\n", t4 - t3);
  double err2 = 0.0, errinf = 0.0;
  for (int i = 0; i < size; i++) {
    const double e = fabs(1.0 - x[i]);
    err2 += e * e;
    if (!(e <= errinf)) errinf = e;
  }
  printf("||x - e||: %25.15e\n", sqrt(err2));
  printf("||x - e||_inf: %25.15e\n", errinf);
  delete ldlt;
  po_ctx_destroy(ctx);
  if (have != 0 || pos != nm || neg != nb || replaced != 0) {
    fprintf(stderr, "inertia (%d, %d, %d) is not (%d, %d, 0)\n", pos, neg, replaced, nm, nb);
    return 5;
  }
  return info == 0 ? 0 : 4;
}
