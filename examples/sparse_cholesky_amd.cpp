// ParOptSparseCholesky on a matrix of the user's own: the bilinear mass matrix of an nx x nx mesh of four-node
// elements with two unknowns per node, factored and solved on the device.
//
//   sparse_cholesky_amd [nx] [ND|AMD|NATURAL]
//
// The matrix is handed over element by element, so entries shared by neighbouring elements are repeated in the
// pattern and summed by setValues.  b = A 1, so the solution is the vector of ones.
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

struct Triplet {
  int row, col;
  double val;
};

// compressed columns from the element loop: count, prefix sum, fill
void assemble(int nx, std::vector<int> *colp, std::vector<int> *rows, std::vector<double> *vals) {
  const int nodes_per_side = nx + 1, size = 2 * nodes_per_side * nodes_per_side;
  std::vector<Triplet> ent;
  ent.reserve((size_t)nx * nx * 32);
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
  assemble(nx, &colp, &rows, &vals);
  const int size = (int)colp.size() - 1;
  std::vector<double> x((size_t)size, 0.0);
  for (int j = 0; j < size; j++) {
    for (int p = colp[j]; p < colp[j + 1]; p++) x[rows[p]] += vals[p];  // b = A 1
  }
  printf("size = %d\n", size);
  const double t0 = now();
  ParOptSparseCholesky *chol = new ParOptSparseCholesky(ctx, size, colp.data(), rows.data(), order);
  if (!chol->handle()) return 3;
  const double t1 = now();
  chol->setValues(size, colp.data(), rows.data(), vals.data());
  const double t2 = now();
  const int info = chol->factor();
  const double t3 = now();
  chol->solve(x.data());
  const double t4 = now();
  int n = 0, num_snodes = 0, nnzL = 0;
  chol->getInfo(&n, &num_snodes, &nnzL);
  printf("supernodes = %d  nnz(L) = %d  factor info = %d\n", num_snodes, nnzL, info);
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
  delete chol;
  po_ctx_destroy(ctx);
  return info == 0 ? 0 : 4;
}
