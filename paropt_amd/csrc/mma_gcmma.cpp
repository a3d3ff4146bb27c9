// The conservative inner iteration of the globally convergent MMA (see mma_gcmma.hpp).  Host only: no HIP include.
#include "mma_gcmma.hpp"

#include <math.h>

#include <algorithm>
#include <vector>

namespace po {

void gcmma_rho_start(int m, const double *sums, int64_t nglobal, const GcmmaParams &p, double *rho) {
  const double scale = p.rho_init / (double)std::max<int64_t>(nglobal, 1);
  for (int i = 0; i <= m; i++) rho[i] = std::max(scale * sums[i], p.rho_min);
}

bool gcmma_accept(int m, const double *fnew, const double *fk, const double *sums, const double *rho, double tol,
                  double *viol) {
  const double D = sums[m + 1];
  bool ok = true;
  for (int i = 0; i <= m; i++) {
    viol[i] = fnew[i] - (fk[i] + sums[i] + rho[i] * D);
    if (!(viol[i] <= tol * std::max(1.0, fabs(fnew[i])))) ok = false;
  }
  return ok || D == 0.0;
}

void gcmma_raise(int m, const double *viol, double D, double *rho) {
  for (int i = 0; i <= m; i++) {
    const double delta = viol[i] / D;
    if (delta > 0.0) rho[i] = std::min(1.1 * (rho[i] + delta), 10.0 * rho[i]);
  }
}

int gcmma_inner(int m, const double *fk, const GcmmaParams &p, const GcmmaTrialFn &trial, double *rho, int *raises,
                bool *capped) {
  std::vector<double> sums(m + 2), fnew(m + 1), viol(m + 1);
  *raises = 0;
  *capped = false;
  for (;;) {
    const int rc = trial(rho, sums.data(), fnew.data());
    if (rc != 0) return rc;
    if (gcmma_accept(m, fnew.data(), fk, sums.data(), rho, p.tol, viol.data())) return 0;
    if (*raises >= p.max_inner) {
      *capped = true;
      return 0;
    }
    gcmma_raise(m, viol.data(), sums[m + 1], rho);
    (*raises)++;
  }
}

}  // namespace po
