/* ParOptScaledQuasiNewton.h -- the reference's header name (src/ParOptScaledQuasiNewton.h), so that code written against smdogroup/paropt
 * recompiles unchanged: ParOptScaledQuasiNewton(prob, qn) from the MI355X facade.
 * Build: -I include/paropt_compat -I <mpi include>, link -lparopt_amd and the MPI library. */
#ifndef PAROPT_AMD_USE_MPI
#define PAROPT_AMD_USE_MPI 1
#endif
#include "../ParOptAMD.hpp"
