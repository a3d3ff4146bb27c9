/* ParOptSparseCholesky.h -- the reference's header name (src/ParOptSparseCholesky.h), so that code written against smdogroup/paropt
 * recompiles unchanged: enum ParOptOrderingType and class ParOptSparseCholesky from the MI355X facade, with the
 * reference's communicator-free constructor on MPI_COMM_SELF (PAROPT_AMD_USE_MPI).
 * Build: -I include/paropt_compat -I <mpi include>, link -lparopt_amd and the MPI library. */
#ifndef PAROPT_AMD_USE_MPI
#define PAROPT_AMD_USE_MPI 1
#endif
#include "../ParOptAMD.hpp"
