/* ParOptSparseUtils.h -- the reference's header name (src/ParOptSparseUtils.h, its CSR/CSC helper routines).  A
 * FORWARDING header only: it provides NONE of the reference's utility functions; the library does its sparse symbolic
 * work behind po_sparse_chol_create.  It exists so that a program that merely includes it beside
 * ParOptSparseCholesky.h (the reference's examples/cholesky) compiles unchanged. */
#ifndef PAROPT_AMD_USE_MPI
#define PAROPT_AMD_USE_MPI 1
#endif
#include "../ParOptAMD.hpp"
