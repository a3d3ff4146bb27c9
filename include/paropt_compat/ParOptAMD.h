/* ParOptAMD.h -- the reference's header name (src/ParOptAMD.h, its approximate-minimum-degree ordering).  A FORWARDING
 * header only: it provides NONE of the reference's ordering functions -- this project has no minimum-degree code, and
 * PAROPT_AMD_ORDER of ParOptSparseCholesky gets the library's nested dissection.  It exists so that a program that
 * merely includes it beside ParOptSparseCholesky.h (the reference's examples/cholesky) compiles unchanged. */
#ifndef PAROPT_AMD_USE_MPI
#define PAROPT_AMD_USE_MPI 1
#endif
#include "../ParOptAMD.hpp"
