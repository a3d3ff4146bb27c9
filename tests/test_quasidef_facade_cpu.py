"""CPU: the createQuasiDefMat extension point compiles and links the reference's way, and the C entry point refuses
NULL handles.

A translation unit written against the reference's interface (src/ParOptSparseMat.h:18-62, src/ParOptProblem.h:72)
-- a ParOptQuasiDefMat subclass with the reference's exact signatures, a problem whose createQuasiDefMat() returns it,
and calls of factor / apply / getFactorInfo on a ParOptQuasiDefBlockMat held as an object -- builds against the facade
through the reference's header name ParOptSparseMat.h.
"""
import ctypes as C
import os
import subprocess

from conftest import ROOT

SOURCE = r"""
#include "ParOptSparseMat.h"
#include "ParOptProblem.h"

class MySolver : public ParOptQuasiDefMat {
 public:
  MySolver() : nfactor(0) {}
  int factor(ParOptVec *x, ParOptVec *Dinv, ParOptVec *Cdiag) { nfactor++; return 0; }
  void apply(ParOptVec *bx, ParOptVec *yx, ParOptVec *yw) { yx->copyValues(bx); yw->zeroEntries(); }
  void apply(ParOptVec *bx, ParOptVec *bw, ParOptVec *yx, ParOptVec *yw) { yx->copyValues(bx); yw->copyValues(bw); }
  const char *getFactorInfo() { return "mine"; }
  int nfactor;
};

class MyProblem : public ParOptProblem {
 public:
  MyProblem(MPI_Comm comm) : ParOptProblem(comm) { setProblemSizes(10, 1, 4); }
  ParOptQuasiDefMat *createQuasiDefMat() { return new MySolver(); }
  void getVarsAndBounds(ParOptVec *x, ParOptVec *lb, ParOptVec *ub) {}
  int evalObjCon(ParOptVec *x, ParOptScalar *fobj, ParOptScalar *cons) { return 0; }
  int evalObjConGradient(ParOptVec *x, ParOptVec *g, ParOptVec **Ac) { return 0; }
};

// reference code that holds one of the library's own solvers as an object and calls it
const char *use_block_mat(ParOptProblem *prob, ParOptVec *x, ParOptVec *Dinv, ParOptVec *Cdiag, ParOptVec *bx,
                          ParOptVec *bw, ParOptVec *yx, ParOptVec *yw) {
  ParOptQuasiDefMat *mat = new ParOptQuasiDefBlockMat(prob, 1);
  mat->incref();
  int info = mat->factor(x, Dinv, Cdiag);
  mat->apply(bx, yx, yw);
  mat->apply(bx, bw, yx, yw);
  const char *text = info == 0 ? mat->getFactorInfo() : NULL;
  mat->decref();
  return text;
}

int main(int argc, char *argv[]) {
  ParOptQuasiDefMat *mat = new MySolver();
  mat->incref();
  const char *t = mat->getFactorInfo();
  mat->decref();
  return (t && t[0] == 'm' && argc > 100) ? (int)(size_t)&use_block_mat : 0;
}
"""


def test_reference_style_quasidef_code_compiles_and_links(tmp_path):
    src = tmp_path / "user_quasidef.cpp"
    src.write_text(SOURCE)
    exe = str(tmp_path / "user_quasidef")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include", "paropt_compat"),
                           "-I/opt/conda/include", str(src), "-o", exe, "-L" + os.path.join(ROOT, "paropt_amd"),
                           "-lparopt_amd", "-Wl,-rpath," + os.path.join(ROOT, "paropt_amd"),
                           "/opt/conda/lib/libmpi.so", "-Wl,-rpath-link,/usr/lib/x86_64-linux-gnu",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/conda/lib"])
    assert os.path.exists(exe)


def test_null_problem_is_refused_with_a_message():
    from paropt_amd import lib as L

    cb = L.QuasiDefCallbacks()
    assert L.lib.po_problem_set_quasidef_callbacks(None, C.byref(cb)) != 0
    assert b"null argument" in L.lib.po_last_error()
    assert L.lib.po_problem_set_quasidef_callbacks(None, None) != 0
    assert L.lib.po_xgram(None, None, 1, None) != 0
