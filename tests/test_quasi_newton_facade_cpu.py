"""CPU checks of the quasi-Newton extension point (po_qn_create_callbacks, paropt_amd.CompactQuasiNewton): bad
arguments are refused with a message and nothing is dereferenced; the Python base class exists and is abstract in
the reference's sense.  The header / export / ctypes agreement is tests/test_capi_symbols.py."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

SOURCE = r"""
#include <type_traits>
#include "ParOptQuasiNewton.h"
#include "ParOptScaledQuasiNewton.h"
#include "ParOptProblem.h"

static_assert(std::is_abstract<ParOptCompactQuasiNewton>::value, "the reference's class is abstract");

class MyQN : public ParOptCompactQuasiNewton {
 public:
  MyQN() : ncalls(0) {}
  void setInitDiagonalType(ParOptQuasiNewtonDiagonalType _diagonal_type) { ncalls++; }
  void reset() { ncalls++; }
  int update(ParOptVec *x, const ParOptScalar *z, ParOptVec *zw, ParOptVec *s, ParOptVec *y) { ncalls++; return 0; }
  int update(ParOptVec *x, const ParOptScalar *z, ParOptVec *zw) { ncalls++; return 0; }
  void mult(ParOptVec *x, ParOptVec *y) { y->copyValues(x); }
  void multAdd(ParOptScalar alpha, ParOptVec *x, ParOptVec *y) { y->axpy(alpha, x); }
  int getCompactMat(ParOptScalar *_b0, const ParOptScalar **_d, const ParOptScalar **_M, ParOptVec ***Z) {
    *_b0 = 1.0; *_d = NULL; *_M = NULL; *Z = NULL;
    return 0;
  }
  int getMaxLimitedMemorySize() { return 0; }
  int ncalls;
};

class MyProblem : public ParOptProblem {
 public:
  MyProblem(MPI_Comm comm) : ParOptProblem(comm) { setProblemSizes(10, 1, 0); }
  void getVarsAndBounds(ParOptVec *x, ParOptVec *lb, ParOptVec *ub) {}
  int evalObjCon(ParOptVec *x, ParOptScalar *fobj, ParOptScalar *cons) { return 0; }
  int evalObjConGradient(ParOptVec *x, ParOptVec *g, ParOptVec **Ac) { return 0; }
};

// every method through a base pointer
int through_the_base(ParOptCompactQuasiNewton *qn, ParOptVec *x, ParOptVec *y, const ParOptScalar *z) {
  ParOptScalar b0;
  const ParOptScalar *d, *M;
  ParOptVec **Z;
  qn->setInitDiagonalType(PAROPT_YTS_OVER_STS);
  qn->reset();
  int rc = qn->update(x, z, NULL, x, y);
  rc += qn->update(x, z, NULL);
  qn->mult(x, y);
  qn->multAdd(0.5, x, y);
  return rc + qn->getCompactMat(&b0, &d, &M, &Z) + qn->getMaxLimitedMemorySize();
}

// reference code that holds the library's class as an object and hands a user class to the solver
void use_library_classes(ParOptProblem *prob, ParOptVec *x, ParOptVec *y) {
  ParOptLBFGS *lbfgs = new ParOptLBFGS(prob, 5);
  lbfgs->incref();
  lbfgs->mult(x, y);
  lbfgs->setBFGSUpdateType(PAROPT_DAMPED_UPDATE);
  ParOptCompactQuasiNewton *scaled = new ParOptScaledQuasiNewton(prob, new ParOptLBFGS(prob, 5));
  scaled->incref();
  ParOptInteriorPoint *opt = new ParOptInteriorPoint(prob, NULL);
  opt->incref();
  opt->setQuasiNewton(new MyQN());
  opt->setQuasiNewton(scaled);
  ParOptQuadraticSubproblem *sub = new ParOptQuadraticSubproblem(prob, new MyQN());
  sub->incref();
  sub->decref();
  opt->decref();
  scaled->decref();
  lbfgs->decref();
}

int main(int argc, char *argv[]) {
  ParOptCompactQuasiNewton *qn = new MyQN();
  qn->incref();
  qn->reset();
  int n = static_cast<MyQN *>(qn)->ncalls;
  qn->decref();
  return (n == 1 && argc > 100) ? (int)(size_t)&use_library_classes + (int)(size_t)&through_the_base : 0;
}
"""


def test_reference_style_quasi_newton_code_compiles_and_links(tmp_path):
    src = tmp_path / "user_qn.cpp"
    src.write_text(SOURCE)
    exe = str(tmp_path / "user_qn")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include", "paropt_compat"),
                           "-I/opt/conda/include", str(src), "-o", exe, "-L" + os.path.join(ROOT, "paropt_amd"),
                           "-lparopt_amd", "-Wl,-rpath," + os.path.join(ROOT, "paropt_amd"),
                           "/opt/conda/lib/libmpi.so", "-Wl,-rpath-link,/usr/lib/x86_64-linux-gnu",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/conda/lib"])
    assert os.path.exists(exe)


def _table(L, without=()):
    fns = dict(reset=L.QN_VOID_FN(lambda u: 0), update=L.QN_UPDATE_FN(lambda u, x, z, zw, s, y, rc: 0),
               mult=L.QN_MULT_FN(lambda u, x, y: 0), mult_add=L.QN_MULTADD_FN(lambda u, a, x, y: 0),
               get_compact_mat=L.QN_COMPACT_FN(lambda u, k, b, d, M, Z: 0), get_max_size=L.QN_SIZE_FN(lambda u, k: 0))
    cb = L.QnCallbacks()
    for name, fn in fns.items():
        if name not in without:
            setattr(cb, name, fn)
    return cb, fns


def test_bad_arguments_are_refused_not_dereferenced():
    import paropt_amd.lib as L

    lib = L.lib
    out = L.po_qn()
    cb, keep = _table(L)
    assert lib.po_qn_create_callbacks(None, 10, C.byref(cb), C.byref(out)) == 2
    assert b"ctx" in lib.po_last_error()
    fake_ctx = C.c_void_p(0x10)  # never dereferenced: the table is checked first
    assert lib.po_qn_create_callbacks(fake_ctx, 10, None, C.byref(out)) == 2
    assert b"cb" in lib.po_last_error()
    for missing in ("get_compact_mat", "update", "mult", "mult_add", "reset", "get_max_size"):
        cb2, keep2 = _table(L, without=(missing,))
        assert lib.po_qn_create_callbacks(fake_ctx, 10, C.byref(cb2), C.byref(out)) == 2
        assert b"mandatory" in lib.po_last_error()
    assert lib.po_qn_create_callbacks(fake_ctx, -1, C.byref(cb), C.byref(out)) == 2
    assert not out
    err = C.c_double()
    assert lib.po_qn_check_compact(None, 0, C.byref(err)) == 2
    assert b"qn" in lib.po_last_error()


def test_python_base_class_is_exported():
    import paropt_amd as pa

    assert issubclass(pa.ScaledQuasiNewton, pa.CompactQuasiNewton)
    for name in ("reset", "update", "updateMultipliers", "mult", "multAdd", "getCompactMat",
                 "getMaxLimitedMemorySize", "setInitDiagonalType", "checkCompactForm", "driver"):
        assert callable(getattr(pa.CompactQuasiNewton, name))
    for cls in (pa.LBFGS, pa.LSR1, pa.EigenQuasiNewton):
        assert callable(cls.checkCompactForm)
    for name in ("reset", "mult", "multAdd", "getCompactMat", "getMaxLimitedMemorySize"):
        with pytest.raises(NotImplementedError):
            getattr(pa.CompactQuasiNewton, name)(*([None] * {"reset": 1, "mult": 3, "multAdd": 4}.get(name, 1)))
