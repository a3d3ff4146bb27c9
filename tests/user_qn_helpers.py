"""User-side quasi-Newton approximations for the tests of the extension point (paropt_amd.CompactQuasiNewton):

  * OracleQN: the numpy classes oracle.paropt_oracle.LBFGS / LSR1 (test infrastructure pinned to the qn_ goldens) behind
    a small adapter, in the binding's host=True mode;
  * PVecLBFGS / PVecLSR1: limited-memory BFGS / SR1 (src/ParOptQuasiNewton.cpp:162-377, 636-747) written on the public
    vector operations of PVec alone.

Every class counts the calls it sees in `calls`."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import paropt_amd as pa
import paropt_amd.lib as L
from conftest import ROOT


def _diag_name(t):
    return "yts_over_sts" if t in (1, "yts_over_sts") else "yty_over_yts"


class OracleQN(pa.CompactQuasiNewton):
    def __init__(self, ctx, n, kind, msub, update_type="skip_negative_curvature"):
        from oracle import paropt_oracle as po

        self.calls = collections.Counter()
        if kind == "bfgs":
            self.inner = po.LBFGS(n, msub, po.VecOps(), update_type)
        else:
            self.inner = po.LSR1(n, msub, po.VecOps())
        super().__init__(ctx, n, host=True)

    def reset(self):
        self.calls["reset"] += 1
        self.inner.reset()

    def update(self, x, z, zw, s, y):
        self.calls["update"] += 1
        return self.inner.update(s, y)

    def mult(self, x, y):
        self.calls["mult"] += 1
        y[:] = self.inner.mult(x)

    def multAdd(self, alpha, x, y):
        self.calls["multAdd"] += 1
        self.inner.mult_add(alpha, x, y)

    def getCompactMat(self):
        self.calls["getCompactMat"] += 1
        return self.inner.get_compact()

    def getMaxLimitedMemorySize(self):
        return self.inner.max_size()

    def setInitDiagonalType(self, t):
        self.inner.diag_type = _diag_name(t)


class _PVecQN(pa.CompactQuasiNewton):
    def __init__(self, ctx, n, msub):
        self.calls = collections.Counter()
        self.m = int(msub)
        self.S = [pa.PVec(ctx, n) for _ in range(self.m)]
        self.Y = [pa.PVec(ctx, n) for _ in range(self.m)]
        self.r = pa.PVec(ctx, n)
        self.diag_type = "yty_over_yts"
        self._clear()
        super().__init__(ctx, n)

    def _clear(self):
        m = self.m
        self.msub, self.b0 = 0, 1.0
        self.D, self.L, self.B = np.zeros(m), np.zeros((m, m)), np.zeros((m, m))
        self.M, self.d, self.Z = np.zeros((0, 0)), np.zeros(0), []

    def reset(self):
        self.calls["reset"] += 1
        self._clear()

    def setInitDiagonalType(self, t):
        self.diag_type = _diag_name(t)

    def _inv(self, rz):
        return self.d * np.linalg.solve(self.M, self.d * rz) if len(rz) else rz

    def _store(self, s, y, sS, sY, sTs, sTy):
        """append / rotate a pair; the new Gram row from the dots with the pairs held before (old ordering)"""
        m, shift = self.m, 0
        if m == 0:
            return
        if self.msub < m:
            self.S[self.msub].copyValues(s)
            self.Y[self.msub].copyValues(y)
            self.msub += 1
        else:
            shift = 1
            self.S[0].copyValues(s)
            self.Y[0].copyValues(y)
            self.S = self.S[1:] + self.S[:1]
            self.Y = self.Y[1:] + self.Y[:1]
            k = self.msub
            self.D[:k - 1] = self.D[1:k].copy()
            self.B[:k - 1, :k - 1] = self.B[1:k, 1:k].copy()
            Lold = self.L.copy()
            for i in range(k - 1):
                for j in range(i):
                    self.L[i, j] = Lold[i + 1, j + 1]
        k = self.msub
        for i in range(k - 1):
            self.B[k - 1, i] = self.B[i, k - 1] = sS[i + shift]
            self.L[k - 1, i] = sY[i + shift]
        self.B[k - 1, k - 1] = sTs
        self.D[k - 1] = sTy

    def mult(self, x, y):
        self.calls["mult"] += 1
        y.copyValues(x)
        y.scale(self.b0)
        if self.Z:
            y.maxpy(1.0, -self._inv(x.mdot(self.Z)), self.Z)

    def multAdd(self, alpha, x, y):
        self.calls["multAdd"] += 1
        y.axpy(alpha * self.b0, x)
        if self.Z:
            y.maxpy(1.0, -alpha * self._inv(x.mdot(self.Z)), self.Z)

    def getCompactMat(self):
        self.calls["getCompactMat"] += 1
        return self.b0, self.d, self.M, self.Z


class PVecLBFGS(_PVecQN):
    def __init__(self, ctx, n, msub, update_type="skip_negative_curvature"):
        self.damped = update_type in (1, "damped_update", "damped")
        super().__init__(ctx, n, msub)

    def getMaxLimitedMemorySize(self):
        return 2 * self.m

    def update(self, x, z, zw, s, y):
        self.calls["update"] += 1
        k, mold = len(self.Z), len(self.Z) // 2
        dots = s.mdot(self.Z + [s, y])
        yTy = y.dot(y)
        sTs, yTs = dots[k], dots[k + 1]
        if 1e-8 * yTy >= abs(yTs):
            return 2
        coef = self._inv(dots[:k])
        sTBs = self.b0 * sTs - float(np.dot(dots[:k], coef))
        sts = self.diag_type == "yts_over_sts"
        if yTs >= 1e-12:
            b0_init = yTs / sTs if sts else yTy / yTs
        else:
            b0_init = 0.5 * (abs(yTy / yTs) + abs(yTs / sTs))
        rc, yu = 0, y
        if yTs >= 0.01 * sTBs:
            self.b0 = b0_init
        elif not self.damped:
            return 2
        else:
            rc = 1
            theta = 0.8 * sTBs / (sTBs - yTs)
            r = self.r  # r = (1 - theta) B s + theta y
            r.copyValues(s)
            r.scale((1.0 - theta) * self.b0)
            r.maxpy(1.0, np.concatenate([-(1.0 - theta) * coef, [theta]]), self.Z + [y])
            yu = r
            yTy, yTs = r.dot(r), r.dot(s)
            self.b0 = yTs / sTs if sts else yTy / yTs
        self._store(s, yu, dots[:mold], dots[mold:2 * mold], sTs, yTs)
        k = self.msub
        M = np.zeros((2 * k, 2 * k))
        M[:k, :k] = self.b0 * self.B[:k, :k]
        for i in range(k):
            for j in range(i):
                M[i, j + k] = M[j + k, i] = self.L[i, j]
            M[k + i, k + i] = -self.D[i]
        self.M = M
        self.d = np.concatenate([np.full(k, self.b0), np.ones(k)])
        self.Z = self.S[:k] + self.Y[:k]
        return rc


class PVecLSR1(_PVecQN):
    def __init__(self, ctx, n, msub):
        super().__init__(ctx, n, msub)
        self.Zown = [pa.PVec(ctx, n) for _ in range(self.m)]

    def getMaxLimitedMemorySize(self):
        return self.m

    def update(self, x, z, zw, s, y):
        self.calls["update"] += 1
        mold = self.msub
        dots = s.mdot(self.S[:mold] + self.Y[:mold] + [s, y])
        yTy = y.dot(y)
        sTs, sTy = dots[2 * mold], dots[2 * mold + 1]
        self.b0 = yTy / sTy if sTy > 1e-12 * yTy else 1.0
        self._store(s, y, dots[:mold], dots[mold:2 * mold], sTs, sTy)
        k = self.msub
        M = self.b0 * self.B[:k, :k].copy()
        for i in range(k):
            for j in range(i):
                M[i, j] -= self.L[i, j]
                M[j, i] -= self.L[i, j]
            M[i, i] -= self.D[i]
        self.M, self.d = M, np.ones(k)
        for i in range(k):  # Z_i = Y_i - b0 S_i: the columns change in content at every update
            self.Zown[i].copyValues(self.Y[i])
            self.Zown[i].axpy(-self.b0, self.S[i])
        self.Z = self.Zown[:k]
        return 0


_CPP = []


def cpp_library():
    """examples/libuser_quasi_newton.so: the C++ example's class behind extern "C" constructors"""
    if not _CPP:
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "libuser_quasi_newton.so"], env=env,
                              stdout=subprocess.DEVNULL)
        lib = C.CDLL(os.path.join(ROOT, "examples", "libuser_quasi_newton.so"))
        lib.user_qn_create.restype = C.c_void_p
        lib.user_qn_create.argtypes = [L.po_ctx, C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(L.po_qn)]
        lib.user_qn_calls.restype = None
        lib.user_qn_calls.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        lib.user_qn_destroy.restype = None
        lib.user_qn_destroy.argtypes = [C.c_void_p]
        _CPP.append(lib)
    return _CPP[0]


class CppLBFGS:
    """examples/user_quasi_newton_amd.cpp's UserLBFGS (a C++ subclass of ParOptCompactQuasiNewton with HIP kernels of
    its own), bound by the facade's trampolines; Python only holds the handle."""

    NAMES = ("reset", "update", "mult", "multAdd", "getCompactMat", "getMaxLimitedMemorySize")

    def __init__(self, ctx, n, msub, update_type="skip_negative_curvature", diag_type="yty_over_yts"):
        self.ctx, self._lib = ctx, cpp_library()
        self._h = L.po_qn()
        self._obj = self._lib.user_qn_create(ctx.handle, int(n), int(msub),
                                             int(update_type in (1, "damped_update", "damped")),
                                             int(_diag_name(diag_type) == "yts_over_sts"), C.byref(self._h))
        assert self._obj and self._h

    @property
    def calls(self):
        out = (C.c_long * 6)()
        self._lib.user_qn_calls(self._obj, out)
        return collections.Counter(dict(zip(self.NAMES, out)))

    def setInitDiagonalType(self, t):
        self.driver().setInitDiagonalType(t)

    def checkCompactForm(self, seed=0):
        return self.driver().checkCompactForm(seed)

    def driver(self):
        d = pa.api._QuasiNewton(self.ctx, 0, 0, 0, handle=self._h)
        d.user = self  # keeps the C++ object alive
        return d

    def __del__(self):
        try:
            if self._obj and self.ctx._h:
                self._lib.user_qn_destroy(self._obj)
        except Exception:
            pass


def make_user_qn(flavour, ctx, n, kind, msub, update_type="skip_negative_curvature", diag_type="yty_over_yts"):
    """flavour: "oracle" (numpy, host mode), "pvec" (device, public vector operations) or "cpp" (the C++ example's
    class, L-BFGS only)"""
    if flavour == "cpp":
        assert kind == "bfgs"
        return CppLBFGS(ctx, n, msub, update_type, diag_type)
    if flavour == "oracle":
        q = OracleQN(ctx, n, kind, msub, update_type)
    elif kind == "bfgs":
        q = PVecLBFGS(ctx, n, msub, update_type)
    else:
        q = PVecLSR1(ctx, n, msub)
    q.setInitDiagonalType(diag_type)
    return q
