"""
Python host harness over the C ABI (paropt_amd/lib.py).  Class and method names follow the
reference's Python layer (paropt/ParOpt.pyx:761-1521: PVec, LBFGS, LSR1, Problem,
InteriorPoint) so tests read like the reference's own; all arithmetic happens in
libparopt_amd.so on the GPU.
"""
import contextlib
import math
import ctypes as C

import numpy as np

from . import lib as L
from .lib import check, lib


def live_objects():
    """(device vectors alive in this process, HBM bytes behind them and behind the sparse factors' arrays): the leak
    check of the C ABI."""
    a, b = C.c_int64(), C.c_int64()
    check(lib.po_live_objects(C.byref(a), C.byref(b)))
    return a.value, b.value


def live_host_mirrors():
    """Pinned host mirrors (getArray) alive in this process."""
    a = C.c_int64()
    check(lib.po_live_host_mirrors(C.byref(a)))
    return a.value


class Context:
    """One per process / GPU: HIP stream + communicator (replaces the MPI communicator)."""

    def __init__(self, device=0):
        self._h = L.po_ctx()
        check(lib.po_ctx_create(int(device), C.byref(self._h)))
        self._keep = []

    @property
    def handle(self):
        return self._h

    def rank_size(self):
        r, s = C.c_int(), C.c_int()
        check(lib.po_ctx_rank(self._h, C.byref(r), C.byref(s)))
        return r.value, s.value

    def synchronize(self):
        check(lib.po_ctx_synchronize(self._h))

    def time_mdot(self, nvecs):
        """Bracket every mdot launch of exactly `nvecs` vectors with HIP events (0: off); resets the totals."""
        check(lib.po_ctx_time_mdot(self._h, int(nvecs)))

    def time_mdot_result(self):
        """(accumulated kernel milliseconds, launches) since time_mdot()."""
        ms, cnt = C.c_double(), C.c_int64()
        check(lib.po_ctx_time_mdot_result(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def time_wgram(self, on):
        """Bracket every weighted-Gram launch with HIP events (resets the totals)."""
        check(lib.po_ctx_time_wgram(self._h, int(bool(on))))

    def time_wgram_result(self, which):
        """(kernel ms, launches, panel width, algorithmic bytes) of the timed weighted-Gram launches;
        which = 0 plain launches, 1 launches that also form the L-SR1 columns."""
        ms, cnt, cols, byt = C.c_double(), C.c_int64(), C.c_int(), C.c_double()
        check(lib.po_ctx_time_wgram_result(self._h, int(which), C.byref(ms), C.byref(cnt), C.byref(cols),
                                           C.byref(byt)))
        return ms.value, cnt.value, cols.value, byt.value

    def comm_info(self):
        """(communicator kind: 0 self / 1 RCCL / 2 host callback, ncclAllReduce calls, ncclAllGather calls)."""
        k, a, b = C.c_int(), C.c_int64(), C.c_int64()
        check(lib.po_ctx_comm_info(self._h, C.byref(k), C.byref(a), C.byref(b)))
        return k.value, a.value, b.value

    def set_reduction_batching(self, on):
        """Let independent reductions share one collective + host sync (default on)."""
        check(lib.po_ctx_set_reduction_batching(self._h, int(bool(on))))
        return self

    def batched_reductions(self):
        """Reductions that shared another reduction's collective + host sync so far."""
        a = C.c_int64()
        check(lib.po_ctx_batched_reductions(self._h, C.byref(a)))
        return a.value

    def counters(self):
        """(host-synchronising reductions, kernel launches) issued on this context so far."""
        a, b = C.c_int64(), C.c_int64()
        check(lib.po_ctx_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sync_counters(self):
        """{flag_waits, flag_timeouts, allreduces, allgathers}: the polled completions of reductions, those that fell back
        to the stream synchronisation after the bounded spin, and the RCCL collectives issued (po_ctx_sync_counters)."""
        v = [C.c_int64() for _ in range(4)]
        check(lib.po_ctx_sync_counters(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("flag_waits", "flag_timeouts", "allreduces", "allgathers"), (x.value for x in v)))

    def bench_collective(self, count, pure_sum=True, reps=50):
        """{median, min, max} host microseconds of one reduction exchange of `count` doubles (collective)."""
        out = (C.c_double * 3)()
        check(lib.po_ctx_bench_collective(self._h, int(count), 1 if pure_sum else 0, int(reps), out))
        return {"median_us": out[0], "min_us": out[1], "max_us": out[2], "count": int(count),
                "form": "allreduce" if pure_sum else "allgather+host combine"}

    def allreduce(self, values, op="sum"):
        """MPI_Allreduce counterpart on host values (numpy float64 array, in place)."""
        import numpy as np

        a = np.ascontiguousarray(values, dtype=np.float64)
        check(lib.po_ctx_allreduce(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size,
                                   {"sum": 0, "min": 1, "max": 2}[op]))
        return a

    def algorithmic_bytes(self):
        """(total, issued from inside problem callbacks): algorithmic HBM bytes of the n-sized launches so far."""
        a, b = C.c_double(), C.c_double()
        check(lib.po_ctx_algorithmic_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def init_rccl_from_torch(self):
        """One process per GPU: ship the RCCL unique id over torch.distributed, then init."""
        import torch.distributed as dist

        rank, size = dist.get_rank(), dist.get_world_size()
        if size == 1:
            return

        def _all_ok(flag, what):
            # every rank takes the same decision, so a failure on one rank cannot leave the others
            # waiting inside a collective
            flags = [None] * size
            dist.all_gather_object(flags, bool(flag))
            if not all(flags):
                raise RuntimeError("%s failed on rank(s) %s" % (what, [r for r, f in enumerate(flags) if not f]))

        # 1. librccl loads and hands out an id on EVERY rank (dlopen + symbols), before any collective
        buf = (C.c_char * 128)()
        _all_ok(lib.po_rccl_unique_id(buf) == 0, "loading RCCL")
        # 2. rank 0's id to everyone, collective init, and agreement that it worked
        obj = [bytes(buf) if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        idbuf = (C.c_char * 128).from_buffer_copy(obj[0])
        _all_ok(lib.po_ctx_comm_init_rccl(self._h, rank, size, idbuf) == 0, "ncclCommInitRank")

    def init_callback_from_torch(self, device=None):
        """Host-side allgather through torch.distributed (gloo, or nccl with `device`): the
        maintainer's-MPI hook."""
        import torch
        import torch.distributed as dist

        rank, size = dist.get_rank(), dist.get_world_size()

        def _gather(inp, out, count, user):
            try:
                loc = torch.from_numpy(np.ctypeslib.as_array(inp, shape=(count,)).copy())
                if device is not None:
                    loc = loc.to(device)
                parts = [torch.empty_like(loc) for _ in range(size)]
                dist.all_gather(parts, loc)
                dst = np.ctypeslib.as_array(out, shape=(count * size,))
                for r in range(size):
                    dst[r * count : (r + 1) * count] = parts[r].cpu().numpy()
                return 0
            except Exception:  # pragma: no cover
                return 1

        cb = L.ALLGATHER_FN(_gather)
        self._keep.append(cb)
        check(lib.po_ctx_comm_init_callback(self._h, rank, size, cb, None))

    def device(self):
        """The device ordinal of the context (po_ctx_device)."""
        d = C.c_int()
        check(lib.po_ctx_device(self._h, C.byref(d)))
        return d.value

    def torch_stream(self):
        """The context's HIP stream as a torch.cuda.ExternalStream (one per context): torch work issued under
        `with torch.cuda.stream(ctx.torch_stream())` is ordered with the library's kernels without any
        synchronisation."""
        if getattr(self, "_torch_stream", None) is None:
            import torch

            self._torch_stream = torch.cuda.ExternalStream(lib.po_ctx_stream(self._h),
                                                           device=torch.device("cuda", self.device()))
        return self._torch_stream

    def close(self):
        """Destroy the context.  Objects created from it must not be used afterwards (their
        destructors become no-ops: the device memory went with the context's process)."""
        if self._h:
            lib.po_ctx_destroy(self._h)
            self._h = None


class PVec:
    """ParOptVec in HBM (reference: paropt/ParOpt.pyx PVec, src/ParOptVec.h:53-70)."""

    def __init__(self, ctx, n=None, handle=None, owned=True):
        self.ctx = ctx
        if handle is None:
            h = L.po_vec()
            check(lib.po_vec_create(ctx.handle, int(n), C.byref(h)))
            self._h = h
            self._owned = True
        else:
            self._h = handle if isinstance(handle, C.c_void_p) else L.po_vec(handle)
            self._owned = owned

    @property
    def handle(self):
        return self._h

    def __len__(self):
        n = C.c_int64()
        check(lib.po_vec_size(self._h, C.byref(n)))
        return n.value

    def __del__(self):
        try:
            if self._owned and self._h and self.ctx._h:
                lib.po_vec_decref(self._h)
        except Exception:
            pass

    # -- the 11 virtuals of ParOptVec --------------------------------------------------------
    def set(self, alpha):
        check(lib.po_vec_set(self._h, float(alpha)))

    def zeroEntries(self):
        check(lib.po_vec_zero(self._h))

    def copyValues(self, other):
        check(lib.po_vec_copy(self._h, other.handle))

    def norm(self):
        out = C.c_double()
        check(lib.po_vec_norm(self._h, C.byref(out)))
        return out.value

    def maxabs(self):
        out = C.c_double()
        check(lib.po_vec_maxabs(self._h, C.byref(out)))
        return out.value

    def l1norm(self):
        out = C.c_double()
        check(lib.po_vec_l1norm(self._h, C.byref(out)))
        return out.value

    def dot(self, other):
        out = C.c_double()
        check(lib.po_vec_dot(self._h, other.handle, C.byref(out)))
        return out.value

    def mdot(self, vecs):
        nv = len(vecs)
        out = np.zeros(max(nv, 1))
        arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
        check(lib.po_vec_mdot(self._h, arr, nv, out.ctypes.data_as(L.c_double_p)))
        return out[:nv]

    def scale(self, alpha):
        check(lib.po_vec_scale(self._h, float(alpha)))

    def axpy(self, alpha, other):
        check(lib.po_vec_axpy(self._h, float(alpha), other.handle))

    def maxpy(self, beta, alphas, vecs):
        nv = len(vecs)
        a = np.ascontiguousarray(alphas, dtype=np.float64)
        arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
        check(lib.po_vec_maxpy(self._h, float(beta), a.ctypes.data_as(L.c_double_p), arr, nv))

    def getArray(self):
        """The vector's data as a numpy view of its pinned host mirror, LIVE as in the reference (ParOptVec::getArray):
        writes through the view are seen by every later operation on the vector and results of operations show
        up in the view (po_vec_get_array); releaseArray() ends that state."""
        p = L.c_double_p()
        check(lib.po_vec_get_array(self._h, C.byref(p)))
        n = len(self)
        if n == 0:
            return np.zeros(0)
        return np.ctypeslib.as_array(p, shape=(n,))

    def _peek(self):
        p = L.c_double_p()
        check(lib.po_vec_peek_array(self._h, C.byref(p)))
        n = len(self)
        return np.ctypeslib.as_array(p, shape=(n,)) if n else np.zeros(0)

    def releaseArray(self, upload=True):
        """End the live state of the host mirror getArray() handed out (final upload unless upload=False).
        Required for vectors the solver owns before the solver runs on (po_vec_release_array)."""
        check(lib.po_vec_release_array(self._h, int(bool(upload))))

    def syncToDevice(self):
        check(lib.po_vec_sync_to_device(self._h))

    def syncToHost(self):
        check(lib.po_vec_sync_to_host(self._h))

    # -- conveniences --------------------------------------------------------------------------
    def to_numpy(self):
        return np.array(self._peek(), copy=True)

    def from_numpy(self, arr):
        a = self._peek()
        a[:] = arr
        self.syncToDevice()
        return self

    def fill_hash(self, seed, aid, offset=0, scale=1.0, shift=0.0):
        check(lib.po_vec_fill_hash(self._h, int(seed), int(aid), int(offset), float(scale), float(shift)))
        return self

    def device_ptr(self):
        p = L.c_double_p()
        check(lib.po_vec_get_device_array(self._h, C.byref(p)))
        return C.cast(p, C.c_void_p).value

    def as_tensor(self):
        """The vector's HBM as a torch tensor (1-D float64 on the context's device, no copy: data_ptr() ==
        device_ptr()).  The tensor holds a reference on the vector, so it stays valid after this wrapper and the
        solver that owns the vector are gone; releasing it after Context.close() is harmless.  A live host mirror
        (getArray) is uploaded and ended first.  Kernels on the tensor are ordered with the library's only under
        `torch.cuda.stream(ctx.torch_stream())` (po_vec_to_dlpack)."""
        mt = C.POINTER(L.DLManagedTensor)()
        check(lib.po_vec_to_dlpack(self._h, C.byref(mt)))
        return _tensor_from_dlpack(mt)


# DLPack capsules ("dltensor", consumed by torch.from_dlpack) made from a managed tensor pointer
_DLTENSOR = b"dltensor"
_PyCapsule_New = C.pythonapi.PyCapsule_New
_PyCapsule_New.restype = C.py_object
_PyCapsule_New.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]


def _tensor_from_dlpack(mt):
    import torch

    try:
        return torch.from_dlpack(_PyCapsule_New(C.cast(mt, C.c_void_p), _DLTENSOR, None))
    except BaseException:
        mt.contents.deleter(mt)  # not consumed: its owner is dropped here
        raise


_BORROWED = {}  # address of a borrowed managed tensor -> the ctypes objects behind it


@L.DL_DELETER_FN
def _borrowed_deleter(mt):
    try:
        _BORROWED.pop(C.addressof(mt.contents), None)
    except Exception:  # pragma: no cover - interpreter shutdown
        pass


def _borrowed_tensor(ptr, n, device):
    """A torch view of `n` doubles of device memory the library owns (no reference is held: valid while the owner
    is, e.g. a problem's sparse Jacobian values)."""
    mt = L.DLManagedTensor()
    shape = (C.c_int64 * 1)(int(n))
    t = mt.dl_tensor
    t.data = ptr
    t.device.device_type, t.device.device_id = L.DL_ROCM, int(device)
    t.ndim = 1
    t.dtype.code, t.dtype.bits, t.dtype.lanes = L.DL_FLOAT, 64, 1
    t.shape = C.cast(shape, L.c_i64_p)
    mt.deleter = _borrowed_deleter
    _BORROWED[C.addressof(mt)] = (mt, shape)
    return _tensor_from_dlpack(C.pointer(mt))


class _QuasiNewton:
    def __init__(self, ctx, kind, n, subspace, handle=None):
        self.ctx = ctx
        if handle is None:
            self._h = L.po_qn()
            check(lib.po_qn_create(ctx.handle, kind, int(n), int(subspace), C.byref(self._h)))
            self._owned = True
        else:
            self._h = handle
            self._owned = False

    def __del__(self):
        try:
            if self._owned and self._h and self.ctx._h:
                lib.po_qn_destroy(self._h)
        except Exception:
            pass

    def reset(self):
        check(lib.po_qn_reset(self._h))

    def update(self, s, y):
        rc = C.c_int()
        check(lib.po_qn_update(self._h, s.handle, y.handle, C.byref(rc)))
        return rc.value

    def mult(self, x, y):
        check(lib.po_qn_mult(self._h, x.handle, y.handle))

    def multAdd(self, alpha, x, y):
        check(lib.po_qn_mult_add(self._h, float(alpha), x.handle, y.handle))

    def setInitDiagonalType(self, t):
        check(lib.po_qn_set_diag_type(self._h, 1 if t in (1, "yts_over_sts") else 0))

    def debugLoad(self, b0, B, Lm, D, S, Y):
        """po_qn_debug_load: take over a complete limited-memory state (test hook).  B, Lm are (ld x ld) arrays in the
        reference's column-major storage (flat), D has ld entries, S / Y are lists of numpy vectors of the local size."""
        msub = len(S)
        ld = len(D)
        Bf = np.ascontiguousarray(B, dtype=np.float64).ravel()
        Lf = np.ascontiguousarray(Lm, dtype=np.float64).ravel()
        Df = np.ascontiguousarray(D, dtype=np.float64).ravel()
        sv = [PVec(self.ctx, len(v)).from_numpy(v) for v in S]
        yv = [PVec(self.ctx, len(v)).from_numpy(v) for v in Y]
        sh = (L.po_vec * max(msub, 1))(*[v.handle.value for v in sv])
        yh = (L.po_vec * max(msub, 1))(*[v.handle.value for v in yv])
        check(lib.po_qn_debug_load(self._h, msub, float(b0), Bf.ctypes.data_as(L.c_double_p),
                                   Lf.ctypes.data_as(L.c_double_p), Df.ctypes.data_as(L.c_double_p), ld, sh, yh))

    def checkCompactForm(self, seed=0):
        """max|mult(x) - (b0 x - Z d M^-1 d Z^T x)| / max|mult(x)| for a hashed probe x (po_qn_check_compact)."""
        err = C.c_double()
        _qn_check(lib.po_qn_check_compact(self._h, int(seed), C.byref(err)))
        return err.value

    def getCompactMat(self):
        k, b0 = C.c_int(), C.c_double()
        d0, M, Z = L.c_double_p(), L.c_double_p(), L.vec_p()
        check(lib.po_qn_get_compact(self._h, C.byref(k), C.byref(b0), C.byref(d0), C.byref(M), C.byref(Z)))
        n = k.value
        d = np.array([d0[i] for i in range(n)])
        Mm = np.array([M[i] for i in range(n * n)]).reshape(n, n).T if n else np.zeros((0, 0))
        Zs = [PVec(self.ctx, handle=L.po_vec(Z[i]), owned=False) for i in range(n)]
        return b0.value, d, Mm, Zs


class LBFGS(_QuasiNewton):
    def __init__(self, ctx, n, subspace=10, update_type="skip_negative_curvature"):
        super().__init__(ctx, 0, n, subspace)
        check(lib.po_qn_set_update_type(self._h, 1 if update_type in (1, "damped_update", "damped") else 0))


class LSR1(_QuasiNewton):
    def __init__(self, ctx, n, subspace=10):
        super().__init__(ctx, 1, n, subspace)


# The first exception thrown inside a callback of a user-written quasi-Newton approximation: the callback reports a
# failed call, the library winds down with PO_ERR_USER, and the optimize() that drove it re-raises the exception.
_QN_PENDING = [None]


def _raise_qn_pending():
    e, _QN_PENDING[0] = _QN_PENDING[0], None
    if e is not None:
        raise e


def _qn_check(rc):
    _raise_qn_pending()
    check(rc)


class CompactQuasiNewton(_QuasiNewton):
    """ParOptCompactQuasiNewton (reference src/ParOptQuasiNewton.h:32-67) as a base class to SUBCLASS: a compact
    quasi-Newton approximation B = b0 I - Z diag(d) M^-1 diag(d) Z^T written by the user, bound through
    po_qn_create_callbacks.  Override

        reset()
        update(x, z, zw, s, y) -> 0 normal | 1 damped | 2 skipped     (x, z, zw may be None)
        updateMultipliers(x, z, zw)                                    (optional)
        mult(x, y)                 y <- B x
        multAdd(alpha, x, y)       y <- y + alpha B x
        getCompactMat() -> (b0, d, M, Z)     M a (k, k) array with M[i, j] = row i, column j; Z a list of k PVec
        getMaxLimitedMemorySize() -> int
        setInitDiagonalType(t)                                         (optional)

    Vector arguments arrive as PVec wrappers of the library's vectors, valid during the call (`.as_tensor()` is the
    zero-copy torch view; with stream_scope=True every callback runs under `torch.cuda.stream(ctx.torch_stream())`).
    host=True: x, zw, s, y arrive as numpy copies, y of mult / multAdd as a live host array written in place, and Z may
    hold numpy arrays: the binding uploads them into vectors it owns and re-uploads a column only when its content
    changed.  z is a numpy array when `ncon` is known (InteriorPoint.setQuasiNewton fills it in), else the raw pointer.

    The library evaluates B through getCompactMat() alone; mult / multAdd serve the handle's po_qn_mult / po_qn_mult_add
    (checkCompactForm() compares the two).  An exception thrown in a callback is re-raised by optimize().  The object
    must stay alive while it is attached.  `driver()` returns the object as the LIBRARY sees it (update(s, y), mult,
    getCompactMat, ... through the C ABI and the callback table)."""

    def __init__(self, ctx, n, host=False, stream_scope=False, ncon=None):
        self.ctx, self.n, self.host, self.ncon = ctx, int(n), bool(host), ncon
        self._zcache = []  # host mode: (PVec, content) per column
        self._keep = None
        scope = contextlib.nullcontext
        if stream_scope:
            import torch

            stream = ctx.torch_stream()

            def scope():
                cur = torch.cuda.current_stream(stream.device)
                if cur.cuda_stream != stream.cuda_stream:
                    stream.wait_stream(cur)
                return torch.cuda.stream(stream)

        def vec(h):
            return PVec(ctx, handle=L.po_vec(h), owned=False) if h else None

        def arg(h):
            v = vec(h)
            return v.to_numpy() if (self.host and v is not None) else v

        def zarr(z):
            if not z:
                return None
            return np.array([z[i] for i in range(self.ncon)]) if self.ncon is not None else z

        def guard(fn):
            def _g(*args):
                if _QN_PENDING[0] is not None:
                    return 1
                try:
                    with scope():
                        return int(fn(*args) or 0)
                except BaseException as e:  # noqa: BLE001 - re-raised by optimize()
                    if _QN_PENDING[0] is None:
                        _QN_PENDING[0] = e
                    return 1
            return _g

        def _reset(user):
            self.reset()

        def _update(user, x, z, zw, s, y, rc):
            rc[0] = int(self.update(arg(x), zarr(z), arg(zw), arg(s), arg(y)) or 0)

        def _updmult(user, x, z, zw):
            self.updateMultipliers(arg(x), zarr(z), arg(zw))

        def out_call(fn, y):
            vy = vec(y)
            if not self.host:
                return fn(vy)
            try:
                return fn(vy.getArray())
            finally:
                vy.releaseArray(True)

        def _mult(user, x, y):
            ax = arg(x)
            out_call(lambda yy: self.mult(ax, yy), y)

        def _mult_add(user, alpha, x, y):
            ax = arg(x)
            out_call(lambda yy: self.multAdd(alpha, ax, yy), y)

        def _compact(user, size, b0, d, M, Z):
            b, dd, MM, ZZ = self.getCompactMat()
            k = len(ZZ)
            dd = np.ascontiguousarray(dd, dtype=np.float64).ravel()
            MM = np.asarray(MM, dtype=np.float64).reshape(k, k)
            if len(dd) != k:
                raise ValueError("getCompactMat: d has %d entries for %d columns of Z" % (len(dd), k))
            Mf = np.ascontiguousarray(MM.T).ravel()  # column-major, as the C ABI holds it
            cols = self._columns(ZZ)
            zh = (L.po_vec * max(k, 1))(*[v.handle.value for v in cols])
            self._keep = (dd, Mf, zh, cols)
            size[0], b0[0] = k, float(b)
            d[0] = dd.ctypes.data_as(L.c_double_p)
            M[0] = Mf.ctypes.data_as(L.c_double_p)
            Z[0] = C.cast(zh, L.vec_p)

        def _max_size(user, size):
            size[0] = int(self.getMaxLimitedMemorySize())

        def _diag(user, t):
            self._user_diag_type(t)

        cls = type(self)
        has_um = cls.updateMultipliers is not CompactQuasiNewton.updateMultipliers
        has_dt = cls.setInitDiagonalType is not CompactQuasiNewton.setInitDiagonalType
        self._user_diag_type = self.setInitDiagonalType if has_dt else (lambda t: None)
        cb = L.QnCallbacks()
        self._fns = (L.QN_VOID_FN(guard(_reset)), L.QN_UPDATE_FN(guard(_update)),
                     L.QN_UPDMULT_FN(guard(_updmult)) if has_um else L.QN_UPDMULT_FN(),
                     L.QN_MULT_FN(guard(_mult)), L.QN_MULTADD_FN(guard(_mult_add)), L.QN_COMPACT_FN(guard(_compact)),
                     L.QN_SIZE_FN(guard(_max_size)), L.QN_DIAG_FN(guard(_diag)) if has_dt else L.QN_DIAG_FN())
        cb.user = None
        (cb.reset, cb.update, cb.update_multipliers, cb.mult, cb.mult_add, cb.get_compact_mat, cb.get_max_size,
         cb.set_init_diagonal_type) = self._fns
        self._cb = cb
        self._h = L.po_qn()
        self._owned = True
        check(lib.po_qn_create_callbacks(ctx.handle, self.n, C.byref(cb), C.byref(self._h)))

    def _columns(self, ZZ):
        """Z as a list of PVec: host-mode numpy columns go through vectors the binding owns (uploaded on change)."""
        cols = []
        for i, zc in enumerate(ZZ):
            if isinstance(zc, PVec):
                cols.append(zc)
                continue
            a = np.asarray(zc, dtype=np.float64)
            if i >= len(self._zcache):
                self._zcache.append([PVec(self.ctx, len(a)), None])
            slot = self._zcache[i]
            if slot[1] is None or slot[1].shape != a.shape or not np.array_equal(slot[1], a):
                if len(slot[0]) != len(a):
                    slot[0] = PVec(self.ctx, len(a))
                slot[0].from_numpy(a)
                slot[1] = a.copy()
            cols.append(slot[0])
        return cols

    # -- the user's side: override these ---------------------------------------------------------
    def reset(self):
        raise NotImplementedError

    def update(self, x, z, zw, s, y):
        raise NotImplementedError

    def updateMultipliers(self, x, z, zw):
        return None

    def mult(self, x, y):
        raise NotImplementedError

    def multAdd(self, alpha, x, y):
        raise NotImplementedError

    def getCompactMat(self):
        raise NotImplementedError

    def getMaxLimitedMemorySize(self):
        raise NotImplementedError

    def setInitDiagonalType(self, t):
        return None

    def debugLoad(self, *args):
        raise L.ParOptAMDError(2, "a user-written approximation has no pair storage to load")

    def driver(self):
        return _QuasiNewtonDriver(self)


class _QuasiNewtonDriver(_QuasiNewton):
    """A user-written approximation as the library sees it: every call goes through the C ABI and the callback table."""

    def __init__(self, user):
        super().__init__(user.ctx, 0, 0, 0, handle=user._h)
        self.user = user

    def _call(self, fn, *args):
        try:
            return fn(*args)
        finally:
            _raise_qn_pending()

    def reset(self):
        return self._call(super().reset)

    def update(self, s, y):
        return self._call(super().update, s, y)

    def mult(self, x, y):
        return self._call(super().mult, x, y)

    def multAdd(self, alpha, x, y):
        return self._call(super().multAdd, alpha, x, y)

    def getCompactMat(self):
        return self._call(super().getCompactMat)

    def checkCompactForm(self, seed=0):
        return self._call(super().checkCompactForm, seed)


class ScaledQuasiNewton(CompactQuasiNewton):
    """ParOptScaledQuasiNewton: B = z0 B0 with B0 the wrapped approximation and z0 = z[0], the multiplier of a
    problem's single constraint, taken at every update.  Written on the public methods alone:
    update scales y by 1/z0 into a vector of its own and forwards, mult / multAdd scale by z0, the compact form is
    (z0 b0, sqrt(z0) d, M, Z).  A multiplier z0 <= 0 (which the reference divides by) leaves the previous scaling in
    place; it starts at 1."""

    def __init__(self, problem, qn):
        self.qn = qn
        self.z0 = 1.0
        self._y0 = PVec(problem.ctx, int(problem.nvars))
        super().__init__(problem.ctx, int(problem.nvars), ncon=int(problem.ncon))

    def _take(self, z):
        if z is not None and self.ncon and z[0] > 0.0:
            self.z0 = float(z[0])

    def reset(self):
        self.qn.reset()
        self.z0 = 1.0

    def update(self, x, z, zw, s, y):
        self._take(z)
        self._y0.copyValues(y)
        self._y0.scale(1.0 / self.z0)
        if isinstance(self.qn, CompactQuasiNewton):
            return self.qn.update(x, z, zw, s, self._y0)
        return self.qn.update(s, self._y0)

    def updateMultipliers(self, x, z, zw):
        self._take(z)
        if isinstance(self.qn, CompactQuasiNewton):
            self.qn.updateMultipliers(x, z, zw)

    def mult(self, x, y):
        self.qn.mult(x, y)
        y.scale(self.z0)

    def multAdd(self, alpha, x, y):
        self.qn.multAdd(self.z0 * alpha, x, y)

    def getCompactMat(self):
        b0, d, M, Z = self.qn.getCompactMat()
        return self.z0 * b0, math.sqrt(self.z0) * np.asarray(d), M, Z

    def getMaxLimitedMemorySize(self):
        if isinstance(self.qn, CompactQuasiNewton):
            return self.qn.getMaxLimitedMemorySize()
        v = C.c_int()
        check(lib.po_qn_max_size(self.qn._h, C.byref(v)))
        return v.value

    def setInitDiagonalType(self, t):
        self.qn.setInitDiagonalType(t)


class _QuasiDefBinding:
    """Binds a Python quasi-definite solver -- an object with factor(x, Dinv, Cdiag), apply(bx, bw, yx, yw) (bw may
    be None) and optionally getFactorInfo() -- to a problem handle (po_problem_set_quasidef_callbacks).  Host mode:
    numpy copies in, live host mirrors of yx / yw out.  Device mode: zero-copy tensors under the context's stream.
    device="pvec": the library's vectors themselves as PVec wrappers (valid during the call), for a solver that is
    written on the library's own vector operations.  A Python exception is kept in owner._pending_exc (re-raised by optimize()) and reported as a failed call."""

    def __init__(self, owner, obj, device):
        self.owner, self.obj = owner, obj
        self.pvec = device == "pvec"
        self.device = bool(device) and not self.pvec
        ctx = owner.ctx
        self._info = None
        if self.device:
            import torch

            self._torch = torch
            self._stream = ctx.torch_stream()

        def scope():
            if not self.device:
                return contextlib.nullcontext()
            s, torch = self._stream, self._torch
            cur = torch.cuda.current_stream(s.device)
            if cur.cuda_stream != s.cuda_stream:
                s.wait_stream(cur)
            return torch.cuda.stream(s)

        def vec(h):
            return PVec(ctx, handle=L.po_vec(h), owned=False)

        def arg_in(h):
            if self.pvec:
                return vec(h)
            return vec(h).as_tensor() if self.device else vec(h).to_numpy()

        def guard(fn, failed):
            def _g(*args):
                if getattr(owner, "_pending_exc", None) is not None:
                    return failed
                try:
                    with scope():
                        return fn(*args)
                except BaseException as e:  # noqa: BLE001 - re-raised by the owner's _raise_pending()
                    if getattr(owner, "_pending_exc", None) is None:
                        owner._pending_exc = e
                    return failed
            return _g

        def _factor(user, x, dinv, cdiag):
            return int(obj.factor(arg_in(x), arg_in(dinv), arg_in(cdiag)) or 0)

        def _apply(user, bx, bw, yx, yw):
            abx, abw = arg_in(bx), (arg_in(bw) if bw else None)
            if self.pvec:
                return int(obj.apply(abx, abw, vec(yx), vec(yw)) or 0)
            if self.device:
                return int(obj.apply(abx, abw, vec(yx).as_tensor(), vec(yw).as_tensor()) or 0)
            vx, vw = vec(yx), vec(yw)
            try:
                return int(obj.apply(abx, abw, vx.getArray(), vw.getArray()) or 0)
            finally:
                vx.releaseArray(True)
                vw.releaseArray(True)

        def _info(user):
            text = obj.getFactorInfo()
            if text is None:
                return None
            self._info = C.create_string_buffer(str(text).encode())
            return C.addressof(self._info)

        cb = L.QuasiDefCallbacks()
        self._fns = (L.QD_FACTOR_FN(guard(_factor, 1)), L.QD_APPLY_FN(guard(_apply, 1)),
                     L.QD_INFO_FN(guard(_info, None)) if hasattr(obj, "getFactorInfo") else L.QD_INFO_FN())
        cb.user = None
        cb.factor, cb.apply, cb.factor_info = self._fns
        self._cb = cb
        check(lib.po_problem_set_quasidef_callbacks(owner.handle, C.byref(cb)))


class _QuasiDefMixin:
    """createQuasiDefMat (reference src/ParOptProblem.h:72) for the Python problem classes."""

    _quasidef_device = False
    _quasidef = None

    def setQuasiDefMat(self, obj, device=None):
        """Attach the problem's own quasi-definite solver (None: the library's own again): an object with
        factor(x, Dinv, Cdiag) -> fail, apply(bx, bw, yx, yw) -> fail writing yx / yw in place (bw is None for the
        three-argument form) and optionally getFactorInfo() -> str.  device=True hands it zero-copy torch tensors
        under the context's stream instead of numpy arrays, device="pvec" the library's vectors as PVec wrappers.
        Before the solver is created."""
        if obj is None:
            check(lib.po_problem_set_quasidef_callbacks(self.handle, None))
            self._quasidef = None
            return self
        self._quasidef = _QuasiDefBinding(self, obj, self._quasidef_device if device is None else device)
        return self

    @property
    def sparse_factor(self):
        """The engine that factors the CSR form's S: "rows" or "multifrontal" (po_problem_sparse_factor)."""
        kind = C.c_int()
        check(lib.po_problem_sparse_factor(self.handle, C.byref(kind)))
        return _SPARSE_FACTORS[kind.value]

    @property
    def dense_columns(self):
        """The columns of the CSR sparse Jacobian that are solved by low-rank update, ascending ([] without any)."""
        dc, cnt = L.c_int_p(), C.c_int()
        check(lib.po_problem_sparse_dense_columns(self.handle, C.byref(dc), C.byref(cnt)))
        return [int(dc[i]) for i in range(cnt.value)]

    def getSparseJacobianData(self, device=False):
        """(rowp, cols, data) of the CSR sparse Jacobian (ParOptSparseProblem::getSparseJacobianData): the host
        pattern and the current entries in the order of cols -- a numpy copy, or with device=True a zero-copy
        tensor of the library's device array."""
        rowp, cols = L.c_int_p(), L.c_int_p()
        data, nnz = C.c_void_p(), C.c_int64()
        check(lib.po_problem_get_sparse_jacobian_data(self.handle, C.byref(rowp), C.byref(cols), C.byref(data),
                                                      C.byref(nnz)))
        w, nz = int(self.nwcon), int(nnz.value)
        rp = np.array(np.ctypeslib.as_array(rowp, shape=(w + 1,)), copy=True)
        cl = np.array(np.ctypeslib.as_array(cols, shape=(nz,)), copy=True) if nz else np.zeros(0, dtype=np.intc)
        if device:
            dev = C.c_int()
            check(lib.po_ctx_device(self.ctx.handle, C.byref(dev)))
            return rp, cl, _borrowed_tensor(data.value, nz, dev.value)
        vals = np.zeros(max(nz, 1))
        if nz:
            check(lib.po_ctx_memcpy(self.ctx.handle, vals.ctypes.data, data.value, 8 * nz, 0))
        return rp, cl, vals[:nz]


class Problem(_QuasiDefMixin):
    _quasidef_asked = False
    """Base class for user problems implemented in Python (host arrays through getArray).

    Mirrors paropt.ParOpt.Problem: override getVarsAndBounds(x, lb, ub), evalObjCon(x) ->
    (fail, fobj, con) and evalObjConGradient(x, g, A) -> fail, all on numpy views.  With
    nwcon > 0 (sparse constraints, nwblock = 1) also override evalSparseCon(x, out),
    addSparseJacobian(alpha, x, px, out), addSparseJacobianTranspose(alpha, x, pzw, out) and
    addSparseInnerProduct(alpha, x, cvec, A) (A is the w-sized diagonal; with nwblock > 1 the packed upper
    triangles of the nwblock x nwblock blocks, nwcon (nwblock+1)/2 entries), all in place on numpy views.

    With rowp / cols (the reference's CSR form, paropt/ParOpt.pyx:849-881) override instead
    evalSparseObjCon(x, sparse_cons) -> (fail, fobj, con) and evalSparseObjConGradient(x, g, A, data) -> fail;
    sparse_cons (nwcon) and data (nnz, in the order of cols) are filled in place.  dense_column_rows is the
    dense-column rule of that form (CsrSymbolic; 0 = automatic), `dense_columns` the columns it took out.
    sparse_factor is the engine that factors that form's S: "rows" (default) or "multifrontal"
    (po_problem_set_sparse_factor); `sparse_factor` reads it back.
    """

    def __init__(self, ctx, nvars, ncon, ninequality=-1, nwcon=0, nwinequality=0, use_lower=True,
                 use_upper=True, rowp=None, cols=None, nwblock=1, dense_column_rows=0, sparse_factor="rows"):
        self.ctx = ctx
        self.nvars, self.ncon = int(nvars), int(ncon)
        self.nwcon = int(nwcon)
        self._csr = rowp is not None and cols is not None
        if self._csr and len(rowp) != self.nwcon + 1:
            raise ValueError("rowp is incorrect length")  # paropt/ParOpt.pyx:861-862
        cb = L.ProblemCallbacks()
        self._pending_exc = None

        def _guard(fn):
            # A Python exception must not look like success to the solver: it is kept (the first one), the
            # callback reports failure through its non-zero return code, and optimize() re-raises it.
            def _g(*args):
                if self._pending_exc is not None:
                    return 1  # fail fast until optimize() has re-raised the first exception
                try:
                    with self._callback_scope():
                        return fn(*args)
                except BaseException as e:  # noqa: BLE001 - re-raised by _raise_pending()
                    if self._pending_exc is None:
                        self._pending_exc = e
                    return 1
            return _g

        # argument translation (_arg_in / _arg_out / _finish / _results, below): numpy copies and live host mirrors
        # here, device views in TorchProblem
        @_guard
        def _gvb(user, x, lb, ub):
            out = []
            ax, al, au = (self._arg_out(h, out) for h in (x, lb, ub))
            fail = self.getVarsAndBounds(ax, al, au)
            self._finish(out)
            return int(fail or 0)

        @_guard
        def _eval(user, x, fobj, cons):
            fail, f, con = self.evalObjCon(self._arg_in(x))
            self._results(fobj, cons, f, con)
            return int(fail)

        @_guard
        def _grad(user, x, g, Ac):
            out = []
            ag = self._arg_out(g, out)
            # Ac is NULL when the problem declared linear constraints and only the objective gradient is wanted
            aa = [self._arg_out(Ac[j], out) for j in range(self.ncon)] if Ac else None
            fail = self.evalObjConGradient(self._arg_in(x), ag, aa)
            self._finish(out)
            return int(fail or 0)

        self._cbs = (L.GET_VARS_FN(_gvb), L.EVAL_FN(_eval), L.GRAD_FN(_grad))
        cb.user = None
        cb.get_vars_and_bounds, cb.eval_obj_con, cb.eval_obj_con_gradient = self._cbs
        cb.qn_update_correction = L.QNCORR_FN()
        cb.write_output = L.WRITE_FN()
        self._cb_struct = cb
        self._h = L.po_problem()
        check(lib.po_problem_create_callbacks(ctx.handle, self.nvars, self.ncon, int(ninequality),
                                              C.byref(cb), C.byref(self._h)))
        if not (use_lower and use_upper):
            check(lib.po_problem_set_var_bound_options(self._h, int(bool(use_lower)), int(bool(use_upper))))
        # optional second-order callbacks (use_hvec_product / use_diag_hessian): evalHvecProduct(x, z, zw,
        # px, hvec) and evalHessianDiag(x, z, zw, hdiag) on numpy views, as in paropt.ParOpt
        has_hvec, has_hdiag = hasattr(self, "evalHvecProduct"), hasattr(self, "evalHessianDiag")
        if has_hvec or has_hdiag:
            def _views(x, z, zw):
                xa = self._arg_in(x)
                za = np.array([z[j] for j in range(self.ncon)])  # z stays on the host, as in the reference
                zwa = self._arg_in(zw) if zw else None
                return xa, za, zwa

            @_guard
            def _hvec(user, x, z, zw, px, hvec):
                xa, za, zwa = _views(x, z, zw)
                out = []
                ah = self._arg_out(hvec, out)
                fail = self.evalHvecProduct(xa, za, zwa, self._arg_in(px), ah)
                self._finish(out)
                return int(fail or 0)

            @_guard
            def _hdiag(user, x, z, zw, hdiag):
                xa, za, zwa = _views(x, z, zw)
                out = []
                ah = self._arg_out(hdiag, out)
                fail = self.evalHessianDiag(xa, za, zwa, ah)
                self._finish(out)
                return int(fail or 0)

            self._hcbs = (L.HVEC_FN(_hvec) if has_hvec else L.HVEC_FN(), L.HDIAG_FN(_hdiag) if has_hdiag else L.HDIAG_FN())
            check(lib.po_problem_set_hessian_callbacks(self._h, self._hcbs[0], self._hcbs[1]))
        if self._csr:
            self._rowp = np.ascontiguousarray(rowp, dtype=np.intc)
            self._cols = np.ascontiguousarray(cols, dtype=np.intc)
            nnz = int(self._rowp[-1])
            if len(self._cols) != nnz:
                raise ValueError("cols is incorrect length")
            self._data_host = None

            @_guard
            def _sobjcon(user, x, fobj, cons, sparse):
                out = []
                asp = self._arg_out(sparse, out)
                fail, f, con = self.evalSparseObjCon(self._arg_in(x), asp)
                self._finish(out)
                self._results(fobj, cons, f, con)
                return int(fail or 0)

            @_guard
            def _sgrad(user, x, g, Ac, data, nnz_):
                out = []
                ag = self._arg_out(g, out)
                aa = [self._arg_out(Ac[j], out) for j in range(self.ncon)]
                fail = self.evalSparseObjConGradient(self._arg_in(x), ag, aa, self._csr_values(data, nnz))
                self._finish(out)
                self._csr_values_done(data, nnz)
                return int(fail or 0)

            self._csr_cbs = (L.SPARSE_OBJCON_FN(_sobjcon), L.SPARSE_GRAD_FN(_sgrad))
            if dense_column_rows != 0:
                check(lib.po_problem_set_sparse_dense_columns(self._h, int(dense_column_rows)))
            if sparse_factor != "rows":
                check(lib.po_problem_set_sparse_factor(self._h, _sparse_factor_kind(sparse_factor)))
            check(lib.po_problem_set_sparse_jacobian_data(
                self._h, self.nwcon, int(nwinequality), self._rowp.ctypes.data_as(L.c_int_p),
                self._cols.ctypes.data_as(L.c_int_p), self._csr_cbs[0], self._csr_cbs[1]))
        elif self.nwcon > 0:
            def _wrap(method):
                @_guard
                def _f(user, alpha, x, v, out):
                    done = []
                    ao = self._arg_out(out, done)
                    fail = method(float(alpha), self._arg_in(x), self._arg_in(v), ao)
                    self._finish(done)
                    return int(fail or 0)
                return _f

            @_guard
            def _wcon(user, x, out):
                done = []
                ao = self._arg_out(out, done)
                fail = self.evalSparseCon(self._arg_in(x), ao)
                self._finish(done)
                return int(fail or 0)

            scb = L.ProblemSparseCallbacks()
            self._scbs = (L.SPARSE_CON_FN(_wcon), L.SPARSE_JAC_FN(_wrap(self.addSparseJacobian)),
                          L.SPARSE_JAC_FN(_wrap(self.addSparseJacobianTranspose)),
                          L.SPARSE_JAC_FN(_wrap(self.addSparseInnerProduct)))
            (scb.eval_sparse_con, scb.add_sparse_jacobian, scb.add_sparse_jacobian_transpose,
             scb.add_sparse_inner_product) = self._scbs
            self._scb_struct = scb
            check(lib.po_problem_set_sparse_callbacks(self._h, self.nwcon, int(nwinequality), C.byref(scb)))
            if int(nwblock) > 1:  # addSparseInnerProduct then fills packed upper nwblock x nwblock blocks
                check(lib.po_problem_set_sparse_block_size(self._h, int(nwblock)))
        self._quasidef_asked = False

    def createQuasiDefMat(self):
        """Override to bring the problem's own quasi-definite solver (see setQuasiDefMat); None: the library's.
        Asked for once, when a solver first takes the problem's handle (as the reference asks when the optimizer is
        created), so the subclass's own __init__ has run by then."""
        return None

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                lib.po_problem_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- argument translation of the callbacks: numpy copies in, live host mirrors out ------------------------------
    def _callback_scope(self):
        return contextlib.nullcontext()

    def _arg_in(self, h):
        """A vector the callback reads (x, px, zw, ...)."""
        return PVec(self.ctx, handle=L.po_vec(h), owned=False).to_numpy()

    def _arg_out(self, h, out):
        """A vector the callback writes: its live host mirror, ended by _finish(out) after the callback."""
        v = PVec(self.ctx, handle=L.po_vec(h), owned=False)
        out.append(v)
        return v.getArray()

    def _finish(self, out):
        for v in out:
            v.releaseArray(True)

    def _results(self, fobj, cons, f, con):
        """(fobj, con) of evalObjCon / evalSparseObjCon into the solver's result pointers."""
        fobj[0] = float(f)
        for j in range(self.ncon):
            cons[j] = float(con[j])

    def _csr_values(self, data, nnz):
        """The `data` argument of evalSparseObjConGradient: a host buffer, copied to the device afterwards."""
        if self._data_host is None:
            self._data_host = np.zeros(max(nnz, 1))
        return self._data_host[:nnz]

    def _csr_values_done(self, data, nnz):
        check(lib.po_ctx_memcpy(self.ctx.handle, data, self._data_host.ctypes.data, 8 * nnz, 1))

    def _raise_pending(self):
        """Re-raise the first exception a callback threw during the last solver call."""
        e, self._pending_exc = self._pending_exc, None
        if e is not None:
            raise e

    def setLinearConstraints(self, flag=True):
        """Declare the dense constraints linear: after the first gradient evaluation of an optimize() call
        evalObjConGradient is called with A = None (objective gradient only)."""
        check(lib.po_problem_set_linear_constraints(self._h, int(bool(flag))))
        return self

    @property
    def handle(self):
        if not self._quasidef_asked:
            self._quasidef_asked = True
            qd = self.createQuasiDefMat()
            if qd is not None and self._quasidef is None:  # (an explicit setQuasiDefMat() made earlier stands)
                self.setQuasiDefMat(qd)
        return self._h


class TorchProblem(Problem):
    """A user problem in Python whose callbacks work on device tensors (torch): the constructor and the method names
    of Problem, but every n- or w-sized argument is a zero-copy view of the library's vector (PVec.as_tensor), to be
    written in place (x[:] = ..., g.copy_(...)).  No host mirror is ever made and nothing is copied between the
    library's kernels and the user's.

    - Callbacks run under torch.cuda.stream(ctx.torch_stream()); the library stream first waits (an event, not a host
      synchronisation) for the torch stream that was current, so data prepared there beforehand is complete.
    - evalObjCon / evalSparseObjCon return (fail, fobj, con) either as host numbers (the final global values, as in
      Problem) or as float64 tensors on the device (fobj 0-d, con of length ncon): this rank's part, summed over the
      ranks by the library (po_ctx_reduce_device) into the solver's results.  The tensors are kept until the
      reduction has consumed them.
    - A of evalObjConGradient is a list of ncon views (None after setLinearConstraints); z of evalHvecProduct /
      evalHessianDiag stays a host numpy array, zw is a view; data of evalSparseObjConGradient is a view of the
      library's device array of Jacobian values (valid during the callback).
    - setDeferredReductions(True): the results are device tensors and the callbacks never read a library reduction
      on the host, so the solver may reduce them together with its own (po_problem_set_deferred_reductions).
    """

    def __init__(self, ctx, nvars, ncon, ninequality=-1, nwcon=0, nwinequality=0, use_lower=True,
                 use_upper=True, rowp=None, cols=None, nwblock=1, dense_column_rows=0, sparse_factor="rows"):
        import collections

        import torch

        self._torch = torch
        self._stream = ctx.torch_stream()
        self._device = self._stream.device
        self._held = collections.deque()  # device results until their reduction has consumed them
        self._drop_cb = L.AFTER_REDUCE_FN(self._drop_held)
        self._data_view = None
        super().__init__(ctx, nvars, ncon, ninequality, nwcon=nwcon, nwinequality=nwinequality, use_lower=use_lower,
                         use_upper=use_upper, rowp=rowp, cols=cols, nwblock=nwblock,
                         dense_column_rows=dense_column_rows, sparse_factor=sparse_factor)

    _quasidef_device = True  # createQuasiDefMat's solver works on device tensors too

    def setDeferredReductions(self, flag=True):
        check(lib.po_problem_set_deferred_reductions(self._h, int(bool(flag))))
        return self

    # -- argument translation: device views ------------------------------------------------------------------------
    def _callback_scope(self):
        s = self._stream
        cur = self._torch.cuda.current_stream(self._device)
        if cur.cuda_stream != s.cuda_stream:
            s.wait_stream(cur)
        return self._torch.cuda.stream(s)

    def _arg_in(self, h):
        return PVec(self.ctx, handle=L.po_vec(h), owned=False).as_tensor()

    def _arg_out(self, h, out):
        return PVec(self.ctx, handle=L.po_vec(h), owned=False).as_tensor()

    def _finish(self, out):
        pass

    def _results(self, fobj, cons, f, con):
        torch = self._torch
        if not (isinstance(f, torch.Tensor) or isinstance(con, torch.Tensor)):
            return super()._results(fobj, cons, f, con)
        ft = self._device_result(f, 1, "fobj")
        ct = self._device_result(con, self.ncon, "con") if self.ncon > 0 else None
        self._held.append((ft, ct))
        check(lib.po_ctx_reduce_device(self.ctx.handle, ft.data_ptr(), 1, 0, fobj))
        if ct is not None:
            check(lib.po_ctx_reduce_device(self.ctx.handle, ct.data_ptr(), self.ncon, 0, cons))
        check(lib.po_ctx_after_reduce(self.ctx.handle, C.cast(self._drop_cb, C.c_void_p), None))

    def _device_result(self, t, n, what):
        torch = self._torch
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self._device
                and t.numel() == n and t.dim() == (0 if what == "fobj" else 1) and t.is_contiguous()):
            raise TypeError("TorchProblem: %s must be a contiguous float64 tensor on %s with %s when the results are "
                            "tensors (got %r)" % (what, self._device, "0 dimensions" if what == "fobj" else
                                                  "%d entries" % n, t if not isinstance(t, torch.Tensor) else
                                                  (t.dtype, t.device, tuple(t.shape))))
        return t

    def _drop_held(self, user):
        if self._held:
            self._held.popleft()

    def _csr_values(self, data, nnz):
        if self._data_view is None or self._data_view[0] != data:
            self._data_view = (data, _borrowed_tensor(data, nnz, self._device.index))
        return self._data_view[1]

    def _csr_values_done(self, data, nnz):
        pass


class SeparableProblem(_QuasiDefMixin):
    """Built-in device-resident workloads: 'quadratic', 'convex', 'rosenbrock'."""

    KINDS = {"quadratic": 0, "convex": 1, "rosenbrock": 2}
    _pending_exc = None

    def _raise_pending(self):
        """Re-raise the first exception an attached quasi-definite solver threw during the last solver call."""
        e, self._pending_exc = self._pending_exc, None
        if e is not None:
            raise e

    def __init__(self, ctx, kind, n, c=2, seed=0, eig_min=1.0, eig_max=100.0):
        self.ctx = ctx
        self._h = L.po_problem()
        check(lib.po_problem_create_separable(ctx.handle, self.KINDS[kind], int(n), int(c), int(seed),
                                              float(eig_min), float(eig_max), C.byref(self._h)))
        nl, off, nc = C.c_int64(), C.c_int64(), C.c_int()
        check(lib.po_problem_sizes(self._h, C.byref(nl), C.byref(off), C.byref(nc)))
        self.nvars, self.offset, self.ncon = nl.value, off.value, nc.value
        self.nwcon = 0

    def setWeighting(self, nwcon, nw, nwstart=0, nwskip=0, nwinequality=None):
        """cw_i = 1 - sum_{k<nw} x[nwstart + i (nw + nwskip) + k], i < nwcon (global indices);
        the first nwinequality of them are inequalities (all by default)."""
        if nwinequality is None:
            nwinequality = nwcon
        check(lib.po_problem_set_weighting(self._h, int(nwcon), int(nw), int(nwstart), int(nwskip),
                                           int(nwinequality)))
        a, b = C.c_int64(), C.c_int64()
        check(lib.po_problem_sparse_sizes(self._h, C.byref(a), C.byref(b)))
        self.nwcon = a.value
        return self

    def setChain(self, span=2, stride=1, reverse_cols=False, dense_vars=0, dense_column_rows=0, sparse_factor="rows"):
        """Rank-local overlapping sparse constraints in CSR form: cw_i = 1 - sum_{k<span} x[i*stride+k]^2 >= 0
        (examples/rosenbrock/sparse_rosenbrock.cpp is span 2, stride 1).  dense_vars > 0: the chain runs over the
        first variables and the last dense_vars local ones enter every row, cw_i -= sum_j x[n - dense_vars + j]^2;
        dense_column_rows is the dense-column rule their columns fall under, sparse_factor the engine that factors
        S, "rows" or "multifrontal" (Problem)."""
        if dense_column_rows != 0:
            check(lib.po_problem_set_sparse_dense_columns(self._h, int(dense_column_rows)))
        if sparse_factor != "rows":
            check(lib.po_problem_set_sparse_factor(self._h, _sparse_factor_kind(sparse_factor)))
        if dense_vars:
            check(lib.po_problem_set_chain_dense(self._h, int(span), int(stride), int(bool(reverse_cols)),
                                                 int(dense_vars)))
        else:
            check(lib.po_problem_set_chain(self._h, int(span), int(stride), int(bool(reverse_cols))))
        a, b = C.c_int64(), C.c_int64()
        check(lib.po_problem_sparse_sizes(self._h, C.byref(a), C.byref(b)))
        self.nwcon = a.value
        return self

    def setVarBoundOptions(self, use_lower=True, use_upper=True):
        check(lib.po_problem_set_var_bound_options(self._h, int(bool(use_lower)), int(bool(use_upper))))
        return self

    def setBoundsMode(self, mode):
        """Deliberately broken bounds for the bound-repair tests (po_problem_set_bounds_mode)."""
        check(lib.po_problem_set_bounds_mode(self._h, int(mode)))
        return self

    def setLinearConstraints(self, flag=True):
        """The dense constraints are linear: the solver keeps the Jacobian of the first gradient evaluation
        of each optimize() and asks for the objective gradient only afterwards (po_problem_set_linear_constraints)."""
        check(lib.po_problem_set_linear_constraints(self._h, int(bool(flag))))
        return self

    @property
    def handle(self):
        return self._h

    def evalObjCon(self, x):
        f = C.c_double()
        con = np.zeros(max(self.ncon, 1))
        check(lib.po_problem_eval_obj_con(self._h, x.handle, C.byref(f), con.ctypes.data_as(L.c_double_p)))
        return 0, f.value, con[: self.ncon]

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                lib.po_problem_destroy(self._h)
        except Exception:
            pass


class UserLibraryProblem:
    """A ParOptProblem subclass that lives in a USER'S shared library built on include/ParOptAMD.hpp (e.g.
    examples/librandom_convex_user.so): the library hands over the `po_problem` of its facade object, the solver
    classes of this module drive it like any other problem.  Entry points expected from the library (extern "C"):
    <prefix>_problem_create(ctx, nglobal, ncon, seed) -> void*, <prefix>_problem_handle(void*) -> po_problem,
    <prefix>_problem_sizes(void*, int64*, int64*), <prefix>_problem_destroy(void*), and optionally
    <prefix>_problem_set_linear_constraints / _set_deferred_reductions(void*, int), _own_kernel_bytes(void*, int)."""

    def __init__(self, ctx, path, nglobal, ncon, seed=0, prefix="rc", nwcon=0, nw=0):
        """nwcon > 0: <prefix>_problem_create_weighting(ctx, nglobal, ncon, seed, nwcon, nw) instead (a problem with one
        sparse constraint per group of nw consecutive variables, examples/weighting_amd.cpp)."""
        self.ctx = ctx
        self._lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        f = lambda name: getattr(self._lib, "%s_problem_%s" % (prefix, name))
        f("create").restype = C.c_void_p
        f("create").argtypes = [L.po_ctx, C.c_int64, C.c_int, C.c_uint64]
        f("handle").restype = L.po_problem
        f("handle").argtypes = [C.c_void_p]
        f("sizes").argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        f("destroy").argtypes = [C.c_void_p]
        self._f = f
        if nwcon > 0:
            f("create_weighting").restype = C.c_void_p
            f("create_weighting").argtypes = [L.po_ctx, C.c_int64, C.c_int, C.c_uint64, C.c_int64, C.c_int]
            self._obj = C.c_void_p(f("create_weighting")(ctx.handle, int(nglobal), int(ncon), int(seed), int(nwcon),
                                                         int(nw)))
        else:
            self._obj = C.c_void_p(f("create")(ctx.handle, int(nglobal), int(ncon), int(seed)))
        if not self._obj:
            raise L.ParOptAMDError(-1, "user library failed to create its problem")
        self._h = L.po_problem(f("handle")(self._obj))
        nl, off = C.c_int64(), C.c_int64()
        f("sizes")(self._obj, C.byref(nl), C.byref(off))
        self.nvars, self.offset, self.ncon, self.nwcon = nl.value, off.value, int(ncon), int(nwcon)

    @property
    def handle(self):
        return self._h

    def setLinearConstraints(self, flag=True):
        fn = self._f("set_linear_constraints")
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(self._obj, int(bool(flag)))
        return self

    def setDeferredReductions(self, flag=True):
        fn = self._f("set_deferred_reductions")
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(self._obj, int(bool(flag)))
        return self

    def ownKernelBytes(self, jacobian_rewritten=True):
        """Algorithmic HBM bytes of the user's own kernels so far (the library cannot count them)."""
        fn = self._f("own_kernel_bytes")
        fn.restype = C.c_double
        fn.argtypes = [C.c_void_p, C.c_int]
        return fn(self._obj, int(bool(jacobian_rewritten)))

    def close(self):
        if self._obj:
            self._f("destroy")(self._obj)
            self._obj = None
            self._h = None

    def __del__(self):
        try:
            if self.ctx._h:
                self.close()
        except Exception:
            pass


_SPARSE_FACTORS = ("rows", "multifrontal")  # PO_SPARSE_FACTOR_ROWS, PO_SPARSE_FACTOR_MULTIFRONTAL


def _sparse_factor_kind(name):
    if name not in _SPARSE_FACTORS:
        raise ValueError("sparse_factor must be one of %s, not %r" % (", ".join(_SPARSE_FACTORS), name))
    return _SPARSE_FACTORS.index(name)


class CsrSymbolic:
    """The one-time host analysis of a CSR sparse Jacobian pattern (no device needed): ordering,
    elimination tree, pattern of the Cholesky factor of S = C + Aw D^-1 Aw^T, dependency level sets."""

    def __init__(self, nvars, rowp, cols, dense_column_rows=0, sparse_factor="rows"):
        """dense_column_rows: the dense-column rule (> 0: columns with at least that many entries leave S and come
        back as a low-rank correction; 0: automatic, only where the pattern would otherwise be refused; -1: never).
        With dense columns (`dense_cols`, ascending) every other field describes S0 = C + As D^-1 As^T.

        sparse_factor="multifrontal": the analysis for the multifrontal engine.  The fields are then those of
        SparseCholesky (num_snodes, nnzL, nlevels, max_snode, max_front, work_bytes, block, perm, snode_first,
        snode_parent, snode_level) plus nnz / nnzS, the assembly table ent_a, ent_b, ent_dst (one entry of lower(S0)
        each, its offset in the engine's L) and frontal_scatter(); the row factor's fields do not exist."""
        rowp = np.ascontiguousarray(rowp, dtype=np.intc)
        cols = np.ascontiguousarray(cols, dtype=np.intc)
        w = len(rowp) - 1
        h = L.po_csr_symbolic()
        self.sparse_factor = sparse_factor
        check(lib.po_csr_symbolic_create_factor(int(nvars), w, rowp.ctypes.data_as(L.c_int_p),
                                                cols.ctypes.data_as(L.c_int_p), int(dense_column_rows),
                                                _sparse_factor_kind(sparse_factor), C.byref(h)))
        self._h = h
        try:
            dc, cnt = L.c_int_p(), C.c_int()
            check(lib.po_csr_symbolic_dense_columns(h, C.byref(dc), C.byref(cnt)))
            self.dense_cols = [int(dc[i]) for i in range(cnt.value)]
            if sparse_factor == "multifrontal":
                self._frontal(w, len(cols))
                return
            info = (C.c_int64 * 7)()
            check(lib.po_csr_symbolic_info(h, info))
            self.nnz, self.nnzS, self.nnzL, self.nlevels = (int(v) for v in info[:4])
            self.sorted_input = bool(info[4])
            self.nfronts, self.max_front = int(info[5]), int(info[6])
            ptrs = [L.c_int_p() for _ in range(6)]
            check(lib.po_csr_symbolic_arrays(h, *[C.byref(p) for p in ptrs]))

            def arr(p, n):
                return np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=np.intc)

            self.perm, self.parent = arr(ptrs[0], w), arr(ptrs[1], w)
            self.Lrowp, self.Lcols = arr(ptrs[2], w + 1), arr(ptrs[3], self.nnzL)
            self.level_ptr = arr(ptrs[4], self.nlevels + 1)
            self.front_of = arr(ptrs[5], w)
        except Exception:
            self.close()
            raise

    def _frontal(self, w, nnz):
        h = self._h
        info = (C.c_int64 * 8)()
        check(lib.po_csr_symbolic_frontal_info(h, info))
        (self.size, self.num_snodes, self.nnzL, self.nlevels, self.max_snode, self.max_front, self.work_bytes,
         self.block) = (int(v) for v in info)
        ptrs = [L.c_int_p() for _ in range(6)]
        dst, cnt = L.c_i64_p(), C.c_int64()
        check(lib.po_csr_symbolic_frontal_arrays(h, *[C.byref(p) for p in ptrs], C.byref(dst), C.byref(cnt)))

        def arr(p, n, dtype=np.intc):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=dtype)

        ns, ne = self.num_snodes, cnt.value
        self.perm, self.snode_first = arr(ptrs[0], w), arr(ptrs[1], ns + 1)
        self.snode_parent, self.snode_level = arr(ptrs[2], ns), arr(ptrs[3], ns)
        self.ent_a, self.ent_b, self.ent_dst = arr(ptrs[4], ne), arr(ptrs[5], ne), arr(dst, ne, np.int64)
        self.nnz, self.nnzS = nnz, ne

    def frontal_scatter(self):
        """The engine's own value scatter of lower(S0) (multifrontal analysis only): (colp, rows, asm_ptr, asm_src,
        asm_dst, l_size) -- destination d at offset asm_dst[d] of the l_size doubles of L sums the entries
        asm_src[asm_ptr[d]:asm_ptr[d+1]] of the pattern (colp, rows)."""
        ptrs = [L.c_int_p() for _ in range(4)]
        dst, cnt, lsize = L.c_i64_p(), C.c_int64(), C.c_int64()
        check(lib.po_csr_symbolic_frontal_scatter(self._h, *[C.byref(p) for p in ptrs], C.byref(dst), C.byref(cnt),
                                                  C.byref(lsize)))

        def arr(p, n, dtype=np.intc):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=dtype)

        w, nd = len(self.perm), cnt.value
        colp = arr(ptrs[0], w + 1)
        ne = int(colp[-1])
        return (colp, arr(ptrs[1], ne), arr(ptrs[2], nd + 1), arr(ptrs[3], ne), arr(dst, nd, np.int64),
                int(lsize.value))

    def kernel_forms(self, nv=1):
        """The kernel forms the device factorization and the two triangular sweeps launch on this pattern for a panel
        of nv right-hand sides: {form name: number of elimination levels that launch it}, every name the solver knows
        (a form no level uses maps to 0).  It is the function the solver itself launches by; no device needed."""
        cnt, names, levels = C.c_int(), C.POINTER(C.c_char_p)(), L.c_int_p()
        check(lib.po_csr_symbolic_kernel_forms(self._h, int(nv), C.byref(cnt), C.byref(names), C.byref(levels)))
        return {names[f].decode(): int(levels[f]) for f in range(cnt.value)}

    def frontal_packing(self):
        """SparseCholesky.packing() for the factor of a multifrontal analysis."""
        return _chol_packing(lib.po_csr_symbolic_frontal_packing, self._h, lambda: self.num_snodes)

    def frontal_kernel_forms(self, nv=1):
        """SparseCholesky.kernel_forms() for the factor of a multifrontal analysis."""
        return _chol_kernel_forms(lib.po_csr_symbolic_frontal_kernel_forms, self._h, nv)

    def close(self):
        if self._h:
            lib.po_csr_symbolic_destroy(self._h)
            self._h = L.po_csr_symbolic()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


def _chol_packing(fn, h, num_snodes):
    info = (C.c_int64 * 4)()
    ptrs = [L.c_int_p() for _ in range(4)]
    upd = L.c_i64_p()
    check(fn(h, info, *[C.byref(p) for p in ptrs], C.byref(upd)))

    def arr(p, n, dtype=np.intc):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=dtype)

    ng, num_snodes = int(info[2]), num_snodes()  # (asked for after the call: a handle without fronts was refused)
    return {"tiny": int(info[0]), "cap": int(info[1]), "num_groups": ng, "factor_levels": int(info[3]),
            "group_first": arr(ptrs[0], ng), "group_root": arr(ptrs[1], ng), "group_level": arr(ptrs[2], ng),
            "front_order": arr(ptrs[3], num_snodes), "upd_off": arr(upd, num_snodes, np.int64)}


def _chol_kernel_forms(fn, h, nv):
    cnt, names, levels = C.c_int(), C.POINTER(C.c_char_p)(), L.c_int_p()
    check(fn(h, int(nv), C.byref(cnt), C.byref(names), C.byref(levels)))
    return {names[f].decode(): int(levels[f]) for f in range(cnt.value)}


class SparseCholesky:
    """ParOptSparseCholesky (src/ParOptSparseCholesky.h:29-47): L L^T = P A P^T of an SPD matrix given by its full
    symmetric pattern in compressed columns, as a multifrontal factorization with dense fronts on the device.

    ctx=None gives an analysis-only object (no device).  order: "nd" (nested dissection), "amd" (accepted, gets the
    same nested dissection), "natural" (the identity, or `perm` with perm[new] = old).

    factorization: "llt" (Cholesky, the default) or "ldlt": L S L^T = P A P^T with S = diag(+-1) and NO pivoting, for
    symmetric quasi-definite matrices ([[E, B^T], [B, -F]] with E, F SPD), which have it under every permutation.  For
    a general indefinite matrix it is only as good as its pivots.

    keep_matrix=True retains A beside the factor (see set_keep_matrix): matvec() and solve_refined() need it.

    schur=<indices> (distinct unknowns, any order) makes the factorization PARTIAL: the set is ordered last, in the
    order given, and left uneliminated, so after factor() the device holds S = A22 - A21 A11^-1 A12 (schur(),
    schur_device()).  The ordering type then applies to the interior unknowns; "natural" with perm needs a perm that
    ends with the set.  solve() and solve_refined() raise on such an object: the solve is condense(), the caller's own
    solve with S, expand() -- until factor_schur() has factored S (plus an optional add) on the device: then
    schur_solve() solves with it and solve() / solve_refined() run the whole solve.  inertia() counts the interior
    pivots only, schur_inertia() those of S."""

    ORDERS = {"natural": 0, "amd": 1, "nd": 2}
    FACTORIZATIONS = {"llt": 0, "ldlt": 1}

    def __init__(self, ctx, size, colp, rows, order="nd", perm=None, factorization="llt", keep_matrix=False,
                 schur=None):
        self.ctx = ctx
        self._colp = np.ascontiguousarray(colp, dtype=np.intc)
        self._rows = np.ascontiguousarray(rows, dtype=np.intc)
        self._h = L.po_sparse_chol()
        p = None
        if perm is not None:
            p = np.ascontiguousarray(perm, dtype=np.intc)
            if p.shape != (int(size),):
                raise ValueError("perm must have `size` entries")
        if self._colp.shape != (int(size) + 1,) and int(size) >= 0:
            raise ValueError("colp must have size + 1 entries")
        if int(size) >= 0 and len(self._rows) < int(self._colp[-1]):
            raise ValueError("rows is shorter than colp[size]")
        args = (ctx.handle if ctx is not None else None, int(size), self._colp.ctypes.data_as(L.c_int_p),
                self._rows.ctypes.data_as(L.c_int_p), self.ORDERS[order] if isinstance(order, str) else int(order),
                p.ctypes.data_as(L.c_int_p) if p is not None else None)
        if schur is None:
            check(lib.po_sparse_chol_create(*args, C.byref(self._h)))
        else:
            sc = np.ascontiguousarray(schur, dtype=np.intc)
            if sc.ndim != 1:
                raise ValueError("schur must be a list of indices")
            check(lib.po_sparse_chol_create_schur(*args, len(sc), sc.ctypes.data_as(L.c_int_p), C.byref(self._h)))
        info = (C.c_int64 * 8)()
        check(lib.po_sparse_chol_info(self._h, info))
        (self.size, self.num_snodes, self.nnzL, self.nlevels, self.max_snode, self.max_front, self.work_bytes,
         self.block_width) = (int(v) for v in info)
        ptrs = [L.c_int_p() for _ in range(4)]
        check(lib.po_sparse_chol_arrays(self._h, *[C.byref(q) for q in ptrs]))

        def arr(q, n):
            return np.ctypeslib.as_array(q, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=np.intc)

        self.perm = arr(ptrs[0], self.size)
        self.snode_first = arr(ptrs[1], self.num_snodes + 1)
        self.snode_parent = arr(ptrs[2], self.num_snodes)
        self.snode_level = arr(ptrs[3], self.num_snodes)
        sinfo = self.schur_info()
        self.num_schur = sinfo["num_schur"]
        q = L.c_int_p()
        check(lib.po_sparse_chol_schur_indices(self._h, C.byref(q)))
        self.schur_indices = arr(q, self.num_schur)
        if factorization != "llt":
            self.set_factorization(factorization)
        if keep_matrix:
            self.set_keep_matrix(True)

    @property
    def handle(self):
        return self._h

    # ---- Schur complement (po_sparse_chol_create_schur and what follows it) ----
    def schur_info(self):
        """{"num_schur", "snode" (index of the Schur supernode, -1 without a set), "children" (its fan-in),
        "gather_entries" (entries of the factorization's gather table)}; no device needed."""
        info = (C.c_int64 * 4)()
        check(lib.po_sparse_chol_schur_info(self._h, info))
        return {"num_schur": int(info[0]), "snode": int(info[1]), "children": int(info[2]),
                "gather_entries": int(info[3])}

    def schur(self):
        """S = A22 - A21 A11^-1 A12 as a (num_schur, num_schur) array in the order of the set as given, exactly
        symmetric; valid after factor() until the next set_values."""
        ns = self.num_schur
        S = np.zeros((ns, ns), dtype=np.float64, order="F")
        check(lib.po_sparse_chol_get_schur(self._h, S.ctypes.data_as(L.c_double_p), max(ns, 1)))
        return S

    def schur_device(self, ptr, lds):
        """S written to device memory at `ptr` (an address, or a contiguous float64 torch tensor on the context's
        device), column-major with leading dimension lds >= num_schur; queued on the context's stream."""
        if not isinstance(ptr, int):
            ptr = self._tensor_ptr(ptr, (self.num_schur - 1) * int(lds) + self.num_schur, "schur_device")
        check(lib.po_sparse_chol_get_schur_device(self._h, ptr, int(lds)))
        self.ctx.synchronize()

    def _half(self, fn, who, x):
        x = np.array(x, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (1, 2) or x.shape[-1] != self.size:
            raise ValueError(who + ": x must have shape (n,) or (nrhs, n)")
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        check(fn(self._h, x.ctypes.data_as(L.c_double_p), nrhs, self.size))
        return x

    def _half_tensor(self, fn, who, t):
        if t.dim() not in (1, 2) or t.shape[-1] != self.size:
            raise ValueError(who + ": t must have shape (n,) or (nrhs, n)")
        nrhs = 1 if t.dim() == 1 else t.shape[0]
        ptr = self._tensor_ptr(t, nrhs * self.size, who)
        check(fn(self._h, ptr, nrhs, self.size))
        self.ctx.synchronize()
        return t

    def condense(self, b):
        """First half of the solve for b of shape (n,) or (nrhs, n); returns a new array whose Schur entries hold
        g = b2 - A21 A11^-1 b1 (the right-hand side of S x2 = g).  Its interior entries are an opaque intermediate:
        pass them unchanged to expand()."""
        return self._half(lib.po_sparse_chol_solve_condense, "condense", b)

    def expand(self, x):
        """Second half: x is what condense() returned with x2 written over the Schur entries; returns the solution of
        A x = b (a new array).  With x2 = 0 its interior entries are A11^-1 b1."""
        return self._half(lib.po_sparse_chol_solve_expand, "expand", x)

    def condense_tensor(self, t):
        """condense() in place on a contiguous float64 torch tensor of shape (n,) or (nrhs, n) on the device."""
        return self._half_tensor(lib.po_sparse_chol_solve_condense_device, "condense_tensor", t)

    def expand_tensor(self, t):
        """expand() in place on a contiguous float64 torch tensor of shape (n,) or (nrhs, n) on the device."""
        return self._half_tensor(lib.po_sparse_chol_solve_expand_device, "expand_tensor", t)

    # ---- factored Schur complement (po_sparse_chol_schur_factor and what follows it) ----
    def factor_schur(self, add=None):
        """Factor S~ = S + add on the device, in a buffer of its own and in the kind of the factor() that produced S;
        valid after factor() until the next set_values.  add: None, or a symmetric (num_schur, num_schur) array in the
        order of the set (its lower triangle is read).  Returns 0, or 1 + the permuted index size - num_schur + k of
        the first pivot replaced.  schur() is untouched, and factor_schur may be called again with another add.
        Afterwards solve() / solve_tensor() work on this object, solve_refined() too when add is None."""
        info = C.c_int()
        if add is None:
            check(lib.po_sparse_chol_schur_factor(self._h, None, 0, C.byref(info)))
            return info.value
        ns = self.num_schur
        a = np.asfortranarray(add, dtype=np.float64)
        if a.shape != (ns, ns):
            raise ValueError("factor_schur: add must have shape (num_schur, num_schur)")
        check(lib.po_sparse_chol_schur_factor(self._h, a.ctypes.data_as(L.c_double_p), max(ns, 1), C.byref(info)))
        return info.value

    def factor_schur_tensor(self, add=None):
        """factor_schur with add a contiguous float64 torch tensor of shape (num_schur, num_schur) on the context's
        device (symmetric: rows and columns are interchangeable), or None."""
        info = C.c_int()
        ns = self.num_schur
        ptr = None
        if add is not None:
            if add.dim() != 2 or tuple(add.shape) != (ns, ns):
                raise ValueError("factor_schur_tensor: add must have shape (num_schur, num_schur)")
            ptr = self._tensor_ptr(add, ns * ns, "factor_schur_tensor")
        check(lib.po_sparse_chol_schur_factor_device(self._h, ptr, max(ns, 1), C.byref(info)))
        return info.value

    def schur_solve(self, g):
        """x2 = S~^-1 g for g of shape (num_schur,) or (nrhs, num_schur), the order of the set; returns a new array."""
        x = np.array(g, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (1, 2) or x.shape[-1] != self.num_schur:
            raise ValueError("schur_solve: g must have shape (num_schur,) or (nrhs, num_schur)")
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        check(lib.po_sparse_chol_schur_solve(self._h, x.ctypes.data_as(L.c_double_p), nrhs, self.num_schur))
        return x

    def schur_solve_tensor(self, t):
        """schur_solve in place on a contiguous float64 torch tensor of shape (num_schur,) or (nrhs, num_schur) on the
        context's device."""
        if t.dim() not in (1, 2) or t.shape[-1] != self.num_schur:
            raise ValueError("schur_solve_tensor: t must have shape (num_schur,) or (nrhs, num_schur)")
        nrhs = 1 if t.dim() == 1 else t.shape[0]
        ptr = self._tensor_ptr(t, nrhs * self.num_schur, "schur_solve_tensor")
        check(lib.po_sparse_chol_schur_solve_device(self._h, ptr, nrhs, self.num_schur))
        self.ctx.synchronize()
        return t

    def schur_inertia(self):
        """(positive, negative, replaced) pivots of the last factor_schur(); they sum to num_schur.  The "llt" rule of
        inertia(): (num_schur, 0, 0), or an error after a factorization that replaced pivots."""
        out = (C.c_int64 * 3)()
        check(lib.po_sparse_chol_schur_inertia(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def schur_solve_info(self):
        """{"panel_width" (W of the dense sweeps), "launches" (of one forward and one backward dense sweep over one
        slab), "factor_bytes" (of the buffer of the factored S~, 0 before the first factor_schur), "factored"}; the
        first two need no device."""
        info = (C.c_int64 * 4)()
        check(lib.po_sparse_chol_schur_solve_info(self._h, info))
        return {"panel_width": int(info[0]), "launches": int(info[1]), "factor_bytes": int(info[2]),
                "factored": bool(info[3])}

    def set_factorization(self, kind):
        """ "llt" or "ldlt" (or PO_CHOL_LLT = 0 / PO_CHOL_LDLT = 1), read by the next factor(); allowed at any time,
        also on an analysis-only object."""
        if isinstance(kind, str):
            if kind not in self.FACTORIZATIONS:
                raise ValueError("factorization must be one of %s" % sorted(self.FACTORIZATIONS))
            kind = self.FACTORIZATIONS[kind]
        check(lib.po_sparse_chol_set_factorization(self._h, int(kind)))

    @property
    def factorization(self):
        kind = C.c_int()
        check(lib.po_sparse_chol_get_factorization(self._h, C.byref(kind)))
        return {v: k for k, v in self.FACTORIZATIONS.items()}[kind.value]

    def inertia(self):
        """(positive, negative, replaced) pivots of the last factor(); they sum to size.  An "llt" factorization that
        replaced no pivot gives (size, 0, 0); one that did raises (its kernels do not count them)."""
        out = (C.c_int64 * 3)()
        check(lib.po_sparse_chol_inertia(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def packing(self):
        """The packed groups of tiny fronts (po_sparse_chol_packing): a dict with tiny (the order up to which a front
        is tiny), cap (fronts per group at most, read from debug switch 38 at creation; 0: no packing), num_groups,
        factor_levels (levels that launch anything in the factorization), group_first / group_root / group_level
        (group g is the supernodes group_first[g] .. group_root[g], run by one lane at level group_level[g]),
        front_order (s + b of every supernode) and upd_off (its update matrix's offset in the arena)."""
        return _chol_packing(lib.po_sparse_chol_packing, self._h, lambda: self.num_snodes)

    def kernel_forms(self, nv=1):
        """{kernel form: number of levels that launch it} for the factorization and one forward and one backward
        sweep over nv right-hand sides, computed by the code the launchers loop over; no device needed."""
        return _chol_kernel_forms(lib.po_sparse_chol_kernel_forms, self._h, nv)

    def getInfo(self):
        """(size, num_snodes, nnzL) as ParOptSparseCholesky::getInfo."""
        return self.size, self.num_snodes, self.nnzL

    def set_values(self, *args):
        """set_values(vals): values in the entry order of the creation pattern; set_values(colp, rows, vals): any
        pattern inside the factor's (the reference's setValues).  Repeated entries add up."""
        if len(args) == 1:
            colp, rows = self._colp, self._rows
        elif len(args) == 3:
            colp = np.ascontiguousarray(args[0], dtype=np.intc)
            rows = np.ascontiguousarray(args[1], dtype=np.intc)
            if colp.shape != (self.size + 1,) or len(rows) < int(colp[-1]):
                raise ValueError("set_values: colp / rows do not describe a matrix of this size")
        else:
            raise TypeError("set_values(vals) or set_values(colp, rows, vals)")
        vals = np.ascontiguousarray(args[-1], dtype=np.float64)
        if len(vals) < int(colp[-1]):
            raise ValueError("set_values: fewer values than entries")
        check(lib.po_sparse_chol_set_values(self._h, self.size, colp.ctypes.data_as(L.c_int_p),
                                            rows.ctypes.data_as(L.c_int_p), vals.ctypes.data_as(L.c_double_p)))

    def _tensor_ptr(self, t, count, who):
        import torch

        if self.ctx is None:
            raise L.ParOptAMDError(3, who + ": an analysis-only object has no device")
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous()
                or t.device != torch.device("cuda", self.ctx.device()) or t.numel() < count):
            raise ValueError(who + ": a contiguous float64 tensor on the context's device is required")
        torch.cuda.current_stream(t.device).synchronize()  # (what produced t is done before the context's stream reads it)
        return t.data_ptr()

    def set_values_device(self, t):
        """Values from a torch tensor on the context's device, in the entry order of the creation pattern (no copy)."""
        ptr = self._tensor_ptr(t, int(self._colp[-1]), "set_values_device")
        check(lib.po_sparse_chol_set_values_device(self._h, ptr))

    def factor(self):
        """0, or 1 + the permuted index of the first non-positive pivot (it is replaced by 1 and the factorization
        finishes).  With "ldlt": of the first pivot that is exactly zero or NaN."""
        info = C.c_int()
        check(lib.po_sparse_chol_factor(self._h, C.byref(info)))
        return info.value

    def solve(self, b):
        """x = A^-1 b for b of shape (n,) or (nrhs, n); returns a new array."""
        x = np.array(b, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (1, 2) or x.shape[-1] != self.size:
            raise ValueError("solve: b must have shape (n,) or (nrhs, n)")
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        check(lib.po_sparse_chol_solve(self._h, x.ctypes.data_as(L.c_double_p), nrhs, self.size))
        return x

    def solve_tensor(self, t):
        """In place on a contiguous float64 torch tensor of shape (n,) or (nrhs, n) on the context's device."""
        if t.dim() not in (1, 2) or t.shape[-1] != self.size:
            raise ValueError("solve_tensor: t must have shape (n,) or (nrhs, n)")
        nrhs = 1 if t.dim() == 1 else t.shape[0]
        ptr = self._tensor_ptr(t, nrhs * self.size, "solve_tensor")
        check(lib.po_sparse_chol_solve_device(self._h, ptr, nrhs, self.size))
        self.ctx.synchronize()
        return t

    # ---- retained matrix, diagonal shift, refined solve (po_sparse_chol_set_keep_matrix and what follows it) ----
    def set_keep_matrix(self, on=True):
        """Retain A -- the symmetric matrix whose permuted lower triangle set_values sums into the factor -- from the
        next set_values on; allowed on an analysis-only object (matrix_arrays() then works)."""
        check(lib.po_sparse_chol_set_keep_matrix(self._h, 1 if on else 0))

    @property
    def keep_matrix(self):
        on = C.c_int()
        check(lib.po_sparse_chol_get_keep_matrix(self._h, C.byref(on)))
        return bool(on.value)

    def matrix_arrays(self):
        """(rowp, col, vidx, nd): the full symmetric matrix in elimination order (row i is unknown perm[i]) as
        compressed rows sorted by column; vidx indexes the nd compact values.  Copies."""
        ptrs = [L.c_int_p() for _ in range(3)]
        nd = C.c_int64()
        check(lib.po_sparse_chol_matrix_arrays(self._h, *[C.byref(q) for q in ptrs], C.byref(nd)))
        rowp = np.ctypeslib.as_array(ptrs[0], shape=(self.size + 1,)).copy()
        nnz = int(rowp[-1])

        def arr(q):
            return np.ctypeslib.as_array(q, shape=(nnz,)).copy() if nnz > 0 else np.zeros(0, dtype=np.intc)

        return rowp, arr(ptrs[1]), arr(ptrs[2]), int(nd.value)

    def set_diagonal_shift(self, shift):
        """shift (size values, the caller's numbering) is added to the diagonal of what the next set_values puts into
        the factor: factor() factors A + diag(shift), the retained A does not get it.  None clears it."""
        if shift is None:
            check(lib.po_sparse_chol_set_diagonal_shift(self._h, None))
            return
        sh = np.ascontiguousarray(shift, dtype=np.float64)
        if sh.shape != (self.size,):
            raise ValueError("set_diagonal_shift: shift must have `size` entries")
        check(lib.po_sparse_chol_set_diagonal_shift(self._h, sh.ctypes.data_as(L.c_double_p)))

    def matvec(self, x):
        """y = A x for x of shape (n,) or (nrhs, n); returns a new array."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim not in (1, 2) or x.shape[-1] != self.size:
            raise ValueError("matvec: x must have shape (n,) or (nrhs, n)")
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        y = np.zeros_like(x)
        check(lib.po_sparse_chol_matvec(self._h, x.ctypes.data_as(L.c_double_p), self.size,
                                        y.ctypes.data_as(L.c_double_p), self.size, nrhs))
        return y

    def matvec_tensor(self, x, y):
        """y = A x on contiguous float64 torch tensors of shape (n,) or (nrhs, n) on the context's device."""
        if x.dim() not in (1, 2) or x.shape[-1] != self.size or y.shape != x.shape:
            raise ValueError("matvec_tensor: x and y must both have shape (n,) or (nrhs, n)")
        nrhs = 1 if x.dim() == 1 else x.shape[0]
        px = self._tensor_ptr(x, nrhs * self.size, "matvec_tensor")
        py = self._tensor_ptr(y, nrhs * self.size, "matvec_tensor")
        check(lib.po_sparse_chol_matvec_device(self._h, px, self.size, py, self.size, nrhs))
        self.ctx.synchronize()
        return y

    @staticmethod
    def _refine_args(nrhs, max_steps, tol):
        steps = np.zeros(nrhs, dtype=np.intc)
        eta0, eta = np.zeros(nrhs), np.zeros(nrhs)
        ptrs = (steps.ctypes.data_as(L.c_int_p), eta0.ctypes.data_as(L.c_double_p), eta.ctypes.data_as(L.c_double_p))
        return {"steps": steps, "eta0": eta0, "eta": eta}, (int(max_steps), -1.0 if tol is None else float(tol)) + ptrs

    def solve_refined(self, b, max_steps=5, tol=None):
        """(x, info): x = A^-1 b by the factorization (of A + diag(shift)) and iterative refinement against the
        retained A; b of shape (n,) or (nrhs, n).  info = {"steps", "eta0", "eta"}, arrays with one entry per
        right-hand side: corrections applied, the backward error max|b - A x| / (||A||_inf max|x| + max|b|) before
        the first of them and that of the x returned.  tol=None: eps."""
        x = np.array(b, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (1, 2) or x.shape[-1] != self.size:
            raise ValueError("solve_refined: b must have shape (n,) or (nrhs, n)")
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        info, args = self._refine_args(nrhs, max_steps, tol)
        check(lib.po_sparse_chol_solve_refined(self._h, x.ctypes.data_as(L.c_double_p), nrhs, self.size, *args))
        return x, info

    def solve_refined_tensor(self, t, max_steps=5, tol=None):
        """solve_refined in place on a contiguous float64 torch tensor of shape (n,) or (nrhs, n) on the context's
        device; returns (t, info)."""
        if t.dim() not in (1, 2) or t.shape[-1] != self.size:
            raise ValueError("solve_refined_tensor: t must have shape (n,) or (nrhs, n)")
        nrhs = 1 if t.dim() == 1 else t.shape[0]
        ptr = self._tensor_ptr(t, nrhs * self.size, "solve_refined_tensor")
        info, args = self._refine_args(nrhs, max_steps, tol)
        check(lib.po_sparse_chol_solve_refined_device(self._h, ptr, nrhs, self.size, *args))
        self.ctx.synchronize()
        return t, info

    def close(self):
        if self._h:
            lib.po_sparse_chol_destroy(self._h)
            self._h = L.po_sparse_chol()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


def quasidef_factor(problem, x, dinv, c):
    """ParOptQuasiDefMat::factor (src/ParOptSparseMat.h:25) of the problem's sparse constraints."""
    check(lib.po_quasidef_factor(problem.handle, x.handle, dinv.handle, c.handle))


def quasidef_apply(problem, x, dinv, c, bx, bw, yx, yw):
    """ParOptQuasiDefMat::apply (:39-56); bw may be None."""
    check(lib.po_quasidef_apply(problem.handle, x.handle, dinv.handle, c.handle, bx.handle,
                                bw.handle if bw is not None else None, yx.handle, yw.handle))


def quasidef_gram(problem, x, dinv, c, P, alpha=None):
    """The panel steps of the sparse solver, stand-alone, after quasidef_factor (c as that call left it): for the list
    P of nv PVecs (n) and U_j = Aw (dinv o P_j) returns (W2, out) with W2 = U^T S^-1 U (nv x nv numpy) and, when alpha
    (nv coefficients) is given, out = -S^-1 (U alpha) as a new PVec (else None).  The sequence is the interior point's
    Gram correction and correction, through the problem's own solver; nv is not limited."""
    nv = len(P)
    handles = (L.po_vec * max(nv, 1))(*[v.handle for v in P])
    W2 = np.zeros((nv, nv), dtype=np.float64, order="F")
    out, a = None, None
    if alpha is not None:
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        if a.shape != (nv,):
            raise ValueError("quasidef_gram: alpha must have one coefficient per panel vector")
        out = PVec(c.ctx, len(c))
    check(lib.po_quasidef_gram(problem.handle, x.handle, dinv.handle, c.handle, handles, nv,
                               W2.ctypes.data_as(L.c_double_p), a.ctypes.data_as(L.c_double_p) if a is not None else None,
                               out.handle if out is not None else None))
    return W2, out


def quasidef_factor_info(problem):
    s = lib.po_quasidef_factor_info(problem.handle)
    return s.decode() if s else None


class _Driver:
    """What InteriorPoint, TrustRegion and MMA share over their po_<x>_* entries: typed setOption, the handle's release,
    the iteration callback and the tail of optimize()."""

    _PREFIX = None  # "ip", "tr", "mma"
    _ITER_FN = L.TR_ITER_FN
    _QN_CALLBACKS = True  # optimize() can run a user-written quasi-Newton approximation

    def _entry(self, name):
        return getattr(lib, "po_%s_%s" % (self._PREFIX, name))

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                self._entry("destroy")(self._h)
        except Exception:
            pass

    def setOption(self, name, value):
        nm = name.encode()
        if isinstance(value, bool):
            check(self._entry("set_option_int")(self._h, nm, int(value)))
        elif isinstance(value, int):
            # int given for a float option is a type error in the reference too; be lenient only
            # in the obvious direction (python ints for float-valued settings)
            rc = self._entry("set_option_int")(self._h, nm, value)
            if rc != 0:
                check(self._entry("set_option_float")(self._h, nm, float(value)))
        elif isinstance(value, float):
            check(self._entry("set_option_float")(self._h, nm, value))
        else:
            check(self._entry("set_option_str")(self._h, nm, str(value).encode()))

    def _keep_callback(self, cb):
        self._cbs.append(cb)

    def setIterationCallback(self, fn):
        def _cb(user, k):
            fn(k)
            return 0

        cb = self._ITER_FN(_cb)
        self._keep_callback(cb)
        check(self._entry("set_iteration_callback")(self._h, cb, None))

    def _finish_optimize(self, rc):
        if hasattr(self.problem, "_raise_pending"):
            self.problem._raise_pending()  # an exception thrown inside a problem callback
        if self._QN_CALLBACKS:
            _raise_qn_pending()  # ... or inside a user-written quasi-Newton approximation
        if rc != 0:
            raise L.ParOptAMDError(rc, lib.po_last_error().decode(errors="replace"))
        return rc


class InteriorPoint(_Driver):
    """ParOptInteriorPoint (reference src/ParOptInteriorPoint.h:128-217)."""

    _PREFIX = "ip"
    _ITER_FN = L.ITER_FN

    def __init__(self, problem, options=None):
        self.problem = problem
        self.ctx = problem.ctx
        self._h = L.po_ip()
        check(lib.po_ip_create(problem.handle, C.byref(self._h)))
        self._iter_cb = None
        opts = dict(options or {})
        # the C ABI keeps the reference's default ("paropt.out" in the working directory); the
        # Python harness only writes the iteration table when asked to
        opts.setdefault("output_file", "")
        for k, v in opts.items():
            self.setOption(k, v)

    def _keep_callback(self, cb):
        self._iter_cb = cb  # one slot: a new callback releases the last

    def optimize(self, checkpoint=None):
        return self._finish_optimize(lib.po_ip_optimize(self._h, checkpoint.encode() if checkpoint else None))

    def writeSolutionFile(self, filename):
        check(lib.po_ip_write_solution_file(self._h, filename.encode()))

    def readSolutionFile(self, filename):
        check(lib.po_ip_read_solution_file(self._h, filename.encode()))

    def getOptimizedPoint(self):
        x, zl, zu = L.po_vec(), L.po_vec(), L.po_vec()
        z = L.c_double_p()
        check(lib.po_ip_get_optimized_point(self._h, C.byref(x), C.byref(z), C.byref(zl), C.byref(zu)))
        c = self.problem.ncon
        # zl / zu are None for a side the problem declares unused (as the reference returns NULL)
        return (PVec(self.ctx, handle=x, owned=False), np.array([z[i] for i in range(c)]),
                PVec(self.ctx, handle=zl, owned=False) if zl else None,
                PVec(self.ctx, handle=zu, owned=False) if zu else None)

    def getOptimizedSlacks(self):
        ptrs = [L.c_double_p() for _ in range(4)]
        check(lib.po_ip_get_optimized_slacks(self._h, *[C.byref(p) for p in ptrs]))
        c = self.problem.ncon
        return tuple(np.array([p[i] for i in range(c)]) for p in ptrs)

    def getOptimizedSparse(self):
        """(zw, sw, tw, zsw, ztw) as borrowed PVec handles, or None when nwcon = 0."""
        hs = [L.po_vec() for _ in range(5)]
        check(lib.po_ip_get_optimized_sparse(self._h, *[C.byref(h) for h in hs]))
        if not hs[0]:
            return None
        return tuple(PVec(self.ctx, handle=h, owned=False) for h in hs)

    def getIterationCounters(self):
        a, b, d = C.c_int(), C.c_int(), C.c_int()
        check(lib.po_ip_get_counters(self._h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value, b.value, d.value

    def setPenaltyGamma(self, gamma):
        check(lib.po_ip_set_penalty_gamma(self._h, float(gamma)))

    def setMultiplePenaltyGamma(self, gamma):
        arr = np.ascontiguousarray(gamma, dtype=np.float64)
        assert len(arr) == self.problem.ncon
        check(lib.po_ip_set_penalty_gamma_array(self._h, arr.ctypes.data_as(L.c_double_p)))

    def setQuasiNewton(self, qn):
        """Use a caller-owned LBFGS / LSR1 (kept alive by this object); None detaches it."""
        self._qn_ref = qn
        if isinstance(qn, CompactQuasiNewton) and qn.ncon is None:
            qn.ncon = int(self.problem.ncon)
        _qn_check(lib.po_ip_set_quasi_newton(self._h, qn._h if qn is not None else None))

    def resetProblemInstance(self, problem):
        self._prob_ref = problem
        check(lib.po_ip_reset_problem_instance(self._h, problem.handle))

    def resetQuasiNewtonHessian(self):
        check(lib.po_ip_reset_quasi_newton(self._h))

    def resetDesignAndBounds(self):
        check(lib.po_ip_reset_design_and_bounds(self._h))

    def checkGradients(self, dh=1e-6):
        """ParOptInteriorPoint::checkGradients(dh) (reference .cpp:6196-6199): the problem's finite-difference check
        at the solver's current point; returns (and prints) the report."""
        t = C.c_char_p()
        check(lib.po_ip_check_gradients(self._h, float(dh), C.byref(t)))
        text = (t.value or b"").decode()
        print(text, end="")
        return text

    def checkMeritFuncGradient(self, xpt=None, dh=1e-6):
        """ParOptInteriorPoint::checkMeritFuncGradient(xpt, dh) (.cpp:3280-3432): returns (finite difference, actual)."""
        fd, act = C.c_double(), C.c_double()
        check(lib.po_ip_check_merit_func_gradient(self._h, xpt.handle if xpt is not None else None, float(dh),
                                                  C.byref(fd), C.byref(act)))
        return fd.value, act.value

    def setBFGSUpdateType(self, update_type):
        """setBFGSUpdateType (.cpp:1179-1186): applies to the solver's own L-BFGS object."""
        h = L.po_qn()
        check(lib.po_ip_get_quasi_newton(self._h, C.byref(h)))
        if h:
            check(lib.po_qn_set_update_type(h, 1 if update_type in (1, "damped_update", "damped") else 0))

    def setUseDiagHessian(self, truth):
        self.setOption("use_diag_hessian", bool(truth))

    def getHvecCount(self):
        v = C.c_int()
        check(lib.po_ip_get_hvec_count(self._h, C.byref(v)))
        return v.value

    HVEC_MODES = {"exact": 0, "when_missing": 1, "always": 2}

    def setHvecFiniteDifference(self, mode="when_missing", central=False, rel_step=None):
        """Hessian-vector products by differences of the Lagrangian's gradient (po_ip_set_hvec_finite_difference; no
        reference counterpart): lets use_hvec_product run with a problem that has no evalHvecProduct.  mode: "exact"
        (the problem's product only, the default of a new solver), "when_missing" (differences once the problem's
        product has failed) or "always"; central: two extra evaluations per product instead of one; rel_step: None
        for sqrt(eps) / cbrt(eps)."""
        m = self.HVEC_MODES[mode] if isinstance(mode, str) else int(mode)
        check(lib.po_ip_set_hvec_finite_difference(self._h, m, 1 if central else 0,
                                                   0.0 if rel_step is None else float(rel_step)))
        return self

    def getHvecFiniteDifferenceCount(self):
        """(products, evaluations) of the differenced products since optimize() began; the evaluations are NOT part
        of getIterationCounters()."""
        a, b = C.c_int(), C.c_int()
        check(lib.po_ip_get_hvec_fd_count(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def getHvecFiniteDifferenceStep(self):
        """The step h of the last differenced product (identical on every rank)."""
        v = C.c_double()
        check(lib.po_ip_get_hvec_fd_step(self._h, C.byref(v)))
        return v.value

    def evalHvec(self, z, zw, px, hvec):
        """hvec = H(x, z, zw) px at the solver's current point by the configured mode (po_ip_eval_hvec); z: dense
        multipliers (array), zw: PVec or None, px / hvec: two different PVec."""
        arr = np.ascontiguousarray(z if z is not None else [], dtype=np.float64)
        assert len(arr) == self.problem.ncon
        raw = [getattr(v, "_v", v) for v in (zw, px, hvec)]  # (ParOpt.PVec wraps the library's vector)
        rc = lib.po_ip_eval_hvec(self._h, arr.ctypes.data_as(L.c_double_p),
                                 raw[0].handle if raw[0] is not None else None, raw[1].handle, raw[2].handle)
        if hasattr(self.problem, "_raise_pending"):
            self.problem._raise_pending()
        check(rc)
        return hvec

    def getBarrierParameter(self):
        v = C.c_double()
        check(lib.po_ip_get_barrier_parameter(self._h, C.byref(v)))
        return v.value

    def getComplementarity(self):
        v = C.c_double()
        check(lib.po_ip_get_complementarity(self._h, C.byref(v)))
        return v.value

    def getObjective(self):
        f, rho = C.c_double(), C.c_double()
        check(lib.po_ip_get_objective(self._h, C.byref(f), C.byref(rho)))
        return f.value, rho.value

    def getQuasiNewton(self):
        h = L.po_qn()
        check(lib.po_ip_get_quasi_newton(self._h, C.byref(h)))
        return _QuasiNewton(self.ctx, 0, 0, 0, handle=h) if h else None

    def getHistory(self):
        t = C.c_char_p()
        check(lib.po_ip_get_history(self._h, C.byref(t)))
        return t.value.decode()

    def setCallbackTiming(self, on=True):
        """Event timing of the problem's callbacks (the "user_eval" entry of getPhaseTimes): off by default, every
        event record costs the stream some dispatch latency (po_ip_set_callback_timing)."""
        check(lib.po_ip_set_callback_timing(self._h, 1 if on else 0))
        return self

    def getPhaseTimes(self):
        names, secs, cnt = C.c_char_p(), L.c_double_p(), C.c_int()
        check(lib.po_ip_get_phase_times(self._h, C.byref(names), C.byref(secs), C.byref(cnt)))
        nm = names.value.decode().split(";") if cnt.value else []
        return {nm[i]: secs[i] for i in range(cnt.value)}

    def debugKKTStep(self, mu):
        px, pzl, pzu = L.po_vec(), L.po_vec(), L.po_vec()
        d = [L.c_double_p() for _ in range(5)]
        check(lib.po_ip_debug_kkt_step(self._h, float(mu), C.byref(px), C.byref(pzl), C.byref(pzu),
                                       *[C.byref(p) for p in d]))
        c = self.problem.ncon
        out = dict(x=PVec(self.ctx, handle=px, owned=False).to_numpy(),
                   zl=PVec(self.ctx, handle=pzl, owned=False).to_numpy(),
                   zu=PVec(self.ctx, handle=pzu, owned=False).to_numpy())
        for name, p in zip(("z", "s", "t", "zs", "zt"), d):
            out[name] = np.array([p[i] for i in range(c)])
        wh = [L.po_vec() for _ in range(5)]
        check(lib.po_ip_debug_kkt_step_sparse(self._h, *[C.byref(h) for h in wh]))
        if wh[0]:
            for name, h in zip(("zw", "sw", "tw", "zsw", "ztw"), wh):
                out[name] = PVec(self.ctx, handle=h, owned=False).to_numpy()
        return out

    def debugSetState(self, z, s, t, zs, zt, mu):
        """po_ip_debug_set_state: dense blocks + barrier parameter of an injected state (x, zl, zu and the sparse
        blocks are written through getOptimizedPoint() / getOptimizedSparse() handles beforehand)."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (z, s, t, zs, zt)]
        check(lib.po_ip_debug_set_state(self._h, *[a.ctypes.data_as(L.c_double_p) for a in arrs], float(mu)))

    def debugKKT(self, mu, mode, tau=0.95):
        """po_ip_debug_kkt: the pieces of one KKT step at the current state as numpy copies (mode 0: one bordered
        solve; mode 1: the fused kernel sequence of a plain iteration = the step after one refinement)."""
        d = L.KKTDump()
        check(lib.po_ip_debug_kkt(self._h, float(mu), int(mode), float(tau), C.byref(d)))
        c, k = d.c, d.k
        m = c + k

        def arr(p, cnt):
            return np.array([p[i] for i in range(cnt)], dtype=np.float64)

        def vec(h):
            return PVec(self.ctx, handle=L.po_vec(h), owned=False).to_numpy()

        out = dict(c=c, k=k, Dinv=vec(d.Dinv), res_x=vec(d.res_x), res_z=arr(d.res_z, c), res_s=arr(d.res_s, c),
                   res_t=arr(d.res_t, c), res_zs=arr(d.res_zs, c), res_zt=arr(d.res_zt, c),
                   res_norms=np.array(list(d.res_norms)),
                   W=arr(d.W, m * m).reshape(m, m).T, G=arr(d.G, c * c).reshape(c, c).T,
                   Ce=arr(d.Ce, k * k).reshape(k, k).T if k > 0 else np.zeros((0, 0)),
                   gpiv=np.array([d.gpiv[i] for i in range(c)], dtype=np.int64) + 1,
                   cpiv=np.array([d.cpiv[i] for i in range(k)], dtype=np.int64) + 1,
                   step_x=vec(d.px), step_zl=vec(d.pzl), step_zu=vec(d.pzu), step_z=arr(d.pz, c),
                   step_s=arr(d.ps, c), step_t=arr(d.pt, c), step_zs=arr(d.pzs, c), step_zt=arr(d.pzt, c),
                   step_mins=np.array(list(d.step_mins)))
        wh = [L.po_vec() for _ in range(5)]
        check(lib.po_ip_debug_kkt_step_sparse(self._h, *[C.byref(h) for h in wh]))
        if wh[0]:
            for name, h in zip(("zw", "sw", "tw", "zsw", "ztw"), wh):
                out["step_" + name] = PVec(self.ctx, handle=h, owned=False).to_numpy()
        return out

    def snapshot(self):
        """State in the layout of oracle snapshots / golden 'itNNN/' records."""
        x, z, zl, zu = self.getOptimizedPoint()
        s, t, zs, zt = self.getOptimizedSlacks()
        niter, neval, ngeval = self.getIterationCounters()
        f, rho = self.getObjective()
        d = dict(mu=self.getBarrierParameter(), rho=rho, fobj=f, z=z, s=s, t=t, zs=zs, zt=zt,
                 counters=np.array([niter, neval, ngeval]),
                 norms=np.array([x.norm(), zl.norm() if zl is not None else np.nan,
                                 zu.norm() if zu is not None else np.nan]))
        wv = self.getOptimizedSparse()
        if wv is not None:
            d["wnorms"] = np.array([v.norm() for v in wv])
        qn = self.getQuasiNewton()
        if qn is not None:
            k, b0 = C.c_int(), C.c_double()
            check(lib.po_qn_get_compact(qn._h, C.byref(k), C.byref(b0), None, None, None))
            d["qn_size"] = k.value
            d["qn_b0"] = b0.value
            pp, pn = L.c_int_p(), C.c_int()
            check(lib.po_qn_get_pivots(qn._h, C.byref(pp), C.byref(pn)))
            d["mfpiv"] = np.array([pp[i] for i in range(pn.value)], dtype=np.int64) + 1  # LAPACK numbering
        d.update(self.getDebugInts())
        return d

    def getDebugInts(self):
        """SURVEY 8a' integers in the reference's numbering: gpiv (1-based LAPACK rows), check_flag, clamped[8]."""
        pp, pn, fl = L.c_int_p(), C.c_int(), C.c_int()
        cl = (C.c_int64 * 8)()
        check(lib.po_ip_get_debug_ints(self._h, C.byref(pp), C.byref(pn), C.byref(fl), cl))
        return dict(gpiv=np.array([pp[i] for i in range(pn.value)], dtype=np.int64) + 1, check_flag=fl.value,
                    clamped=np.array(list(cl), dtype=np.int64))

    def getBounds(self):
        """(lb, ub) as repaired by initAndCheckDesignAndBounds (borrowed)."""
        a, b = L.po_vec(), L.po_vec()
        check(lib.po_ip_get_bounds(self._h, C.byref(a), C.byref(b)))
        return PVec(self.ctx, handle=a, owned=False), PVec(self.ctx, handle=b, owned=False)


class EigenApprox:
    """ParOptCompactEigenApprox as seen by the model-update callback: c0 (settable), g0 (PVec), N,
    M and Minv (row-major N x N numpy views, writable), hvecs (list of PVec)."""

    def __init__(self, ctx, handle):
        c0, g0, N = L.c_double_p(), L.po_vec(), C.c_int()
        M, Minv, hv = L.c_double_p(), L.c_double_p(), L.vec_p()
        check(lib.po_eig_get_approximation(handle, C.byref(c0), C.byref(g0), C.byref(N), C.byref(M),
                                           C.byref(Minv), C.byref(hv)))
        self.N = N.value
        self._c0 = c0
        self.g0 = PVec(ctx, handle=g0, owned=False)
        self.M = np.ctypeslib.as_array(M, shape=(self.N, self.N))
        self.Minv = np.ctypeslib.as_array(Minv, shape=(self.N, self.N))
        self.hvecs = [PVec(ctx, handle=L.po_vec(hv[i]), owned=False) for i in range(self.N)]

    @property
    def c0(self):
        return self._c0[0]

    @c0.setter
    def c0(self, v):
        self._c0[0] = float(v)


class CompactEigenApprox(EigenApprox):
    """ParOptCompactEigenApprox(problem, N) (reference src/ParOptCompactEigenvalueApprox.h:7-32): the object the user's
    code creates and hands to EigenQuasiNewton; c0 / g0 / M / Minv / hvecs as in EigenApprox."""

    def __init__(self, problem, N):
        self.ctx = problem.ctx
        self.problem = problem
        self._eh = L.po_eig()
        check(lib.po_eig_create(problem.handle, int(N), C.byref(self._eh)))
        super().__init__(problem.ctx, self._eh)

    def __del__(self):
        try:
            if self._eh and self.ctx._h:
                lib.po_eig_destroy(self._eh)
        except Exception:
            pass

    @property
    def handle(self):
        return self._eh

    def multAdd(self, alpha, x, y):
        check(lib.po_eig_mult_add(self._eh, float(alpha), x.handle, y.handle))

    def evalApproximation(self, s=None, t=None):
        v = C.c_double()
        check(lib.po_eig_eval_approximation(self._eh, s.handle if s is not None else None,
                                            t.handle if t is not None else None, C.byref(v)))
        return v.value

    def evalApproximationGradient(self, s, grad):
        check(lib.po_eig_eval_approximation_gradient(self._eh, s.handle, grad.handle))


class EigenQuasiNewton(_QuasiNewton):
    """ParOptEigenQuasiNewton(qn, eigh, index) (.h:34-84): B = B_qn - z0 H M H^T as one compact matrix; qn may be
    None.  A quasi-Newton object like any other (mult / multAdd / getCompactMat)."""

    def __init__(self, qn, eigh, index=0):
        self.qn, self.eigh = qn, eigh  # kept alive: the library object borrows both
        h = L.po_qn()
        check(lib.po_eigqn_create(qn._h if qn is not None else None, eigh.handle, int(index), C.byref(h)))
        super().__init__(eigh.ctx, 0, 0, 0, handle=h)
        self._owned = True
        self.index = int(index)

    def setUseQuasiNewtonObjective(self, truth):
        check(lib.po_eigqn_set_use_quasi_newton_objective(self._h, int(bool(truth))))

    def updateMultipliers(self, z):
        za = (C.c_double * len(z))(*[float(v) for v in z])
        check(lib.po_eigqn_update_multipliers(self._h, za))


class TrustRegionSubproblem:
    """ParOptTrustRegionSubproblem (reference src/ParOptTrustRegion.h:15-151) in its library forms.  Also the
    ParOptProblem the interior-point solver is built on: ``InteriorPoint(subproblem, options)``."""

    def __init__(self, problem):
        self.problem = problem
        self.ctx = problem.ctx
        self.nvars, self.ncon = problem.nvars, problem.ncon
        self.nwcon = getattr(problem, "nwcon", 0)
        self._h = L.po_trsub()
        self._keep = []

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                lib.po_trsub_destroy(self._h)
        except Exception:
            pass

    @property
    def handle(self):
        """the subproblem as a po_problem (borrowed)"""
        p = L.po_problem()
        check(lib.po_trsub_problem(self._h, C.byref(p)))
        return p

    def _raise_pending(self):
        if hasattr(self.problem, "_raise_pending"):
            self.problem._raise_pending()

    def initModelAndBounds(self, tr_size):
        check(lib.po_trsub_init_model_and_bounds(self._h, float(tr_size)))

    def setTrustRegionBounds(self, tr_size):
        check(lib.po_trsub_set_trust_region_bounds(self._h, float(tr_size)))

    def evalTrialStepAndUpdate(self, update_flag, step, z, zw=None):
        za = (C.c_double * max(1, self.ncon))(*[float(v) for v in z])
        f, cons = C.c_double(), (C.c_double * max(1, self.ncon))()
        check(lib.po_trsub_eval_trial_step_and_update(self._h, int(update_flag), step.handle, za,
                                                      zw.handle if zw is not None else None, C.byref(f), cons))
        return f.value, np.array(cons[:self.ncon])

    def acceptTrialStep(self, step, z, zw=None):
        za = (C.c_double * max(1, self.ncon))(*[float(v) for v in z]) if z is not None else None
        check(lib.po_trsub_accept_trial_step(self._h, step.handle, za, zw.handle if zw is not None else None))

    def rejectTrialStep(self):
        check(lib.po_trsub_reject_trial_step(self._h))

    def getQuasiNewtonUpdateType(self):
        t = C.c_int()
        check(lib.po_trsub_get_quasi_newton_update_type(self._h, C.byref(t)))
        return t.value

    # the ParOptProblem side (the model in the step), as the interior point sees it
    def getVarsAndBounds(self, step, lower, upper):
        check(lib.po_problem_get_vars_and_bounds(self.handle, step.handle, lower.handle, upper.handle))

    def evalObjCon(self, step):
        f = C.c_double()
        con = np.zeros(max(self.ncon, 1))
        rc = lib.po_problem_eval_obj_con(self.handle, step.handle, C.byref(f), con.ctypes.data_as(L.c_double_p))
        return rc, f.value, con[: self.ncon]

    def evalObjConGradient(self, step, g, A):
        hs = (L.po_vec * max(1, self.ncon))(*[a.handle for a in A])
        return lib.po_problem_eval_obj_con_gradient(self.handle, step.handle, g.handle, hs)

    def getLinearModel(self):
        """(xk, fk, gk, ck, Ak, lb, ub) of the current model (borrowed vectors)."""
        xk, gk, lb, ub, Ak = L.po_vec(), L.po_vec(), L.po_vec(), L.po_vec(), L.vec_p()
        fk, ck, m = C.c_double(), L.c_double_p(), C.c_int()
        check(lib.po_trsub_get_linear_model(self._h, C.byref(xk), C.byref(fk), C.byref(gk), C.byref(ck), C.byref(Ak),
                                            C.byref(lb), C.byref(ub), C.byref(m)))
        wrap = lambda h: PVec(self.ctx, handle=h, owned=False)  # noqa: E731
        return (wrap(xk), fk.value, wrap(gk), np.array([ck[i] for i in range(m.value)]),
                [wrap(L.po_vec(Ak[i])) for i in range(m.value)], wrap(lb), wrap(ub))


class UserTrustRegionSubproblem(TrustRegionSubproblem):
    """A trust-region subproblem written by the USER: subclass and override the virtuals of
    ParOptTrustRegionSubproblem (reference src/ParOptTrustRegion.h:15-151) -- all arguments are device vectors (PVec),
    multipliers numpy arrays:

        getQuasiNewton() -> LBFGS / LSR1 / EigenQuasiNewton or None
        initModelAndBounds(tr_size); setTrustRegionBounds(tr_size)
        evalTrialStepAndUpdate(update_flag, step, z, zw) -> (fail, fobj, cons)
        acceptTrialStep(step, z, zw) -> fail;  rejectTrialStep();  getQuasiNewtonUpdateType() -> int
        getLinearModel() -> (xk, fk, gk, ck, Ak, lb, ub)            (the user's own vectors; borrowed by the driver)

    and the ParOptProblem side the interior point solves (the model in the step):

        getVarsAndBounds(step, lower, upper)                         (filled in place)
        evalObjCon(step or None) -> (fail, fobj, cons)               (None: the values at a zero step)
        evalObjConGradient(step, g, A) -> fail                       (A is None when only g is wanted)

    ``TrustRegion(sub, options).optimize(InteriorPoint(sub, options))`` then drives it exactly like the library's own
    subproblems (po_trsub_create_callbacks)."""

    def __init__(self, problem):
        super().__init__(problem)
        ctx, m = self.ctx, self.ncon
        self._pending_exc = None
        wrap = lambda h: PVec(ctx, handle=L.po_vec(h), owned=False) if h else None  # noqa: E731

        def guard(fn):
            def g(*args):
                if self._pending_exc is not None:
                    return 1
                try:
                    return int(fn(*args) or 0)
                except BaseException as e:  # noqa: BLE001 - re-raised by _raise_pending()
                    self._pending_exc = e
                    return 1
            return g

        @guard
        def _getqn(user, out):
            q = self.getQuasiNewton()
            out[0] = q._h if q is not None else None
            return 0

        @guard
        def _init(user, tr):
            return self.initModelAndBounds(tr)

        @guard
        def _setb(user, tr):
            return self.setTrustRegionBounds(tr)

        @guard
        def _trial(user, flag, step, z, zw, fobj, cons):
            fail, f, c = self.evalTrialStepAndUpdate(flag, wrap(step), np.array([z[i] for i in range(m)]), wrap(zw))
            fobj[0] = float(f)
            for i in range(m):
                cons[i] = float(c[i])
            return fail

        @guard
        def _accept(user, step, z, zw):
            za = np.array([z[i] for i in range(m)]) if z else None
            return self.acceptTrialStep(wrap(step), za, wrap(zw))

        @guard
        def _reject(user):
            return self.rejectTrialStep()

        def _utype(user):
            try:
                return int(self.getQuasiNewtonUpdateType())
            except BaseException as e:  # noqa: BLE001
                self._pending_exc = self._pending_exc or e
                return 0

        @guard
        def _model(user, xk, fk, gk, ck, Ak, lb, ub):
            vx, f, vg, c, A, vl, vu = self.getLinearModel()
            # the arrays handed out must outlive the call: kept on the object until the next call
            self._ck_arr = (C.c_double * max(1, m))(*[float(v) for v in c])
            self._ak_arr = (L.po_vec * max(1, m))(*[a.handle.value for a in A])
            xk[0], gk[0], lb[0], ub[0] = vx.handle.value, vg.handle.value, vl.handle.value, vu.handle.value
            fk[0] = float(f)
            ck[0] = C.cast(self._ck_arr, L.c_double_p)
            Ak[0] = C.cast(self._ak_arr, L.vec_p)
            return 0

        @guard
        def _bounds(user, step, lo, up):
            return self.getVarsAndBounds(wrap(step), wrap(lo), wrap(up))

        @guard
        def _eval(user, step, fobj, cons):
            fail, f, c = self.evalObjCon(wrap(step))
            fobj[0] = float(f)
            for i in range(m):
                cons[i] = float(c[i])
            return fail

        @guard
        def _grad(user, step, g, Ac):
            A = [wrap(Ac[i]) for i in range(m)] if Ac else None
            return self.evalObjConGradient(wrap(step), wrap(g), A)

        cb = L.TrSubCallbacks()
        self._fns = (L.TRSUB_GETQN_FN(_getqn), L.TRSUB_SIZE_FN(_init), L.TRSUB_SIZE_FN(_setb), L.TRSUB_TRIAL_FN(_trial),
                     L.TRSUB_ACCEPT_FN(_accept), L.TRSUB_VOID_FN(_reject), L.TRSUB_VOID_FN(_utype),
                     L.TRSUB_MODEL_FN(_model), L.TRSUB_BOUNDS_FN(_bounds), L.TRSUB_EVAL_FN(_eval), L.TRSUB_GRAD_FN(_grad))
        cb.user = None
        (cb.get_quasi_newton, cb.init_model_and_bounds, cb.set_trust_region_bounds, cb.eval_trial_step_and_update,
         cb.accept_trial_step, cb.reject_trial_step, cb.get_quasi_newton_update_type, cb.get_linear_model,
         cb.get_vars_and_bounds, cb.eval_obj_con, cb.eval_obj_con_gradient) = self._fns
        self._cb_struct = cb
        check(lib.po_trsub_create_callbacks(problem.handle, C.byref(cb), C.byref(self._h)))

    def _raise_pending(self):
        e, self._pending_exc = self._pending_exc, None
        if e is not None:
            raise e
        super()._raise_pending()

    # the virtuals (the base class's versions of these names call INTO the library: a user subproblem defines them)
    def getQuasiNewton(self):
        return None

    def getQuasiNewtonUpdateType(self):
        return 0

    def rejectTrialStep(self):
        return 0


class QuadraticSubproblem(TrustRegionSubproblem):
    """ParOptQuadraticSubproblem(problem, qn) (.h:153-300); qn may be None."""

    def __init__(self, problem, qn=None):
        super().__init__(problem)
        self.qn = qn
        check(lib.po_trsub_create_quadratic(problem.handle, qn._h if qn is not None else None, C.byref(self._h)))

    def getQuasiNewton(self):
        return self.qn


class EigenSubproblem(TrustRegionSubproblem):
    """ParOptEigenSubproblem(problem, eig_qn) (src/ParOptCompactEigenvalueApprox.h:86-206)."""

    def __init__(self, problem, eig_qn):
        super().__init__(problem)
        self.eig_qn = eig_qn
        check(lib.po_trsub_create_eigen(problem.handle, eig_qn._h, C.byref(self._h)))

    def getQuasiNewton(self):
        return self.eig_qn

    def setEigenModelUpdate(self, update):
        """update(x: PVec, approx: CompactEigenApprox) is called at the starting point and at every accepted point with
        c0 / g0 preset; it fills hvecs, M and Minv (setEigenModelUpdate, .h:166-170)."""
        approx = self.eig_qn.eigh

        def _cb(user, x, eig):
            update(PVec(self.ctx, handle=L.po_vec(x), owned=False), approx)
            return 0

        fn = L.EIG_UPDATE_FN(_cb)
        self._keep.append(fn)
        check(lib.po_trsub_set_eigen_model_update(self._h, fn, None))


class InfeasSubproblem:
    """ParOptInfeasSubproblem(subproblem, subproblem_objective, subproblem_constraint) (reference
    src/ParOptTrustRegion.h:293-374, .cpp:468-650): the problem of the trust-region driver's steering step as a problem
    of its own -- ``InteriorPoint(InfeasSubproblem(sub, LINEAR_OBJECTIVE, LINEAR_CONSTRAINT), options)``.  The selector
    constants are the reference's."""

    SUBPROBLEM_OBJECTIVE, LINEAR_OBJECTIVE, CONSTANT_OBJECTIVE = 1, 2, 3
    SUBPROBLEM_CONSTRAINT, LINEAR_CONSTRAINT = 1, 2

    def __init__(self, subproblem, subproblem_objective, subproblem_constraint):
        self.subproblem = subproblem  # borrowed by the library object: kept alive here
        self.ctx = subproblem.ctx
        self.nvars, self.ncon, self.nwcon = subproblem.nvars, subproblem.ncon, subproblem.nwcon
        self._h = L.po_problem()
        check(lib.po_infeas_create(subproblem._h, int(subproblem_objective), int(subproblem_constraint),
                                   C.byref(self._h)))

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                lib.po_problem_destroy(self._h)
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _raise_pending(self):
        self.subproblem._raise_pending()

    def setObjectiveScaling(self, scale):
        check(lib.po_infeas_set_objective_scaling(self._h, float(scale)))

    def getVarsAndBounds(self, x, lb, ub):
        check(lib.po_problem_get_vars_and_bounds(self._h, x.handle, lb.handle, ub.handle))

    def evalObjCon(self, x):
        f = C.c_double()
        con = np.zeros(max(self.ncon, 1))
        rc = lib.po_problem_eval_obj_con(self._h, x.handle, C.byref(f), con.ctypes.data_as(L.c_double_p))
        return rc, f.value, con[: self.ncon]

    def evalObjConGradient(self, x, g, A):
        hs = (L.po_vec * max(1, self.ncon))(*[a.handle for a in A])
        return lib.po_problem_eval_obj_con_gradient(self._h, x.handle, g.handle, hs)


class TrustRegion(_Driver):
    """ParOptTrustRegion.  ``TrustRegion(problem, options)`` assembles quasi-Newton object, quadratic (or eigenvalue)
    subproblem and interior-point solver the way ParOptOptimizer does for algorithm='tr' (reference
    src/ParOptOptimizer.cpp:108-183); ``TrustRegion(subproblem, options)`` with a TrustRegionSubproblem is the
    reference's own constructor (src/ParOptTrustRegion.cpp:660-718) and takes the solver at ``optimize(ip)``.
    `options` may mix interior-point and trust-region option names (one shared registry)."""

    _PREFIX = "tr"
    COLS = ("fobj", "infeas", "l1", "linfty", "smax", "tr", "rho", "model_reduc", "zav", "zmax", "gav", "gmax")

    def __init__(self, problem, options=None):
        self.problem = problem
        self.ctx = problem.ctx
        self._h = L.po_tr()
        self.subproblem = problem if isinstance(problem, TrustRegionSubproblem) else None
        if self.subproblem is not None:
            check(lib.po_tr_create_subproblem(problem._h, C.byref(self._h)))
        else:
            check(lib.po_tr_create(problem.handle, C.byref(self._h)))
        self._cbs = []
        opts = dict(options or {})
        opts.setdefault("tr_output_file", "")
        for k, v in opts.items():
            self.setOption(k, v)

    def setEigenModel(self, N, index, update):
        """update(x: PVec, approx: EigenApprox) fills approx.hvecs / M / Minv (c0, g0 are preset)."""
        def _cb(user, x, approx):
            update(PVec(self.ctx, handle=L.po_vec(x), owned=False), EigenApprox(self.ctx, L.po_eig(approx)))
            return 0

        fn = L.EIG_UPDATE_FN(_cb)
        self._cbs.append(fn)
        check(lib.po_tr_set_eigen_model(self._h, int(N), int(index), fn, None))

    def setEigenModelSynthetic(self, N, index, seed=0, curv=1.0):
        check(lib.po_tr_set_eigen_model_synthetic(self._h, int(N), int(index), int(seed), float(curv)))

    def optimize(self, ip=None):
        """optimize() for the self-assembled form; optimize(ip) with an InteriorPoint built on the subproblem for the
        reference's form (ParOptTrustRegion::optimize(ParOptInteriorPoint*), .cpp:2365-2384)."""
        if ip is not None:
            self._ip = ip
            rc = lib.po_tr_optimize_with(self._h, ip._h)
        else:
            rc = lib.po_tr_optimize(self._h)
        return self._finish_optimize(rc)

    def initialize(self):
        check(lib.po_tr_initialize(self._h))

    def setPenaltyGamma(self, gamma):
        if np.isscalar(gamma):
            check(lib.po_tr_set_penalty_gamma(self._h, float(gamma)))
        else:
            ga = (C.c_double * len(gamma))(*[float(v) for v in gamma])
            check(lib.po_tr_set_penalty_gamma_array(self._h, ga))

    def getOptimizedPoint(self):
        x, z, zw = L.po_vec(), L.c_double_p(), L.po_vec()
        check(lib.po_tr_get_optimized_point(self._h, C.byref(x), C.byref(z), C.byref(zw)))
        c = self.problem.ncon
        return (PVec(self.ctx, handle=x, owned=False), np.array([z[i] for i in range(c)]),
                PVec(self.ctx, handle=zw, owned=False) if zw else None)

    def getState(self):
        tr, it, si, ai, fk = C.c_double(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        pg, ck = L.c_double_p(), L.c_double_p()
        check(lib.po_tr_get_state(self._h, C.byref(tr), C.byref(it), C.byref(si), C.byref(ai), C.byref(pg),
                                  C.byref(fk), C.byref(ck)))
        c = self.problem.ncon
        return dict(tr_size=tr.value, iter_count=it.value, subproblem_iters=si.value,
                    adaptive_subproblem_iters=ai.value, penalty_gamma=np.array([pg[i] for i in range(c)]),
                    fk=fk.value, ck=np.array([ck[i] for i in range(c)]))

    def getLastRow(self):
        row, info = L.c_double_p(), C.c_char_p()
        check(lib.po_tr_get_last_row(self._h, C.byref(row), C.byref(info)))
        return [row[i] for i in range(12)], info.value.decode().split()

    def getLastSolveLines(self):
        """Last iteration-table line of the steering (or restoration) solve and of the QP solve of the latest
        trust-region iteration: how each interior-point solve ended."""
        a, b = C.c_char_p(), C.c_char_p()
        check(lib.po_tr_get_last_solve_lines(self._h, C.byref(a), C.byref(b)))
        return (a.value or b"").decode(), (b.value or b"").decode()

    def getHistory(self):
        t = C.c_char_p()
        check(lib.po_tr_get_history(self._h, C.byref(t)))
        return t.value.decode()

    def getQuasiNewton(self):
        h = L.po_qn()
        check(lib.po_tr_get_quasi_newton(self._h, C.byref(h)))
        return _QuasiNewton(self.ctx, 0, 0, 0, handle=h) if h else None

    def getModelVectors(self):
        xk, gk = L.po_vec(), L.po_vec()
        check(lib.po_tr_get_model_vectors(self._h, C.byref(xk), C.byref(gk)))
        return PVec(self.ctx, handle=xk, owned=False), PVec(self.ctx, handle=gk, owned=False)

    def snapshot(self):
        """State in the layout of the golden 'trNNN/' records (oracle/ref_driver.cpp TrHook)."""
        s = self.getState()
        xk, gk = self.getModelVectors()
        d = dict(tr_size=s["tr_size"], penalty_gamma=s["penalty_gamma"], fk=s["fk"], ck=s["ck"],
                 iters=np.array([s["iter_count"], s["subproblem_iters"], s["adaptive_subproblem_iters"]]),
                 norms=np.array([xk.norm(), gk.norm()]), qn_size=0, qn_b0=0.0)
        qn = self.getQuasiNewton()
        if qn is not None:
            k, b0 = C.c_int(), C.c_double()
            check(lib.po_qn_get_compact(qn._h, C.byref(k), C.byref(b0), None, None, None))
            d["qn_size"], d["qn_b0"] = k.value, b0.value
        return d


class MMA(_Driver):
    """ParOptMMA (reference src/ParOptMMA.h:22-192) with its interior-point sub-solver, assembled the
    way ParOptOptimizer does for algorithm='mma'.  `options` may mix interior-point and mma_* names.
    mma_subproblem_solver='dual' solves the subproblems through their dual instead (getDualStats)."""

    _PREFIX = "mma"
    _QN_CALLBACKS = False  # (MMA takes no quasi-Newton object, user-written or not)

    def __init__(self, problem, options=None):
        self.problem = problem
        self.ctx = problem.ctx
        self._h = L.po_mma()
        check(lib.po_mma_create(problem.handle, C.byref(self._h)))
        self._cbs = []
        opts = dict(options or {})
        opts.setdefault("mma_output_file", "")
        for k, v in opts.items():
            self.setOption(k, v)

    def optimize(self):
        return self._finish_optimize(lib.po_mma_optimize(self._h))

    def getOptimizedPoint(self):
        x, z, zw, zl, zu = L.po_vec(), L.c_double_p(), L.po_vec(), L.po_vec(), L.po_vec()
        check(lib.po_mma_get_optimized_point(self._h, C.byref(x), C.byref(z), C.byref(zw), C.byref(zl), C.byref(zu)))
        c = self.problem.ncon
        wrap = lambda h: PVec(self.ctx, handle=h, owned=False) if h else None  # noqa: E731
        return wrap(x), np.array([z[i] for i in range(c)]), wrap(zw), wrap(zl), wrap(zu)

    def getAsymptotes(self):
        lo, up = L.po_vec(), L.po_vec()
        check(lib.po_mma_get_asymptotes(self._h, C.byref(lo), C.byref(up)))
        return PVec(self.ctx, handle=lo, owned=False), PVec(self.ctx, handle=up, owned=False)

    def getState(self):
        a, b, f, cons = C.c_int(), C.c_int(), C.c_double(), L.c_double_p()
        check(lib.po_mma_get_state(self._h, C.byref(a), C.byref(b), C.byref(f), C.byref(cons)))
        c = self.problem.ncon
        return dict(mma_iter=a.value, subproblem_iter=b.value, fobj=f.value, cons=np.array([cons[i] for i in range(c)]))

    def getLastRow(self):
        row = L.c_double_p()
        check(lib.po_mma_get_last_row(self._h, C.byref(row)))
        return [row[i] for i in range(5)]

    def getHistory(self):
        t = C.c_char_p()
        check(lib.po_mma_get_history(self._h, C.byref(t)))
        return t.value.decode()

    def getDualStats(self):
        """Counters of the dual sub-solver (mma_subproblem_solver='dual'): solves, accepted steps, evaluations of the
        dual function, and status / max|projected gradient| of the last solve (po_mma_get_dual_stats)."""
        a, b, e, st, pg = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(lib.po_mma_get_dual_stats(self._h, C.byref(a), C.byref(b), C.byref(e), C.byref(st), C.byref(pg)))
        return dict(solves=a.value, iterations=b.value, evaluations=e.value, last_status=st.value, last_pg=pg.value)

    def getDualGroupStats(self):
        """Of the last dual solve with mma_dual_sparse_constraints='groups' (po_mma_get_dual_group_stats): the groups
        whose multiplier is strictly inside its interval, at its lower end and at gamma; the most evaluations one
        group's root search took, the searches that hit their step cap, and the largest |psi| of a strict group."""
        a, b, g, cap = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        mx, psi = C.c_int(), C.c_double()
        check(lib.po_mma_get_dual_group_stats(self._h, C.byref(a), C.byref(b), C.byref(g), C.byref(mx), C.byref(cap),
                                              C.byref(psi)))
        return dict(strict=a.value, at_lower=b.value, at_gamma=g.value, max_inner=mx.value, cap_hits=cap.value,
                    max_psi=psi.value)

    def getGlobalizationStats(self):
        """Counters of mma_globalization='conservative' (po_mma_get_globalization_stats): raises of rho in total, in
        the last MMA iteration and the most in one, iterations that hit mma_gcmma_max_inner, and rho (ncon + 1 values,
        the objective's first) of the last accepted iteration."""
        a, b, mx, cap, rho = C.c_int(), C.c_int(), C.c_int(), C.c_int(), L.c_double_p()
        check(lib.po_mma_get_globalization_stats(self._h, C.byref(a), C.byref(b), C.byref(mx), C.byref(cap),
                                                 C.byref(rho)))
        return dict(inner_total=a.value, inner_last=b.value, inner_max=mx.value, cap_hits=cap.value,
                    rho=np.array([rho[i] for i in range(self.problem.ncon + 1)]))

    def getSubproblem(self):
        """Borrowed views of the current subproblem (po_mma_get_subproblem): dict with alpha, beta, p0, q0 (PVec),
        p, q (lists of ncon PVec) and b (numpy copy)."""
        al, be, p0, q0 = L.po_vec(), L.po_vec(), L.po_vec(), L.po_vec()
        pp, qq, b = C.POINTER(L.po_vec)(), C.POINTER(L.po_vec)(), L.c_double_p()
        check(lib.po_mma_get_subproblem(self._h, C.byref(al), C.byref(be), C.byref(p0), C.byref(q0), C.byref(pp),
                                        C.byref(qq), C.byref(b)))
        c = self.problem.ncon
        wrap = lambda h: PVec(self.ctx, handle=L.po_vec(h), owned=False)  # noqa: E731
        return dict(alpha=wrap(al.value), beta=wrap(be.value), p0=wrap(p0.value), q0=wrap(q0.value),
                    p=[wrap(pp[i]) for i in range(c)], q=[wrap(qq[i]) for i in range(c)],
                    b=np.array([b[i] for i in range(c)]))


    def getDualLinearStats(self):
        """Of mma_dual_linearized_constraints='newton' (po_mma_get_dual_linear_stats), over every pass of this solver:
        element root searches that ran into their step cap, and the most evaluations one search took."""
        cap, mx = C.c_long(), C.c_int()
        check(lib.po_mma_get_dual_linear_stats(self._h, C.byref(cap), C.byref(mx)))
        return dict(cap_hits=cap.value, max_steps=mx.value)

    def getLinearSubproblem(self):
        """Borrowed views of the current linearised subproblem (po_mma_get_linear_subproblem): dict with alpha, beta,
        p0, q0, xk (PVec), A (list of ncon PVec) and cons (numpy copy).  Inside the iteration callback of iteration k
        the move limits and p0, q0 still describe subproblem k - 1; A, cons and xk are already those of subproblem k."""
        al, be, p0, q0, xk = L.po_vec(), L.po_vec(), L.po_vec(), L.po_vec(), L.po_vec()
        aa, cons = C.POINTER(L.po_vec)(), L.c_double_p()
        check(lib.po_mma_get_linear_subproblem(self._h, C.byref(al), C.byref(be), C.byref(p0), C.byref(q0),
                                               C.byref(aa), C.byref(cons), C.byref(xk)))
        c = self.problem.ncon
        wrap = lambda h: PVec(self.ctx, handle=L.po_vec(h), owned=False)  # noqa: E731
        return dict(alpha=wrap(al.value), beta=wrap(be.value), p0=wrap(p0.value), q0=wrap(q0.value),
                    xk=wrap(xk.value), A=[wrap(aa[i]) for i in range(c)], cons=np.array([cons[i] for i in range(c)]))


def _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q, who=""):
    """m and the (ctx, m, L, U, alpha, beta, p0, q0, p[], q[]) head of the po_mma_dual_eval family's arguments."""
    m = len(p)
    if len(q) != m:
        raise ValueError(who + "p and q must hold the same number of vectors")
    pa_ = (L.po_vec * max(m, 1))(*[v.handle for v in p])
    qa_ = (L.po_vec * max(m, 1))(*[v.handle for v in q])
    return m, (ctx.handle, m, Lo.handle, Up.handle, alpha.handle, beta.handle, p0.handle, q0.handle, pa_, qa_)


def _f64(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    return a, a.ctypes.data_as(L.c_double_p)


def _f64_sized(sizes, message, *values):
    """_f64 of each array; ValueError(message) unless array i holds sizes[i] entries.  Returns the pointers."""
    pairs = [_f64(v) for v in values]
    if any(a.size != n for (a, _), n in zip(pairs, sizes)):
        raise ValueError(message)
    return [ptr for _, ptr in pairs]


def _mma_eval_outputs(m, hessian):
    """W, grad and H (None unless `hessian`) of an evaluation, and the three pointers the entries take for them."""
    W, g = C.c_double(), np.zeros(max(m, 1))
    H = np.zeros((m, m)) if hessian else None
    return W, g, H, (C.byref(W), g.ctypes.data_as(L.c_double_p),
                     H.ctypes.data_as(L.c_double_p) if hessian and m > 0 else None)


def _handles(vecs, count=3):
    """The handles of optional PVecs: of each of `vecs`, or `count` times None when there are none."""
    if vecs is None:
        return [None] * count
    return [v.handle if v is not None else None for v in vecs]


def _group_args(nwcon, nw, start, skip, a, c, nwinequality, gamma):
    return (int(nwcon), int(nw), int(start), int(skip), float(a), _handles([c])[0], int(nwinequality), float(gamma))


_LAM_RHO = "lam holds one entry per constraint, rho one more"


def mma_dual_eval(ctx, Lo, Up, alpha, beta, p0, q0, p, q, b, lam, form=0, hessian=True, point=None, xk=None, rho=None):
    """The dual function of an MMA subproblem given by caller vectors (po_mma_dual_eval): returns (W, grad, H) with
    H = minus the Hessian (None unless `hessian`).  form: 0 the library's choice, 1 fused, 2 panel.  point = (x, zl, zu)
    PVecs: also filled with the primal point and its bound multipliers at lam.
    xk (PVec) and rho (ncon + 1 values) given: the conservative approximations f~_i + rho_i d around xk
    (po_mma_dual_eval_rho); returns (W, grad, H, D) with D = d at the primal point."""
    if (xk is None) != (rho is None):
        raise ValueError("mma_dual_eval: xk and rho are given together")
    if xk is not None:
        if point is not None:
            raise ValueError("mma_dual_eval: the point of the rho form comes from mma_gcmma_point")
        return _mma_dual_eval_rho(ctx, Lo, Up, alpha, beta, p0, q0, p, q, b, lam, form, hessian, xk, rho)
    m, head = _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q, "mma_dual_eval: ")
    bp, lp = _f64_sized((m, m), "mma_dual_eval: b and lam must hold one entry per constraint", b, lam)
    W, g, H, out = _mma_eval_outputs(m, hessian)
    check(lib.po_mma_dual_eval(*head, bp, lp, int(form), *out, *_handles(point)))
    return W.value, g[:m], H


def _mma_dual_eval_rho(ctx, Lo, Up, alpha, beta, p0, q0, p, q, b, lam, form, hessian, xk, rho):
    m, head = _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q)
    lp, rp = _f64_sized((m, m + 1), _LAM_RHO, lam, rho)
    bp, = _f64_sized((m,), "mma_dual_eval: b must hold one entry per constraint", b)
    W, g, H, out = _mma_eval_outputs(m, hessian)
    D = C.c_double()
    check(lib.po_mma_dual_eval_rho(*head, bp, lp, xk.handle, rp, int(form), *out, C.byref(D)))
    return W.value, g[:m], H, D.value


def mma_dual_linear_eval(ctx, Lo, Up, alpha, beta, p0, q0, A, cons, xk, lam, xstart, form=0, hessian=True, point=None):
    """The dual function of an MMA subproblem with linearised constraints c_i = cons_i + A_i . (x - xk), given by caller
    vectors (po_mma_dual_linear_eval): returns (W, grad, H, stats) with H = minus the Hessian (None unless `hessian`)
    and stats = dict(cap_hits, max_steps) of the element root searches.  xstart (PVec) holds their starts on entry and
    x(lam) on return.  form: 0 the library's choice, 1 fused, 2 panel.  point = (x, zl, zu) PVecs: also filled with the
    primal point and its bound multipliers at lam."""
    m = len(A)
    cp, lp = _f64_sized((m, m), "mma_dual_linear_eval: cons and lam must hold one entry per constraint", cons, lam)
    cols = (L.po_vec * max(m, 1))(*[v.handle for v in A])
    W, g, H, out = _mma_eval_outputs(m, hessian)
    st = np.zeros(2)
    check(lib.po_mma_dual_linear_eval(ctx.handle, m, Lo.handle, Up.handle, alpha.handle, beta.handle, p0.handle,
                                      q0.handle, cols, cp, xk.handle, lp, int(form), xstart.handle, *out,
                                      *_handles(point), st.ctypes.data_as(L.c_double_p)))
    return W.value, g[:m], H, dict(cap_hits=int(st[0]), max_steps=int(st[1]))


def mma_dual_group_eval(ctx, Lo, Up, alpha, beta, p0, q0, p, q, b, lam, nwcon, nw, start, skip, a, c, nwinequality,
                        gamma, point, zw, hessian=True, xk=None, rho=None):
    """The dual function with grouped sparse constraints kept in it (po_mma_dual_group_eval): group i owns the variables
    start + i (nw + skip) + [0, nw), psi_i = a sum x + c[i] >= 0 (= 0 from group nwinequality on), zw_i in [0, gamma]
    ([-gamma, gamma]).  point = (x, zl, zu) PVecs and zw (PVec of nwcon, None when nwcon = 0) are filled.  Returns
    (W, grad, H, stats) with stats a dict of the group solve's counters.
    xk (PVec) and rho (ncon + 1 values) given: the conservative approximations f~_i + rho_i d around xk
    (po_mma_dual_group_eval_rho); returns (W, grad, H, stats, D) with D = d at the point."""
    if (xk is None) != (rho is None):
        raise ValueError("mma_dual_group_eval: xk and rho are given together")
    m, head = _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q, "mma_dual_group_eval: ")
    bp, lp = _f64_sized((m, m), "mma_dual_group_eval: b and lam must hold one entry per constraint", b, lam)
    W, g, H, out = _mma_eval_outputs(m, hessian)
    st = np.zeros(8)
    args = (*head, bp, lp, *_group_args(nwcon, nw, start, skip, a, c, nwinequality, gamma), *out,
            *_handles([*point, zw]), st.ctypes.data_as(L.c_double_p))
    if xk is None:
        check(lib.po_mma_dual_group_eval(*args))
        return W.value, g[:m], H, _group_stats(st)
    rp, = _f64_sized((m + 1,), "mma_dual_group_eval: rho holds one entry per constraint and one more", rho)
    D = C.c_double()
    check(lib.po_mma_dual_group_eval_rho(*args, xk.handle, rp, C.byref(D)))
    return W.value, g[:m], H, _group_stats(st), D.value


def _group_stats(st):
    return dict(strict=int(st[0]), at_lower=int(st[1]), at_gamma=int(st[2]), cap_hits=int(st[3]), steps=int(st[4]),
                max_inner=int(st[5]), max_psi=float(st[6]), zw_psi=float(st[7]))


def mma_gcmma_group_point(ctx, Lo, Up, alpha, beta, p0, q0, p, q, lam, nwcon, nw, start, skip, a, c, nwinequality,
                          gamma, xk, rho, point, zw):
    """The point of a conservative trial with grouped sparse constraints (po_mma_gcmma_group_point): the group solve
    at lam for the approximations f~_i + rho_i d around xk fills point = (x, zl, zu) and zw; returns (sums, stats)
    with the m + 2 sums [Delta_0, Delta_1..m, D] of mma_gcmma_point at that x."""
    m, head = _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q, "mma_gcmma_group_point: ")
    lp, rp = _f64_sized((m, m + 1), _LAM_RHO, lam, rho)
    sums, st = np.zeros(m + 2), np.zeros(8)
    check(lib.po_mma_gcmma_group_point(*head, lp, *_group_args(nwcon, nw, start, skip, a, c, nwinequality, gamma),
                                       xk.handle, rp, *_handles([*point, zw]), sums.ctypes.data_as(L.c_double_p),
                                       st.ctypes.data_as(L.c_double_p)))
    return sums, _group_stats(st)


def mma_gcmma_point(ctx, Lo, Up, alpha, beta, p0, q0, p, q, lam, xk, rho, point):
    """The point pass of a conservative inner iteration (po_mma_gcmma_point): fills point = (x, zl, zu) PVecs at lam
    and returns the m + 2 sums [Delta_0, Delta_1..m, D]."""
    m, head = _mma_subproblem_args(ctx, Lo, Up, alpha, beta, p0, q0, p, q)
    lp, rp = _f64_sized((m, m + 1), _LAM_RHO, lam, rho)
    sums = np.zeros(m + 2)
    check(lib.po_mma_gcmma_point(*head, lp, xk.handle, rp, *_handles(point), sums.ctypes.data_as(L.c_double_p)))
    return sums


def mma_gcmma_rho_sums(ctx, Lo, Up, g, A):
    """The m + 1 sums behind the start values of rho (po_mma_gcmma_rho_sums): sum |g| (U - L), then sum |A_i| (U - L)
    per constraint."""
    m = len(A)
    arr = (L.po_vec * max(m, 1))(*[v.handle for v in A])
    sums = np.zeros(m + 1)
    check(lib.po_mma_gcmma_rho_sums(ctx.handle, m, Lo.handle, Up.handle, g.handle, arr,
                                    sums.ctypes.data_as(L.c_double_p)))
    return sums


def wgram(d, vecs, rhs_last=False):
    """W = P^T diag(d) P; rhs_last: the last vector is pre-weighted (its row / column are plain dots)."""
    nv = len(vecs)
    W = np.zeros((nv, nv))
    arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
    fn = lib.po_wgram_with_rhs if rhs_last else lib.po_wgram
    check(fn(d.handle, arr, nv, W.ctypes.data_as(L.c_double_p)))
    return W.T  # column-major symmetric


def xgram(U, Z):
    """X = U^T Z for two panels of equally many vectors of equal length: X[r, s] = U[r] . Z[s], one pass over both
    panels (po_xgram)."""
    nv = len(U)
    if len(Z) != nv:
        raise ValueError("xgram: the two panels must have the same number of vectors")
    X = np.zeros((nv, nv))
    ua = (L.po_vec * max(nv, 1))(*[v.handle for v in U])
    za = (L.po_vec * max(nv, 1))(*[v.handle for v in Z])
    check(lib.po_xgram(ua, za, nv, X.ctypes.data_as(L.c_double_p)))
    return X.T  # out[r + nv * s] is column-major


def group_panel(d, vecs, nwcon, nw, skip, alpha, U):
    """U_j = alpha * (sums of d o vecs_j over groups of nw consecutive variables, period nw + skip): the structured
    sparse-Jacobian panel image in a pass of its own."""
    nv = len(vecs)
    arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
    uarr = (L.po_vec * max(nv, 1))(*[u.handle for u in U])
    check(lib.po_group_panel(d.handle, arr, nv, nwcon, nw, skip, alpha, uarr))


def wgram_with_groups(d, vecs, nwcon, nw, skip, alpha, U, rhs_last=False):
    """wgram() with the panel image of the first len(U) columns riding in the same pass; returns (W, fused)."""
    nv = len(vecs)
    W = np.zeros((nv, nv))
    arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
    uarr = (L.po_vec * max(len(U), 1))(*[u.handle for u in U])
    fused = C.c_int(0)
    check(lib.po_wgram_with_groups(d.handle, arr, nv, 1 if rhs_last else 0, nwcon, nw, skip, alpha, uarr, len(U),
                                   W.ctypes.data_as(L.c_double_p), C.byref(fused)))
    return W.T, bool(fused.value)


def bench_mdot(x, vecs, reps=10):
    nv = len(vecs)
    arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
    ms = C.c_double()
    out = np.zeros(max(nv, 1))
    check(lib.po_bench_mdot(x.handle, arr, nv, int(reps), C.byref(ms), out.ctypes.data_as(L.c_double_p)))
    return ms.value, out[:nv]


def bench_kernels(ctx, n, c, k, reps=5):
    """Every hot kernel of an interior-point iteration timed in isolation (po_bench_kernels): list of dicts."""
    import json

    buf = C.create_string_buffer(16384)
    check(lib.po_bench_kernels(ctx.handle, int(n), int(c), int(k), int(reps), buf, len(buf)))
    return json.loads(buf.value.decode())


def bench_vec_api(ctx, n, reps=10):
    """Roofline rows of the vector API and the quasi-Newton products at size n (po_bench_vec_api): list of dicts."""
    import json

    buf = C.create_string_buffer(32768)
    check(lib.po_bench_vec_api(ctx.handle, int(n), int(reps), buf, len(buf)))
    return json.loads(buf.value.decode())


def bench_mma_dual(ctx, n, m, form, reps=5):
    """(pass ms, Gram ms, ms of the trivial kernel of the pass's stream mix) of one evaluation of the MMA dual at
    (n, m) on synthetic data (po_bench_mma_dual); form 1 fused (m <= 8), 2 panel."""
    a, g, b = C.c_double(), C.c_double(), C.c_double()
    check(lib.po_bench_mma_dual(ctx.handle, int(n), int(m), int(form), int(reps), C.byref(a), C.byref(g), C.byref(b)))
    return a.value, g.value, b.value


def bench_mma_dual_linear(ctx, n, m, form, reps=5):
    """The dual pass with linearised constraints on synthetic data (po_bench_mma_dual_linear): (warm ms, cold ms,
    gram ms, ceiling ms, [most root-search evaluations warm, cold]); warm starts every root search from the point of
    the call before, cold from the expansion point."""
    w, c, g, b = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    st = (C.c_double * 2)()
    check(lib.po_bench_mma_dual_linear(ctx.handle, int(n), int(m), int(form), int(reps), C.byref(w), C.byref(c),
                                       C.byref(g), C.byref(b), st))
    return w.value, c.value, g.value, b.value, [int(st[0]), int(st[1])]


def bench_mma_dual_rho(ctx, n, m, form, reps=5):
    """The dual pass and its rho form alternating in one call (po_bench_mma_dual_rho): ([plain ms] * 2, [rho ms] * 2,
    Gram ms, ms of the trivial kernel of the rho form's stream mix, 2m + 7 in)."""
    a, r, g, b = (C.c_double * 2)(), (C.c_double * 2)(), C.c_double(), C.c_double()
    check(lib.po_bench_mma_dual_rho(ctx.handle, int(n), int(m), int(form), int(reps), a, r, C.byref(g), C.byref(b)))
    return list(a), list(r), g.value, b.value


def bench_stream(x, y, kind, reps=10):
    """Average kernel ms of a read-only stream (kind 0: x.y) or a copy (kind 1: y <- x), HIP events."""
    ms = C.c_double()
    check(lib.po_bench_stream(x.handle, y.handle, int(kind), int(reps), C.byref(ms)))
    return ms.value


def bench_wgram(d, vecs, reps=10):
    nv = len(vecs)
    arr = (L.po_vec * max(nv, 1))(*[v.handle for v in vecs])
    ms = C.c_double()
    check(lib.po_bench_wgram(d.handle, arr, nv, int(reps), C.byref(ms)))
    return ms.value
