"""CPU checks of the zero-copy tensor boundary (po_vec_to_dlpack, po_ctx_device, paropt_amd.TorchProblem): NULL handles
are refused, the DLPack structs have the layout of dlpack.h, and importing the package does not import torch."""
import ctypes as C
import subprocess
import sys

from conftest import ROOT


def test_new_entry_points_refuse_null_handles():
    import paropt_amd.lib as L

    lib = L.lib
    mt = C.POINTER(L.DLManagedTensor)()
    assert lib.po_vec_to_dlpack(None, C.byref(mt)) == 2  # PO_ERR_ARG
    assert not mt
    assert b"null" in lib.po_last_error()
    d = C.c_int(-7)
    assert lib.po_ctx_device(None, C.byref(d)) == 2  # PO_ERR_ARG
    assert d.value == -7
    assert b"null" in lib.po_last_error()


def test_dlpack_struct_layout():
    """DLTensor / DLManagedTensor of the unversioned DLPack ABI on a 64-bit host."""
    import paropt_amd.lib as L

    assert C.sizeof(L.DLDevice) == 8 and C.sizeof(L.DLDataType) == 4
    assert C.sizeof(L.DLTensor) == 48
    assert [getattr(L.DLTensor, f).offset for f in ("data", "device", "ndim", "dtype", "shape", "strides",
                                                    "byte_offset")] == [0, 8, 16, 20, 24, 32, 40]
    assert C.sizeof(L.DLManagedTensor) == 64
    assert (L.DLManagedTensor.manager_ctx.offset, L.DLManagedTensor.deleter.offset) == (48, 56)
    assert (L.DL_ROCM, L.DL_FLOAT) == (10, 2)


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import paropt_amd; "
            "assert hasattr(paropt_amd, 'TorchProblem'); "
            "from paropt_amd import ParOpt; assert hasattr(ParOpt, 'TorchProblem'); "
            "print('torch' in sys.modules)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False"
