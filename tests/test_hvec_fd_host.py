"""CPU checks of the differenced Hessian-vector products (InteriorPoint.setHvecFiniteDifference): the C header, the
ctypes table and the Python layer agree on the new entry points, and the new kernels are in the device assembly without
scratch memory or spilled registers."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = {
    "po_ip_set_hvec_finite_difference": (C.c_int, ["po_ip", C.c_int, C.c_int, C.c_double]),
    "po_ip_get_hvec_fd_count": (C.c_int, ["po_ip", "int*", "int*"]),
    "po_ip_get_hvec_fd_step": (C.c_int, ["po_ip", "double*"]),
    "po_ip_eval_hvec": (C.c_int, ["po_ip", "double*", "po_vec", "po_vec", "po_vec"]),
}


def header_text():
    return open(os.path.join(ROOT, "include", "paropt_amd.h")).read()


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import paropt_amd.lib as L

    named = {"po_ip": L.po_ip, "po_vec": L.po_vec, "int*": L.c_int_p, "double*": L.c_double_p}
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for name, (res, args) in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "include/paropt_amd.h does not declare %s" % name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hasattr(L.lib, name), "libparopt_amd.so does not export %s" % name
        sig = L.SIGNATURES[name]
        assert sig[0] is res and list(sig[1]) == [named.get(a, a) for a in args], (name, sig)


def test_mode_constants_are_the_headers():
    import paropt_amd as pa

    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"enum\s*\{\s*PO_HVEC_EXACT\s*=\s*(\d+)\s*,\s*PO_HVEC_FD_WHEN_MISSING\s*=\s*(\d+)\s*,\s*"
                  r"PO_HVEC_FD_ALWAYS\s*=\s*(\d+)\s*\}", code)
    assert m, "the PO_HVEC_* enumeration is missing from include/paropt_amd.h"
    assert pa.InteriorPoint.HVEC_MODES == {"exact": int(m.group(1)), "when_missing": int(m.group(2)),
                                           "always": int(m.group(3))}
    from paropt_amd import ParOpt

    for name in ("setHvecFiniteDifference", "getHvecFiniteDifferenceCount", "getHvecFiniteDifferenceStep", "evalHvec"):
        assert callable(getattr(pa.InteriorPoint, name)) and callable(getattr(ParOpt.InteriorPoint, name))
    facade = open(os.path.join(ROOT, "include", "ParOptAMD.hpp")).read()
    for name in ("setHvecFiniteDifference", "getHvecFiniteDifferenceCount", "evalHvec"):
        assert re.search(r"\b%s\s*\(" % name, facade), name


def test_null_solver_handle_is_refused():
    import paropt_amd.lib as L

    a, b, h = C.c_int(), C.c_int(), C.c_double()
    assert L.lib.po_ip_set_hvec_finite_difference(None, 1, 0, 0.0) != 0
    assert L.lib.po_ip_get_hvec_fd_count(None, C.byref(a), C.byref(b)) != 0
    assert L.lib.po_ip_get_hvec_fd_step(None, C.byref(h)) != 0
    assert L.lib.po_ip_eval_hvec(None, None, None, None, None) != 0
    assert len(L.lib.po_last_error()) > 0


def test_new_kernels_use_no_scratch():
    from test_kernel_resources import kernel_metadata

    meta = kernel_metadata()
    for pat, at_least in ((r"hvec_fd_prepare_kernel", 1), (r"hvec_fd_combine_kernelILi\d+E", 2)):
        hits = {n: v for n, v in meta.items() if re.search(pat, n)}
        assert len(hits) >= at_least, (pat, sorted(hits))
        for n, v in hits.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
            assert v["vgpr_count"] <= 128, (n, v)  # two workgroups per CU and more fit
    # the perturbed point is the existing panel axpy: no kernel of its own
    assert not [n for n in meta if re.search(r"hvec_fd_(point|perturb)", n)]
