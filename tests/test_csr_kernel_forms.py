"""CPU: which kernel form every elimination level of the CSR sparse Cholesky launches (CsrSymbolic.kernel_forms, the
function the device solver itself launches by), on patterns built to sit on either side of each selector, and that
the patterns of the suite together plan every form.  No device needed.

Not reached: `level:thin` for the FACTORIZATION through its second clause (at least 65536 ordinary rows of 25..96
entries in one level, w of about 1.7 M).  The kernel is the one short rows already run, so it is left out on purpose;
the same clause of the triangular sweeps counts rows times right-hand sides and is reached (arrow_blocks at nv = 64)."""
import numpy as np
import pytest

from paropt_amd import CsrSymbolic

from csr_helpers import (arrow_blocks_pattern, arrow_pattern, dense_jacobian, emulate_factor, grid_pattern,
                         shared_pattern)

NEW_PATTERNS = {
    "arrow_2049_1": lambda: (2049, *arrow_pattern(2049, 1)),
    "arrow_2047_1": lambda: (2047, *arrow_pattern(2047, 1)),
    "arrow_256_16": lambda: (256, *arrow_pattern(256, 16)),
    "arrow_255_16": lambda: (255, *arrow_pattern(255, 16)),
    "arrow_2049_16": lambda: (2049, *arrow_pattern(2049, 16)),
    "arrow_2048_16": lambda: (2048, *arrow_pattern(2048, 16)),
    "arrow_2049_15": lambda: (2049, *arrow_pattern(2049, 15)),
    "shared_2049": lambda: (2050, *shared_pattern(2049)),
    "shared_2048": lambda: (2049, *shared_pattern(2048)),
    "arrow_blocks_1024_25": lambda: (1024 * 25, *arrow_blocks_pattern(1024, 25)),
    "arrow_blocks_1023_25": lambda: (1023 * 25, *arrow_blocks_pattern(1023, 25)),
}
_SYM = {}


def symbolic(name):
    """analysed once per pattern (shared_2049 takes half a second)"""
    if name not in _SYM:
        _SYM[name] = CsrSymbolic(*NEW_PATTERNS[name]())
    return _SYM[name]


def used(name, nv=1):
    return {k: v for k, v in symbolic(name).kernel_forms(nv).items() if v > 0}


def factor_forms(forms):
    return {k: v for k, v in forms.items() if not k.startswith("trsv")}


# pattern -> (w, nnz(L), forms of the factorization with the number of levels)
TABLE = {
    "arrow_2049_1": (2050, 4099, {"level:thin": 1, "level:search": 1}),
    "arrow_2047_1": (2048, 4095, {"level:thin": 1, "level:table": 1}),
    "arrow_256_16": (272, 4488, {"level:thin": 1, "front_rows:wide": 1, "front_syrk:table": 1, "front_dense:lds": 1}),
    "arrow_255_16": (271, 4471, {"level:thin": 1, "front_rows:table": 1, "front_syrk:table": 1, "front_dense:lds": 1}),
    "arrow_2049_16": (2065, 34969,
                      {"level:thin": 1, "front_rows:search": 1, "front_syrk:search": 1, "front_dense:lds": 1}),
    "arrow_2048_16": (2064, 34952,
                      {"level:thin": 1, "front_rows:wide": 1, "front_syrk:table": 1, "front_dense:lds": 1}),
    "arrow_2049_15": (2064, 32904, {"level:thin": 1, "level:search": 15}),
    "shared_2049": (2049, 2100225, {"front_rows:table": 1, "front_syrk:table": 1, "front_dense:global": 1}),
    "shared_2048": (2048, 2098176, {"front_rows:table": 1, "front_syrk:table": 1, "front_dense:lds": 1}),
    "arrow_blocks_1024_25": (26624, 52224, {"level:thin": 1, "level:table": 1}),
    "arrow_blocks_1023_25": (26598, 52173, {"level:thin": 1, "level:table": 1}),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_factor_forms_on_either_side_of_each_selector(name):
    w, nnzL, forms = TABLE[name]
    sym = symbolic(name)
    assert len(sym.perm) == w and sym.nnzL == nnzL
    assert factor_forms(used(name)) == forms
    assert factor_forms(used(name, 5)) == forms  # the factorization does not depend on the panel width
    if name == "arrow_2049_15":  # 15 < 16 rows: no front, one level per long row, each with predecessors
        assert sym.nfronts == 0 and sym.nlevels == 16
    if name.startswith("shared"):
        assert sym.nfronts == 1 and sym.max_front == w


def sweeps(forms):
    return {k: v for k, v in forms.items() if k.startswith("trsv")}


def test_sweep_forms_of_the_long_rows():
    # one row of 2050 entries after 2049 single-entry rows: a wavefront for it forward, and every column is short
    assert sweeps(used("arrow_2049_1")) == {"trsv_fwd:thin": 1, "trsv_fwd:wave": 1, "trsv_bwd:thin": 2}
    assert sweeps(used("arrow_2049_1", 5)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave_split": 1, "trsv_bwd:thin": 2}
    assert sweeps(used("arrow_2049_15", 5)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave_split": 15, "trsv_bwd:thin": 16}
    # a front has no ordinary rows: its sweeps are the front kernels, not a trsv form
    assert sweeps(used("shared_2049", 5)) == {}


def test_sweep_forms_by_rows_and_panel_width():
    """Level 1 of arrow_blocks(1024, 25) has 1024 ordinary rows of 26 entries: at least 1024 rows keep the wave form
    unsplit, 65536 (row, right-hand side) items make it thin; one block less and the wave form splits."""
    name = "arrow_blocks_1024_25"
    for nv in (1, 4):  # (up to four right-hand sides never split)
        assert sweeps(used(name, nv)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave": 1, "trsv_bwd:thin": 2}
    for nv in (5, 8, 63):
        assert sweeps(used(name, nv)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave": 1, "trsv_bwd:thin": 2}
    assert sweeps(used(name, 64)) == {"trsv_fwd:thin": 2, "trsv_bwd:thin": 2}
    assert sweeps(used("arrow_blocks_1023_25", 8)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave_split": 1,
                                                       "trsv_bwd:thin": 2}
    assert sweeps(used("arrow_blocks_1023_25", 4)) == {"trsv_fwd:thin": 1, "trsv_fwd:wave": 1, "trsv_bwd:thin": 2}


def test_panel_slabs_are_planned_one_by_one():
    """A panel wider than one kernel's pointer table (96) goes in slabs; a level counts the forms of every slab."""
    sym = CsrSymbolic(26 * 24, *grid_pattern(26, 24))
    f96, f97, f130 = (sym.kernel_forms(nv) for nv in (96, 97, 130))
    assert f96["trsv_fwd:wave"] == 0 and f96["trsv_fwd:wave_split"] > 0 and f96["trsv_bwd:wave_split"] > 0
    # 97 = 96 + 1: the last slab is a single right-hand side, which does not split
    assert f97["trsv_fwd:wave"] == f97["trsv_fwd:wave_split"] == f96["trsv_fwd:wave_split"]
    assert f97["trsv_bwd:wave"] == f97["trsv_bwd:wave_split"] == f96["trsv_bwd:wave_split"]
    assert f130 == f96  # 96 + 34
    f1 = sym.kernel_forms(1)
    assert f1["trsv_fwd:wave"] > 0 and f1["trsv_bwd:wave"] > 0 and f1["level:table"] > 0 and f1["front_dense:lds"] > 0
    assert sum(f1[k] for k in ("level:thin", "level:table", "level:search")) <= sym.nlevels
    with pytest.raises(Exception):
        sym.kernel_forms(0)


def test_every_form_is_planned_by_some_pattern_of_the_suite():
    """The patterns of test_gpu_csr.py and the ones above, at the panel widths test_gpu_csr_forms.py uses, plan every
    form the accessor knows (the accessor defines the list).  `level:thin` is in it through short rows; its second
    clause for the factorization is out of reach of a test (see the module docstring)."""
    from test_gpu_csr import PATTERNS

    names = set(symbolic("arrow_2047_1").kernel_forms())
    assert len(names) == 16
    seen = set()
    for make in PATTERNS.values():
        sym = CsrSymbolic(*make())
        for nv in (1, 5):
            seen |= {k for k, v in sym.kernel_forms(nv).items() if v > 0}
    old = set(seen)
    for name in NEW_PATTERNS:
        for nv in (1, 5, 8, 64):
            seen |= set(used(name, nv))
    assert seen == names, names - seen
    # what the new patterns add to the suite
    assert names - old == {"level:search", "front_rows:wide", "front_rows:search", "front_syrk:search",
                           "front_dense:global"}


@pytest.mark.parametrize("make", [lambda: (40, *arrow_pattern(40, 16)), lambda: (40, *arrow_pattern(40, 15)),
                                  lambda: (18, *shared_pattern(17))], ids=["arrow_40_16", "arrow_40_15", "shared_17"])
def test_emulated_factor_on_the_new_patterns(make):
    n, rowp, cols = make()
    w = len(rowp) - 1
    sym = CsrSymbolic(n, rowp, cols)
    rng = np.random.default_rng(0)
    A = dense_jacobian(n, rowp, cols, rng.uniform(0.5, 1.5, size=int(rowp[-1])))
    S = np.diag(rng.uniform(0.1, 1.0, size=w)) + (A * rng.uniform(0.5, 2.0, size=n)) @ A.T
    L, Sp = emulate_factor(sym, S)
    np.testing.assert_allclose(L @ L.T, Sp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(L, np.linalg.cholesky(Sp), rtol=1e-10, atol=1e-12)
