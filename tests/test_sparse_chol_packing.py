"""Packed groups of tiny fronts in the sparse Cholesky analysis (sparse_chol.cpp), without a device: the grouping rule
against a numpy restatement, its invariants, the launch schedule as kernel_forms reports it, and the arena layout."""
import numpy as np
import pytest

from csr_helpers import chain_pattern, grid_pattern
from sparse_chol_packing_helpers import CAPS, DEFAULT_CAP, TINY, analysis, groups_by_rule, pack_cap

NAMES = ["tridiag70", "tridiag4096", "forest", "grid12", "grid40", "arrow", "clique8"]
PACK_FORMS = ("pack_factor", "pack_fwd", "pack_bwd")


def launch_level(s, p):
    """the level whose launches run each front: its group's, or its own"""
    lev = s.snode_level.copy()
    for f, r, l in zip(p["group_first"], p["group_root"], p["group_level"]):
        lev[f:r + 1] = l
    return lev


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", NAMES)
def test_groups_follow_the_rule(name, cap):
    s = analysis(name, cap)
    p = s.packing()
    assert (p["tiny"], p["cap"]) == (TINY, cap)
    nsn = s.num_snodes
    s_of = np.diff(s.snode_first)
    assert len(p["front_order"]) == nsn and (p["front_order"] >= s_of).all()
    assert p["front_order"].max() == s.max_front
    first, root, cand = groups_by_rule(s.snode_first, s.snode_parent, p["front_order"], cap)
    np.testing.assert_array_equal(p["group_first"], first)
    np.testing.assert_array_equal(p["group_root"], root)
    np.testing.assert_array_equal(p["group_level"], s.snode_level[root])
    assert p["num_groups"] == len(root)
    # invariants, stated on what the library returned
    gf, gr = p["group_first"], p["group_root"]
    assert (gf <= gr).all() and (gf[1:] > gr[:-1]).all()  # disjoint contiguous ranges
    member = np.full(nsn, -1)
    for g, (f, r) in enumerate(zip(gf, gr)):
        member[f:r + 1] = g
        assert r - f + 1 <= cap
        par = s.snode_parent[f:r]
        assert ((par > np.arange(f, r)) & (par <= r)).all()  # closed under "child of": every parent inside
        if r > f:
            P = s.snode_parent[r]
            assert P < 0 or not cand[P]
    kids_in = member[np.nonzero(s.snode_parent >= 0)[0]]
    par_in = member[s.snode_parent[s.snode_parent >= 0]]
    # a child of a multi-front group's member is a member: the group is the whole subtree of its root
    multi = np.isin(par_in, np.nonzero(gr > gf)[0])
    assert (kids_in[multi] == par_in[multi]).all()
    tiny = p["front_order"] <= TINY
    assert (member[tiny] >= 0).all() and (member[~tiny] == -1).all()


def test_arrow_has_a_large_child_under_a_tiny_parent():
    s = analysis("arrow", 16)
    p = s.packing()
    assert list(np.diff(s.snode_first)) == [10, 1, 2] and list(p["front_order"]) == [11, 2, 2]
    assert list(p["group_first"]) == [1, 2] and list(p["group_root"]) == [1, 2]


def test_clique8_has_children_that_carry_all_rows_of_a_tiny_front():
    s = analysis("clique8", 16)
    p = s.packing()
    assert list(np.diff(s.snode_first)) == [1, 1, 8] and list(p["front_order"]) == [9, 9, 8]
    assert list(s.snode_parent) == [2, 2, -1]
    assert list(p["group_first"]) == [2] and list(p["group_root"]) == [2]
    assert s.kernel_forms() == {"assemble": 1, "small": 1, "blocked": 0, "pack_factor": 1, "fwd": 1, "bwd": 1,
                                "pack_fwd": 1, "pack_bwd": 1}


def test_tridiagonal_4096_schedule():
    """Nested dissection leaves 512 leaf sets of eight vertices, each a chain of one-column fronts; cap 16 packs all
    3840 fronts of levels 0 - 8 into 256 groups rooted on levels 7 and 8, so levels 0 - 6 launch nothing."""
    s = analysis("tridiag4096", 16)
    p = s.packing()
    assert p["cap"] == 16 and s.num_snodes == 4095 and s.nlevels == 17
    size = p["group_root"] - p["group_first"] + 1
    multi = size > 1
    assert int(multi.sum()) == 256 and int(size[multi].sum()) == 3840
    assert sorted(set(p["group_level"][multi])) == [7, 8]
    lev = launch_level(s, p)
    assert int((s.snode_level <= 8).sum()) == 3840 and (lev[s.snode_level <= 8] >= 7).all()
    assert lev.min() == 7
    assert p["factor_levels"] == 10
    forms = s.kernel_forms()
    assert forms == {"assemble": 0, "small": 0, "blocked": 0, "pack_factor": 10, "fwd": 0, "bwd": 0, "pack_fwd": 10,
                     "pack_bwd": 10}
    assert s.kernel_forms(33)["pack_fwd"] == 20  # two slabs of right-hand sides


def test_grid_40_mixes_both_kinds():
    s = analysis("grid40", 16)
    p = s.packing()
    forms = s.kernel_forms()
    assert s.num_snodes == 1130 and s.nlevels == 23
    assert forms["pack_factor"] > 0 and forms["small"] > 0 and forms["blocked"] > 0 and forms["assemble"] > 0
    assert forms["fwd"] == forms["bwd"] and forms["pack_fwd"] == forms["pack_bwd"] == forms["pack_factor"]
    assert p["factor_levels"] <= s.nlevels
    lev = launch_level(s, p)
    assert p["factor_levels"] == len(set(lev))


@pytest.mark.parametrize("name", NAMES)
def test_cap_0_is_the_unpacked_engine(name):
    s = analysis(name, 0)
    p = s.packing()
    assert p["cap"] == 0 and p["num_groups"] == 0 and len(p["group_first"]) == 0
    forms = s.kernel_forms(5)
    assert all(forms[f] == 0 for f in PACK_FORMS)
    assert forms["fwd"] == forms["bwd"] == s.nlevels and p["factor_levels"] == s.nlevels
    # and the analysis itself does not depend on the cap
    t = analysis(name, 16)
    for a in ("perm", "snode_first", "snode_parent", "snode_level"):
        np.testing.assert_array_equal(getattr(s, a), getattr(t, a))
    assert (s.nnzL, s.nlevels, s.max_front) == (t.nnzL, t.nlevels, t.max_front)


@pytest.mark.parametrize("cap", (0,) + CAPS)
@pytest.mark.parametrize("name", NAMES)
def test_arena_slots_live_together_do_not_overlap(name, cap):
    """A front's update matrix is written in the launches of its level (its group's level when packed) and read in
    those of its parent's: from the first to the second it shares the arena with nothing."""
    s = analysis(name, cap)
    p = s.packing()
    b = p["front_order"] - np.diff(s.snode_first)
    size = ((b + 1) // 2 * 2).astype(np.int64) * b
    born = launch_level(s, p)
    dies = np.where(s.snode_parent >= 0, born[np.maximum(s.snode_parent, 0)], born)
    assert (dies >= born).all()
    assert ((size == 0) == (s.snode_parent < 0)).all()
    assert (p["upd_off"] >= 0).all() and ((p["upd_off"] + size) * 8 <= s.work_bytes).all()
    for l in range(s.nlevels):
        live = np.nonzero((born <= l) & (l <= dies) & (size > 0))[0]
        order = live[np.argsort(p["upd_off"][live], kind="stable")]
        end = p["upd_off"][order] + size[order]
        assert (end[:-1] <= p["upd_off"][order][1:]).all(), (l, name, cap)


def test_csr_symbolic_accessors():
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    rowp, cols = chain_pattern(201, 2, 1)
    with pack_cap(16):
        mf = pa.CsrSymbolic(201, rowp, cols, sparse_factor="multifrontal")
    p = mf.frontal_packing()
    first, root, _ = groups_by_rule(mf.snode_first, mf.snode_parent, p["front_order"], 16)
    np.testing.assert_array_equal(p["group_first"], first)
    np.testing.assert_array_equal(p["group_root"], root)
    assert p["cap"] == 16 and (root > first).any()
    forms = mf.frontal_kernel_forms(33)
    assert forms["pack_factor"] == p["factor_levels"] > 0 and forms["pack_fwd"] == 2 * forms["pack_factor"]
    with pack_cap(0):
        off = pa.CsrSymbolic(201, rowp, cols, sparse_factor="multifrontal")
    assert off.frontal_packing()["num_groups"] == 0 and off.frontal_kernel_forms()["pack_factor"] == 0
    assert off.frontal_kernel_forms()["small"] == off.nlevels
    with pytest.raises(ParOptAMDError):
        mf.kernel_forms()  # (the row factor's forms: still refused)
    rows = pa.CsrSymbolic(100, *grid_pattern(10, 10))
    with pytest.raises(ParOptAMDError):
        rows.frontal_packing()
    with pytest.raises(ParOptAMDError):
        rows.frontal_kernel_forms()
    with pytest.raises(ParOptAMDError):
        mf.frontal_kernel_forms(0)


def test_the_switch_is_back_at_its_default():
    assert analysis("tridiag70", None).packing()["cap"] == DEFAULT_CAP
