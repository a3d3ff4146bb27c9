"""GPU: a problem owns one quasi-definite solver object per form of its sparse constraints (quasidef.hpp), replaced
where the form can change.  Every comparison is == on bytes: both sides are the same library.

The library's breakdown count and the count of grouped-to-CSR fallbacks have no reader in the C ABI; they are asserted
through what they decide: po_quasidef_factor reports a breakdown exactly when the count of the solver in charge rose,
and the fallback is announced on stderr the first time only.
"""
import numpy as np
import pytest

import sparse_forms_helpers as H
from test_gpu_quasidef_user import BlockSolver, DenseSolver, DiagonalSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def _weighting_jacobian():
    return H.po.SepProblem("convex", H.N, 2, nwcon=60, nw=H.NW).sparse_jacobian_dense()


FORMS = {
    "grouped": (lambda ctx: H.grouped(ctx), lambda p: DiagonalSolver(_weighting_jacobian()), "nblock: 1"),
    "block3": (lambda ctx: H.block(ctx, 3), lambda p: BlockSolver(H.block_jacobian(3), 3), "nblock: 3"),
    "csr": (lambda ctx: H.csr_chain(ctx), DenseSolver, "nnz(L)"),
}


class FailingFactor:
    """a user solver whose factor reports failure: only its own breakdown count moves"""

    def factor(self, x, dinv, cdiag):
        return 7

    def apply(self, bx, bw, yx, yw):
        return 0


@pytest.mark.parametrize("form", sorted(FORMS))
def test_attach_then_detach_brings_the_library_form_back(ctx, form):
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    build, user, info = FORMS[form]
    p = H.upload_entries(build(ctx))
    before = H.factor_and_apply(ctx, p)
    assert info in pa.quasidef_factor_info(p)
    p.setQuasiDefMat(user(p))
    with_user = H.factor_and_apply(ctx, p)
    assert np.isfinite(np.frombuffer(with_user[1])).all()
    assert info not in (pa.quasidef_factor_info(p) or "")
    p.setQuasiDefMat(FailingFactor())
    with pytest.raises(ParOptAMDError, match="failed factorization \\(7\\)"):  # the user's count rose
        H.factor_and_apply(ctx, p)
    p.setQuasiDefMat(None)
    assert info in pa.quasidef_factor_info(p)
    assert H.factor_and_apply(ctx, p) == before  # ... and the count read now is the library form's, which did not


def test_both_ways_into_the_grouped_form_take_the_fused_solver(ctx):
    """setWeighting and a recognised CSR pattern: equal bits and equal launches.  The grouped solver factors in one
    launch (group sum and reciprocal) and applies in one (the map tiles) or three; the scalar solver through the
    Jacobian hooks gives the same bits in two and seven, so only the launch count tells which one answered."""
    runs = []
    for build in (H.grouped, H.csr_groups):
        launches = []
        runs.append((H.factor_and_apply(ctx, H.upload_entries(build(ctx)), launches=launches), launches))
    assert runs[0] == runs[1]
    assert runs[0][1][0] == 1 and runs[0][1][1] in (1, 3), runs[0][1]


def test_block_size_round_trip(ctx):
    import paropt_amd as pa

    p = H.block(ctx, 2)
    first = H.factor_and_apply(ctx, p)
    assert H.set_block_size(p, 1) == 0 and pa.quasidef_factor_info(p) == "nblock: 1"
    assert H.factor_and_apply(ctx, p) != first
    assert H.set_block_size(p, 2) == 0 and pa.quasidef_factor_info(p) == "nblock: 2"
    assert H.factor_and_apply(ctx, p) == first


def test_refused_block_size_keeps_the_previous_solver(ctx):
    import paropt_amd as pa

    p = H.block(ctx, 2)
    first = H.factor_and_apply(ctx, p)
    assert H.set_block_size(p, 7) != 0  # 7 does not divide 60
    assert pa.quasidef_factor_info(p) == "nblock: 2"
    assert H.factor_and_apply(ctx, p) == first


def test_fallback_swaps_in_the_csr_solver_once(ctx, capfd):
    import paropt_amd as pa

    p = H.csr_groups(ctx, differ_after=3)
    ip = pa.InteriorPoint(p, {"max_major_iters": 0})
    ip.optimize()
    assert pa.quasidef_factor_info(p) == "nblock: 1"  # recognised: the grouped scalar form
    capfd.readouterr()
    pa.InteriorPoint(p, H.IP_OPTS).optimize()  # the entries differ from the fourth gradient evaluation on
    assert p.ngrad > 3
    assert "nnz(L)" in pa.quasidef_factor_info(p)
    pa.InteriorPoint(p, H.IP_OPTS).optimize()  # for good: nothing is given up a second time
    assert "nnz(L)" in pa.quasidef_factor_info(p)
    assert capfd.readouterr().err.count("general CSR path") == 1


class Recording(DiagonalSolver):
    """counts the calls and notes the point every factor is made at, with the number of gradient evaluations so far"""

    def __init__(self, problem):
        super().__init__(_weighting_jacobian())
        self.problem, self.factors, self.napply = problem, [], 0

    def factor(self, x, dinv, cdiag):
        self.factors.append((H.sha(x), self.problem.ngrad))
        return super().factor(x, dinv, cdiag)

    def apply(self, bx, bw, yx, yw):
        self.napply += 1
        return super().apply(bx, bw, yx, yw)


def test_trust_region_subproblem_reaches_the_users_solver_at_xk(ctx):
    import paropt_amd as pa

    p = H.csr_groups(ctx)
    solver = Recording(p)
    p.setQuasiDefMat(solver)
    pa.TrustRegion(p, {"tr_max_iterations": 3, "qn_subspace_size": 4}).optimize()
    assert len(solver.factors) > 0 and solver.napply > 0
    # the subproblem's own variable is the step; every factor sees a point the problem was linearised at
    assert {point for point, _ in solver.factors} <= set(p.grad_points)


def test_mma_subproblem_reaches_the_users_solver_at_xvec(ctx):
    import paropt_amd as pa

    p = H.csr_groups(ctx)
    solver = Recording(p)
    p.setQuasiDefMat(solver)
    pa.MMA(p, {"mma_max_iterations": 3}).optimize()
    assert len(solver.factors) > 0 and solver.napply > 0
    # the interior point iterates on the subproblem; every factor sees the expansion point of the current subproblem
    assert all(point == p.grad_points[ngrad - 1] for point, ngrad in solver.factors)
