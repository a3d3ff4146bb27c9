"""Small problems, one per form of the quasi-definite solver of the sparse constraints (quasidef.hpp), with fixed
inputs for po_quasidef_factor / po_quasidef_apply: shared by tools/sparse_digest.py and tests/test_gpu_sparse_forms.py.

  grouped            SeparableProblem.setWeighting, n = 240, nw = 4: 60 groups without a gap, 48 with nwskip = 1
  csr_groups         the same constraints posed through the CSR interface (a recognised pattern)
  csr_fallback       ... with one entry made different from the fourth gradient evaluation on
  csr                SeparableProblem.setChain(2, 1), n = 241: overlapping rows, the sparse Cholesky
  scalar             callbacks with nwblock = 1, n = 40, 8 disjoint rows with unequal entries
  block2, block3     callbacks with packed blocks, n = 240, nwcon = 60
"""
import hashlib

import numpy as np

from oracle import paropt_oracle as po  # problem data only

N, NW = 240, 4
IP_OPTS = {"max_major_iters": 6, "qn_subspace_size": 4, "abs_res_tol": 1e-12, "write_output_frequency": 1}


def groups_of(skip):
    """60 groups fill n = 240 exactly; with a gap of one variable 48 fit"""
    return 60 if skip == 0 else N // (NW + skip)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def grouped(ctx, skip=0):
    import paropt_amd as pa

    return pa.SeparableProblem(ctx, "convex", N, 2).setWeighting(groups_of(skip), NW, 0, skip)


def csr_chain(ctx):
    import paropt_amd as pa

    return pa.SeparableProblem(ctx, "convex", 241, 2).setChain(2, 1)


def csr_groups(ctx, skip=0, differ_after=None):
    """The weighting constraints as a CSR pattern; differ_after = k: entry (0, 0) is -1.5 from gradient evaluation
    k + 1 on, which ends the grouped form in the middle of a run."""
    import paropt_amd as pa

    w, c = groups_of(skip), 2
    ref = po.SepProblem("convex", N, c, nwcon=w, nw=NW, nwskip=skip)
    rowp = np.arange(w + 1, dtype=np.intc) * NW
    cols = (np.arange(w)[:, None] * (NW + skip) + np.arange(NW)[None, :]).astype(np.intc).ravel()
    rows = np.repeat(np.arange(w), NW)

    class _P(pa.Problem):
        def __init__(self):
            self.A = ref.sparse_jacobian_dense()
            self.ngrad = 0
            self.grad_points = []
            super().__init__(ctx, N, c, c, nwcon=w, nwinequality=w, rowp=rowp, cols=cols)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = ref.vars_and_bounds()

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = 1.0 + self.A @ x
            return ref.eval_obj_con(x)

        def evalSparseObjConGradient(self, x, g, A, data):
            self.ngrad += 1
            self.grad_points.append(sha(x))
            if differ_after is not None and self.ngrad > differ_after:
                self.A[0, 0] = -1.5
            fail, gg, AA = ref.eval_obj_con_gradient(x)
            g[:] = gg
            for j in range(c):
                A[j][:] = AA[j]
            data[:] = self.A[rows, cols]
            return fail

    return _P()


def _callbacks(ctx, n, c, Aw, nwblock):
    import paropt_amd as pa

    w = Aw.shape[0]
    ref = po.SepProblem("convex", n, c)

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, c, c, nwcon=w, nwinequality=w, nwblock=nwblock)
            self.B = nwblock  # the block size addSparseInnerProduct fills (po_problem_set_sparse_block_size changes it)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = ref.vars_and_bounds()

        def evalObjCon(self, x):
            return ref.eval_obj_con(x)

        def evalObjConGradient(self, x, g, A):
            fail, gg, AA = ref.eval_obj_con_gradient(x)
            g[:] = gg
            for j in range(c):
                A[j][:] = AA[j]
            return fail

        def evalSparseCon(self, x, out):
            out[:] = 1.0 + Aw @ x

        def addSparseJacobian(self, alpha, x, px, out):
            out[:] = np.array(out) + alpha * (Aw @ px)

        def addSparseJacobianTranspose(self, alpha, x, pzw, out):
            out[:] = np.array(out) + alpha * (Aw.T @ pzw)

        def addSparseInnerProduct(self, alpha, x, cvec, A):
            S, B = (Aw * cvec) @ Aw.T, self.B
            incr = B * (B + 1) // 2  # packed upper triangles, column by column
            for b in range(w // B):
                for j in range(B):
                    for i in range(j + 1):
                        A[b * incr + i + j * (j + 1) // 2] += alpha * S[b * B + i, b * B + j]

    return _P()


def scalar(ctx):
    n, w, nw = 40, 8, 5
    Aw = np.zeros((w, n))
    for i in range(w):
        Aw[i, i * nw:(i + 1) * nw] = -(1.0 + 0.25 * np.arange(nw))
    return _callbacks(ctx, n, 2, Aw, 1)


def block_jacobian(B):
    return po.SepProblem("convex", N, 2, nwcon=60, nw=6, nwskip=2, nwblock=B).sparse_jacobian_dense()


def block(ctx, B):
    return _callbacks(ctx, N, 2, block_jacobian(B), B)


def set_block_size(problem, B):
    """po_problem_set_sparse_block_size on a problem of _callbacks; returns the C return code"""
    from paropt_amd import lib

    rc = lib.lib.po_problem_set_sparse_block_size(problem.handle, int(B))
    if rc == 0:
        problem.B = int(B)
    return rc


def factor_and_apply(ctx, problem, with_bw=True, launches=None):
    """po_quasidef_factor + po_quasidef_apply on fixed inputs: the bytes of (yx, yw); `launches` (a list) receives the
    kernel launches of the factor and of the apply, which tell the fused forms from the unfused ones"""
    import paropt_amd as pa

    n, w = problem.nvars, problem.nwcon
    rng = np.random.default_rng(11)
    arrays = [np.full(n, 0.5), rng.uniform(0.2, 3.0, n), rng.uniform(0.05, 2.0, w), rng.standard_normal(n),
              rng.standard_normal(w)]
    x, d, c, bx, bw = (pa.PVec(ctx, len(a)).from_numpy(a) for a in arrays)
    yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
    n0 = ctx.counters()[1]
    pa.quasidef_factor(problem, x, d, c)
    n1 = ctx.counters()[1]
    pa.quasidef_apply(problem, x, d, c, bx, bw if with_bw else None, yx, yw)
    if launches is not None:
        launches += [n1 - n0, ctx.counters()[1] - n1]
    return yx.to_numpy().tobytes(), yw.to_numpy().tobytes()


def upload_entries(problem):
    """one gradient evaluation: a CSR problem's Jacobian entries reach the device"""
    import paropt_amd as pa

    pa.InteriorPoint(problem, {"max_major_iters": 0}).optimize()
    return problem
