"""BASELINE.json's metric workload (config 3) as a Python user writes it with torch: the twin of
examples/random_convex_amd.cpp on paropt_amd.TorchProblem, whose callbacks receive zero-copy views of the library's
vectors and run on the context's stream.

    f(x)   = sum_i b_i^2 / (eps + x_i)
    c_j(x) = beta_j - a_j . x >= 0,  beta_j = 0.25 sum_i a_ji
    0 <= x <= 1,  x0 = 0.05 + 0.9 u

b (array id 2), a_j (100 + j) and u (3) are the library's counter-hash arrays (po_vec_fill_hash on the GLOBAL index),
the data of the built-in SeparableProblem("convex"), so the three forms of this problem can be compared iteration by
iteration.  Like the reference's example, evalObjConGradient rewrites every A[j] at every call.

device_results=False returns final host values (the reference's semantics): one host synchronisation of the problem's
own per evaluation, counted in `host_syncs` (the library cannot see it).  device_results=True returns this rank's f and
c as device tensors, which the library reduces over the ranks; with setDeferredReductions(True) it does so together
with its own reductions of the same step.

    python examples/random_convex_torch.py n=1000000 c=32 iters=30 [device] [deferred]
"""
import sys

import numpy as np
import torch

import paropt_amd as pa

EPS = 1e-3  # examples/random_convex_amd.cpp kEps


class RandomConvexTorch(pa.TorchProblem):
    def __init__(self, ctx, nglobal, ncon, seed=0, device_results=False):
        rank, size = ctx.rank_size()
        base, rem = divmod(int(nglobal), size)
        nlocal = base + (1 if rank < rem else 0)
        self.offset = rank * base + min(rank, rem)
        self.seed, self.rank, self.size = int(seed), rank, size
        self.device_results = bool(device_results)
        self.host_syncs = 0
        super().__init__(ctx, nlocal, ncon, ncon)
        dev = ctx.torch_stream().device
        bv = pa.PVec(ctx, nlocal).fill_hash(seed, 2, self.offset)
        av = [pa.PVec(ctx, nlocal).fill_hash(seed, 100 + j, self.offset) for j in range(ncon)]
        x0 = pa.PVec(ctx, nlocal).fill_hash(seed, 3, self.offset, 0.9, 0.05)
        beta = np.zeros(ncon)
        if ncon > 0:  # products with a vector of ones (collective), as the C++ twin forms them
            ones = pa.PVec(ctx, nlocal)
            ones.set(1.0)
            beta = 0.25 * ones.mdot(av)
        self.beta = beta
        with torch.cuda.stream(ctx.torch_stream()):
            b = bv.as_tensor()
            self.b2 = b * b
            self.x0 = x0.as_tensor()
            self.a = torch.stack([v.as_tensor() for v in av]) if ncon else torch.zeros(0, nlocal, dtype=torch.float64,
                                                                                        device=dev)
            # this rank's part of beta for the device results: summed over the ranks it is beta
            self.beta_local = torch.tensor(beta if rank == 0 else np.zeros(ncon), dtype=torch.float64, device=dev)

    def getVarsAndBounds(self, x, lb, ub):
        x.copy_(self.x0)
        lb.fill_(0.0)
        ub.fill_(1.0)
        return 0

    def evalObjCon(self, x):
        f = (self.b2 / (x + EPS)).sum()
        ax = torch.mv(self.a, x)
        if self.device_results:
            return 0, f, self.beta_local - ax
        vals = torch.cat([f.reshape(1), ax]).cpu().numpy()
        self.host_syncs += 1
        if self.size > 1:
            self.ctx.allreduce(vals)
        return 0, float(vals[0]), self.beta - vals[1:]

    def evalObjConGradient(self, x, g, A):
        d = x + EPS
        torch.div(self.b2, d.mul_(d), out=g)
        g.neg_()
        if A is not None:
            for j in range(self.ncon):
                torch.neg(self.a[j], out=A[j])
        return 0


def main(argv):
    kw = dict(a.split("=", 1) for a in argv if "=" in a)
    n, c, iters = int(kw.get("n", 1000000)), int(kw.get("c", 32)), int(kw.get("iters", 30))
    ctx = pa.Context(0)
    prob = RandomConvexTorch(ctx, n, c, device_results="device" in argv or "deferred" in argv)
    if "deferred" in argv:
        prob.setDeferredReductions(True)
    ip = pa.InteriorPoint(prob, {"qn_type": kw.get("qn", "sr1"), "qn_subspace_size": 10, "abs_res_tol": 1e-8,
                                 "start_affine_multiplier_min": 0.01, "max_major_iters": iters,
                                 "write_output_frequency": 0})
    ip.optimize()
    print("iterations %d, evaluations %d, gradients %d, fobj %.15e" % (ip.getIterationCounters() +
                                                                         (ip.getObjective()[0],)))


if __name__ == "__main__":
    main(sys.argv[1:])
