"""Helpers shared by the MMA GPU tests (tests/test_gpu_mma_*.py): plain functions, no fixtures."""
import math
import socket

import numpy as np


def accurate_sum(terms):
    """Sums with an error far below the double-precision bound of the checks: x87 extended precision (64-bit
    mantissa, pairwise) where numpy has it, math.fsum otherwise."""
    if np.finfo(np.longdouble).eps < 1e-18:
        return np.sum(terms, axis=-1, dtype=np.longdouble).astype(np.float64)
    t = np.atleast_2d(terms)
    out = np.array([math.fsum(row) for row in t])
    return out if np.ndim(terms) > 1 else out[0]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_two_ranks(worker):
    """worker(rank, 2, port, queue) in two spawned processes that share the GPU: what rank 0 put into the queue, once
    both processes have ended with exit code 0."""
    import torch.multiprocessing as mp

    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    port = free_port()
    procs = [mpctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    result = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return result
