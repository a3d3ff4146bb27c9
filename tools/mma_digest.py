"""
Digest of MMA.optimize() on a fixed list of small problems and of the stand-alone dual entries on drawn subproblems,
one JSON line per record.  Two libraries compute the same thing bit for bit, refuse the same calls with the same words
and issue the same launches and host syncs exactly when their outputs are byte-identical:

    PAROPT_AMD_LIB=<one libparopt_amd.so> python tools/mma_digest.py > a.jsonl
    PAROPT_AMD_LIB=<another>              python tools/mma_digest.py > b.jsonl
    cmp a.jsonl b.jsonl

Whole runs (mma_max_iterations = 6): the full iteration history, SHA-256 of the bytes of x, zl, zu, zw, L, U, and z,
getState() and every stats getter as they are.  They cover the three ways a subproblem is solved and, for the dual,
every path of its pass: n = 1, an odd tail, the last fused width (c = 8), the first panel width (c = 9) and the first
width past the register-hold capacity (c = 33); grouped sparse constraints at a fused and a panel width, plain and
conservative; linearised constraints at c = 2, 9 and 33, and a dense equality.

Entries: every stand-alone dual entry at n = 513 with m on both sides of every column capacity of the passes; SHA-256
of W, grad, H, x, zl, zu, zw and the sums, and the stats.  Refusals: a fixed list of faulty arguments, each given to
every entry, with the return code and the text of po_last_error ("not refused" where an entry does not take the
argument and runs).  Every record carries the deltas of Context.counters() and Context.sync_counters() across it.

--brief: per record its name, the counters that moved (flag_waits only where it is not syncs), a refusal's return code
and 16 hex digits of the SHA-256 of the full line -- what profiles/ keeps.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DUAL = {"mma_subproblem_solver": "dual"}
GCMMA = {"mma_subproblem_solver": "dual", "mma_globalization": "conservative"}
GROUPS = dict(DUAL, mma_dual_sparse_constraints="groups")
GCMMA_GROUPS = dict(GROUPS, mma_globalization="conservative", mma_gcmma_sparse_constraints="groups")
LINEAR = dict(DUAL, mma_use_constraint_linearization=1, mma_dual_linearized_constraints="newton")
WEIGHTING = (85, 5, 0, 1)  # setWeighting: 85 groups of 5 variables, period 6, inside n = 513
CONFIGS = [
    ("convex", 200, 2, {}, None),
    ("convex", 200, 2, {"mma_use_constraint_linearization": 1}, None),
    ("convex", 1, 1, DUAL, None),
    ("convex", 511, 3, DUAL, None),
    ("convex", 513, 8, DUAL, None),
    ("convex", 513, 9, DUAL, None),
    ("convex", 4097, 33, DUAL, None),
    ("quadratic", 200, 2, GCMMA, None),
    ("convex", 513, 9, GCMMA, None),
    ("convex", 4097, 33, GCMMA, None),
    ("convex", 513, 3, GROUPS, WEIGHTING),
    ("convex", 513, 9, GROUPS, WEIGHTING),
    ("convex", 513, 3, GCMMA_GROUPS, WEIGHTING),
    ("convex", 513, 9, GCMMA_GROUPS, WEIGHTING),
    ("convex", 513, 2, LINEAR, None),
    ("convex", 513, 9, LINEAR, None),
    ("convex", 513, 33, LINEAR, None),
    ("equality", 64, 2, LINEAR, None),
]
ENTRY_N = 513
ENTRY_M = (2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 95)  # both sides of every capacity step, and kMmaDualMax
M_FUSED, M_MAX = 8, 95
GAMMA = 2.0


def _plain(d):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _shas(**arrays):
    return {k: _sha(v.to_numpy() if hasattr(v, "to_numpy") else v) for k, v in arrays.items() if v is not None}


class Counted:
    """the deltas of the context's launch and sync counters across a with block, into rec['counters']"""

    def __init__(self, ctx, rec):
        self.ctx, self.rec = ctx, rec

    def _now(self):
        syncs, launches = self.ctx.counters()
        return dict(self.ctx.sync_counters(), syncs=syncs, launches=launches)

    def __enter__(self):
        self.start = self._now()

    def __exit__(self, *exc):
        now = self._now()
        self.rec["counters"] = {k: now[k] - self.start[k] for k in now}
        return False


def equality_problem(pa, ctx, n):
    """the dense-equality problem of tests/test_gpu_mma_dual_linear.py: minimise sum w (x - a)^2 + 0.1 x^4 subject to
    14 - sum x^2 >= 0 and sum x - 24 = 0, -1 <= x <= 2"""
    j = np.arange(n)
    w, a = 1.0 + 2.0 * ((7 * j) % 11) / 10.0, ((5 * j) % 13) / 12.0

    class Equality(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, -1.0, 2.0

        def evalObjCon(self, x):
            f = float(np.sum(w * (x - a) ** 2 + 0.1 * x**4))
            return 0, f, np.array([14.0 - np.sum(x * x), np.sum(x) - 24.0])

        def evalObjConGradient(self, x, g, A):
            g[:] = 2.0 * w * (x - a) + 0.4 * x**3
            A[0][:] = -2.0 * x
            A[1][:] = 1.0
            return 0

    return Equality(ctx, n, 2, ninequality=1)


def digest(pa, ctx, kind, n, c, options, weighting):
    if kind == "equality":
        prob = equality_problem(pa, ctx, n)
    else:
        prob = pa.SeparableProblem(ctx, kind, n, c, 0)
        if weighting:
            prob.setWeighting(*weighting)
    rec = dict(problem=kind, n=n, c=c, options=options, weighting=weighting)
    mma = pa.MMA(prob, dict(options, mma_max_iterations=6))
    with Counted(ctx, rec):
        mma.optimize()
    x, z, zw, zl, zu = mma.getOptimizedPoint()
    lo, up = mma.getAsymptotes()
    rec.update(history=mma.getHistory(), sha256=_shas(x=x, zl=zl, zu=zu, L=lo, U=up, zw=zw if weighting else None),
               z=z.tolist(), state=_plain(mma.getState()), dual_stats=_plain(mma.getDualStats()),
               globalization_stats=_plain(mma.getGlobalizationStats()),
               group_stats=_plain(mma.getDualGroupStats()), linear_stats=_plain(mma.getDualLinearStats()))
    return rec


# ---- the stand-alone entries on a drawn subproblem --------------------------------------------------------------------
def draw(n, m, seed):
    """L < alpha < x0 < beta < U, p, q >= 0 and A with about half the entries exactly 0, lambda mixing 0, interior values
    and gamma; groups of nw = 5 with period 6 (psi = c - sum x) whose c cycles through inactive, strict and at gamma"""
    rng = np.random.default_rng([seed, m])
    x0 = 5.0 + rng.random(n)
    lo = x0 - (2.0 + 2.0 * rng.random(n))
    up = x0 + (2.0 + 2.0 * rng.random(n))
    d = dict(L=lo, U=up, alpha=x0 - (0.2 + 0.4 * rng.random(n)) * (x0 - lo),
             beta=x0 + (0.2 + 0.4 * rng.random(n)) * (up - x0), p0=0.2 * 10.0 ** (-2.0 * rng.random(n)),
             q0=0.2 * 10.0 ** (-2.0 * rng.random(n)), xk=x0, g=rng.standard_normal(n))
    d["p"] = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    d["q"] = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    d["A"] = (0.08 / np.sqrt(m)) * rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.5)
    d["b"] = rng.standard_normal(m)
    d["cons"] = rng.standard_normal(m)
    lam = GAMMA * rng.random(m)
    lam[0::3] = 0.0
    lam[1::3] = GAMMA
    d["lam"] = lam
    d["rho"] = 1e-3 * (1.0 + rng.random(m + 1))
    nw, period = 5, 6
    nwcon = n // period
    idx = np.arange(nwcon)[:, None] * period + np.arange(nw)[None, :]
    sa, s0, sb = d["alpha"][idx].sum(axis=1), x0[idx].sum(axis=1), d["beta"][idx].sum(axis=1)
    d["c"] = np.where(np.arange(nwcon) % 3 == 0, sb + 0.1 * nw, np.where(np.arange(nwcon) % 3 == 1, s0, sa - 0.1 * nw))
    d["groups"] = (nwcon, nw, 0, 1, -1.0, (2 * nwcon) // 3)  # nwcon, nw, start, skip, a, nwinequality
    return d


class Dev:
    """the draw on the device"""

    def __init__(self, pa, ctx, d):
        n = d["L"].size
        up = lambda a: pa.PVec(ctx, a.size).from_numpy(a)  # noqa: E731
        self.pa, self.ctx, self.n, self.d = pa, ctx, n, d
        for k in ("L", "U", "alpha", "beta", "p0", "q0", "xk", "g", "c"):
            setattr(self, k, up(d[k]))
        self.p, self.q, self.A = ([up(row) for row in d[k]] for k in ("p", "q", "A"))
        self.head = (ctx, self.L, self.U, self.alpha, self.beta, self.p0, self.q0)

    def point(self):
        return [self.pa.PVec(self.ctx, self.n) for _ in range(3)]

    def zw(self, nwcon):
        return self.pa.PVec(self.ctx, nwcon) if nwcon > 0 else None


def entry_records(pa, ctx, m):
    """(name, callable -> dict of arrays and stats) for every entry at this m"""
    d = draw(ENTRY_N, m, 7)
    dev = Dev(pa, ctx, d)
    lam, rho, b = d["lam"], d["rho"], d["b"]
    out = []

    def dual(form, with_rho, with_point):
        def run():
            pt = dev.point() if with_point else None
            r = pa.mma_dual_eval(*dev.head, dev.p, dev.q, b, lam, form=form, point=pt,
                                 **(dict(xk=dev.xk, rho=rho) if with_rho else {}))
            arrays = dict(W=[r[0]], grad=r[1], H=r[2], D=[r[3]] if with_rho else None)
            if pt:
                arrays.update(x=pt[0], zl=pt[1], zu=pt[2])
            return arrays, None
        return "mma_dual_eval form %d%s%s" % (form, " rho" if with_rho else "", " point" if with_point else ""), run

    for form in (0, 1, 2):
        if form == 1 and m > M_FUSED:
            continue
        out += [dual(form, False, False), dual(form, False, True), dual(form, True, False)]

    def gcmma_point():
        pt = dev.point()
        sums = pa.mma_gcmma_point(*dev.head, dev.p, dev.q, lam, dev.xk, rho, pt)
        return dict(sums=sums, x=pt[0], zl=pt[1], zu=pt[2]), None

    def rho_sums():
        return dict(sums=pa.mma_gcmma_rho_sums(ctx, dev.L, dev.U, dev.g, dev.A)), None

    out += [("mma_gcmma_point", gcmma_point), ("mma_gcmma_rho_sums", rho_sums)]

    def group(grouped, with_rho, point_only):
        nwcon, nw, start, skip, a, nwineq = d["groups"] if grouped else (0, 1, 0, 0, -1.0, 0)

        def run():
            pt, zw = dev.point(), dev.zw(nwcon)
            c = dev.c if grouped else None
            if point_only:
                sums, st = pa.mma_gcmma_group_point(*dev.head, dev.p, dev.q, lam, nwcon, nw, start, skip, a, c, nwineq,
                                                    GAMMA, dev.xk, rho, pt, zw)
                arrays = dict(sums=sums)
            else:
                r = pa.mma_dual_group_eval(*dev.head, dev.p, dev.q, b, lam, nwcon, nw, start, skip, a, c, nwineq, GAMMA,
                                           pt, zw, **(dict(xk=dev.xk, rho=rho) if with_rho else {}))
                arrays, st = dict(W=[r[0]], grad=r[1], H=r[2], D=[r[4]] if with_rho else None), r[3]
            arrays.update(x=pt[0], zl=pt[1], zu=pt[2], zw=zw)
            return arrays, st
        name = "mma_gcmma_group_point" if point_only else "mma_dual_group_eval" + (" rho" if with_rho else "")
        return name + (" nwcon %d" % nwcon), run

    for grouped in (False, True):
        out += [group(grouped, False, False), group(grouped, True, False), group(grouped, False, True)]

    def linear(form, with_point):
        def run():
            xs = pa.PVec(ctx, ENTRY_N).from_numpy(d["xk"])
            pt = dev.point() if with_point else None
            W, g, H, st = pa.mma_dual_linear_eval(*dev.head, dev.A, d["cons"], dev.xk, lam, xs, form=form, point=pt)
            arrays = dict(W=[W], grad=g, H=H, xstart=xs)
            if pt:
                arrays.update(x=pt[0], zl=pt[1], zu=pt[2])
            return arrays, st
        return "mma_dual_linear_eval form %d%s" % (form, " point" if with_point else ""), run

    for form in (0, 1, 2):
        if form == 1 and m > M_FUSED:
            continue
        out += [linear(form, False), linear(form, True)]
    return out


def entries(pa, ctx):
    for m in ENTRY_M:
        for name, run in entry_records(pa, ctx, m):
            rec = dict(entry=name, n=ENTRY_N, m=m)
            with Counted(ctx, rec):
                arrays, stats = run()
            rec.update(sha256=_shas(**arrays), stats=stats)
            yield rec


# ---- calls that must be refused ---------------------------------------------------------------------------------------
class Null:
    handle = None


def refusals(pa, ctx):
    """(name, callable) in a fixed order; every callable must raise ParOptAMDError (or be refused by an MMA run)"""
    n = 64
    other = pa.Context(0)
    out = []

    def family(m, **swap):
        """the seven entries on a draw of m constraints with some arguments replaced"""
        d = draw(n, min(m, M_MAX), 3)
        dev = Dev(pa, ctx, d)
        if m > M_MAX:  # (the columns of one too many constraints: the last one repeated)
            dev.p, dev.q, dev.A = (v + [v[-1]] * (m - M_MAX) for v in (dev.p, dev.q, dev.A))
            for k in ("b", "lam", "cons"):
                d[k] = np.concatenate([d[k], np.zeros(m - M_MAX)])
            d["rho"] = np.concatenate([d["rho"], np.zeros(m - M_MAX)])
        form = swap.pop("form", 0)
        gamma = swap.pop("gamma", GAMMA)
        groups = swap.pop("groups", (n // 6, 5, 0, 1, -1.0, 4))
        point = swap.pop("point", None)
        cvec = swap.pop("c", None)
        for k, v in swap.items():
            if k in ("p0", "U", "xk"):
                setattr(dev, k, v(dev))
            else:  # p, q, A: column 1 replaced
                getattr(dev, k)[1] = v(dev)
        dev.head = (ctx, dev.L, dev.U, dev.alpha, dev.beta, dev.p0, dev.q0)
        lam, rho, b = d["lam"], d["rho"], d["b"]
        nwcon, nw, start, skip, a, nwineq = groups
        c = cvec(dev) if cvec else pa.PVec(ctx, max(nwcon, 1)).from_numpy(np.full(max(nwcon, 1), 27.0))
        pt = lambda: point(dev) if point else dev.point()  # noqa: E731
        return [
            ("mma_dual_eval", lambda: pa.mma_dual_eval(*dev.head, dev.p, dev.q, b, lam, form=form,
                                                       point=point(dev) if point else None)),
            ("mma_dual_eval rho", lambda: pa.mma_dual_eval(*dev.head, dev.p, dev.q, b, lam, form=form, xk=dev.xk,
                                                           rho=rho)),
            ("mma_gcmma_point", lambda: pa.mma_gcmma_point(*dev.head, dev.p, dev.q, lam, dev.xk, rho, pt())),
            ("mma_gcmma_rho_sums", lambda: pa.mma_gcmma_rho_sums(ctx, dev.L, dev.U, dev.g, dev.A)),
            ("mma_dual_group_eval", lambda: pa.mma_dual_group_eval(*dev.head, dev.p, dev.q, b, lam, nwcon, nw, start,
                                                                   skip, a, c, nwineq, gamma, pt(), dev.zw(nwcon))),
            ("mma_dual_group_eval rho", lambda: pa.mma_dual_group_eval(*dev.head, dev.p, dev.q, b, lam, nwcon, nw,
                                                                       start, skip, a, c, nwineq, gamma, pt(),
                                                                       dev.zw(nwcon), xk=dev.xk, rho=rho)),
            ("mma_gcmma_group_point", lambda: pa.mma_gcmma_group_point(*dev.head, dev.p, dev.q, lam, nwcon, nw, start,
                                                                       skip, a, c, nwineq, gamma, dev.xk, rho, pt(),
                                                                       dev.zw(nwcon))),
            ("mma_dual_linear_eval", lambda: pa.mma_dual_linear_eval(
                *dev.head, dev.A, d["cons"], dev.xk, lam, pa.PVec(ctx, n).from_numpy(d["xk"]), form=form,
                point=point(dev) if point else None)),
        ]

    def add(what, calls, only=None):
        for name, run in calls:
            if only is None or any(name.startswith(o) for o in only):
                out.append(("%s: %s" % (what, name), run))

    longer = lambda dev: pa.PVec(ctx, n + 2)  # noqa: E731
    foreign = lambda dev: pa.PVec(other, n)  # noqa: E731
    formed = ("mma_dual_eval", "mma_dual_linear_eval")
    add("m past kMmaDualMax", family(M_MAX + 1))
    add("form 3", family(3, form=3), formed)
    add("form -1", family(3, form=-1), formed)
    add("form 1 past its width", family(M_FUSED + 1, form=1), formed)
    add("bad m and bad form", family(M_MAX + 1, form=7), formed)
    add("a null column", family(3, p=lambda dev: Null, A=lambda dev: Null))
    add("a null q column", family(3, q=lambda dev: Null))
    add("a null p0", family(3, p0=lambda dev: Null))
    add("a column of another length", family(3, p=longer, A=longer))
    add("a q column of another length", family(3, q=longer))
    add("U of another length", family(3, U=longer))
    add("xk of another length", family(3, xk=longer))
    add("a column on another context", family(3, q=foreign, A=foreign))
    add("p0 on another context", family(3, p0=foreign))
    add("x without zl", family(3, point=lambda dev: [dev.pa.PVec(ctx, n), Null, Null]),
        ("mma_dual_eval", "mma_gcmma_point", "mma_dual_group", "mma_gcmma_group", "mma_dual_linear_eval"))
    add("zu of another length", family(3, point=lambda dev: [dev.pa.PVec(ctx, n), dev.pa.PVec(ctx, n), longer(dev)]),
        ("mma_dual_eval", "mma_gcmma_point", "mma_dual_group", "mma_gcmma_group", "mma_dual_linear_eval"))
    grouped = ("mma_dual_group", "mma_gcmma_group")
    add("groups past the variables", family(3, groups=(n // 6 + 1, 5, 0, 1, -1.0, 4)), grouped)
    add("a period beyond a tile", family(3, groups=(1, 600, 0, 0, -1.0, 1)), grouped)
    add("nw = 0", family(3, groups=(4, 0, 0, 1, -1.0, 4)), grouped)
    add("negative nwcon", family(3, groups=(-1, 5, 0, 1, -1.0, 0)), grouped)
    add("gamma = 0", family(3, gamma=0.0), grouped)
    add("gamma < 0 without groups", family(3, gamma=-1.0, groups=(0, 1, 0, 0, -1.0, 0)), grouped)
    add("c of the wrong length", family(3, c=lambda dev: pa.PVec(ctx, n // 6 + 1)), grouped)
    add("c missing", family(3, c=lambda dev: Null), grouped)

    def run_mma(make, options):
        return lambda: pa.MMA(make(), dict(options, mma_max_iterations=2)).optimize()

    weighting = lambda: pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)  # noqa: E731
    plain = lambda: pa.SeparableProblem(ctx, "convex", 240, 3)  # noqa: E731
    out += [
        ("MMA: sparse constraints without groups", run_mma(weighting, DUAL)),
        ("MMA: conservative groups without their option", run_mma(weighting, dict(GROUPS,
                                                                                mma_globalization="conservative"))),
        ("MMA: a period beyond a tile",
         run_mma(lambda: pa.SeparableProblem(ctx, "convex", 1200, 2).setWeighting(2, 600, 0, 0), GROUPS)),
        ("MMA: linearised with groups", run_mma(weighting, dict(LINEAR, mma_dual_sparse_constraints="groups"))),
        ("MMA: linearised and conservative", run_mma(plain, dict(LINEAR, mma_globalization="conservative"))),
        ("MMA: a dense equality in the rational dual", run_mma(lambda: equality_problem(pa, ctx, 64), DUAL)),
        ("MMA: linearised without newton", run_mma(plain, dict(DUAL, mma_use_constraint_linearization=1))),
        ("MMA: conservative without the dual", run_mma(plain, {"mma_globalization": "conservative"})),
    ]
    for name, run in out:
        rec = dict(refusal=name)
        with Counted(ctx, rec):
            try:
                run()
                rec.update(code=0, text="not refused")
            except pa.ParOptAMDError as e:
                rec.update(code=e.code, text=str(e))
        yield rec
    other.close()


def brief(rec):
    """the --brief form of a record"""
    line = json.dumps(rec, sort_keys=True)
    if "history" in rec:
        opts = ",".join("%s=%s" % (k.replace("mma_", ""), v) for k, v in sorted(rec["options"].items()))
        name = "run %s n=%d c=%d %s%s" % (rec["problem"], rec["n"], rec["c"], opts or "interior_point",
                                         " weighting" if rec["weighting"] else "")
    else:
        name = "%s m=%d" % (rec["entry"], rec["m"]) if "entry" in rec else "refusal " + rec["refusal"]
    moved = {k: v for k, v in rec["counters"].items() if v}
    if moved.get("flag_waits") == moved.get("syncs"):  # (every host sync a polled completion: the usual case)
        moved.pop("flag_waits", None)
    out = dict(id=name, sha=hashlib.sha256(line.encode()).hexdigest()[:16], **moved)
    if "code" in rec:
        out["code"] = rec["code"]
    return out


def main():
    import paropt_amd as pa

    show = brief if "--brief" in sys.argv[1:] else (lambda rec: rec)
    ctx = pa.Context(0)
    for kind, n, c, options, weighting in CONFIGS:
        print(json.dumps(show(digest(pa, ctx, kind, n, c, options, weighting)), sort_keys=True), flush=True)
    for rec in entries(pa, ctx):
        print(json.dumps(show(rec), sort_keys=True), flush=True)
    for rec in refusals(pa, ctx):
        print(json.dumps(show(rec), sort_keys=True), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
