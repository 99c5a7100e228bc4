"""GPU (-m gpu): PBiCG, PBiCGStab and smoothSolver through every single-rank pipeline, at the edges of their solver controls.

mi_pbicg_solve takes one of three loops (engine.hip, multi.inc): the multi-vector solver with one right-hand side (M, the default),
pbicg_solve_device (D: MI_PBICG_MULTI=0, compact rows, cyclicAMI patches) and the host-stepped loop (H: MI_PBICG_HOST_STEPPED=1).
M, D and PBiCGStab's device loop are iteration bodies inside one host frame (engine.hip: stage_in, drive_batches, finish_device);
M's first batch is 1 iteration, the others' 2.  PBiCGStab has its device loop (pbicgstab_solve_device) and a host-stepped twin; smoothSolver swaps two buffers after every Jacobi sweep.  Every run is held
against the oracle (PBiCG.C, PBiCGStab.C, smoothSolver.C): iteration count and flags equal, the history through _check_hist,
normFactor to 1e-13, psi to 1e-9 of max|psi_ref| -- smoothSolver's psi bit for bit.  The counters of mi_ctx_stat say which loop ran.

Families whose members run the same arithmetic in the same order, compared BIT FOR BIT run by run:
  PBiCG, fused dots: M (any batch, MI_MULTI_PIPE 0 / 1, fuse_prologue 0 / 1) and D with the paired A / A^T pass (MI_PBICG_PAIR=1).
      D's tile_pair is tile_multi with one component -- the kernel M runs -- and both fold its per-tile dot partials with the same
      loop (k_fold_partials / k_fold_partials3); the update kernels are the same k_bicg_* launches; the two prologues are the fused
      one-pass forms test_prologue_fused.py holds to the separate passes.
  PBiCG, separate dots: M with MI_MULTI_TILE=0, D with MI_PBICG_PAIR=0 and H.  Without the multi-vector pass both dots of an
      iteration are k_reduce sums over the vectors, grouped unlike the per-tile partials (hence a family of their own); H's
      precondition + reduce_sync, k_xpsy (one fma) and host divisions are the device kernels' fma chains and divisions one by one.
  PBiCGStab: the device loop with any batch and the host-stepped loop.  k_stab_s, k_reduce_two and k_stab_update are H's k_xpsy
      and reduce_sync passes fused with the same per-thread fma / fabs order (psi += alpha yA, then += omega q, in one fma chain).
Batching is invisible: convergence and maxIter land inside a batch and on either side of a batch boundary (tolerance 0 with
maxIter derived from each loop's growing schedule)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import random_graph_case
from test_gpu_parity import HIST_RTOL, _check_hist

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_ref import SMOOTH_CONTROLS, SOLVER_CONTROLS  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("nIterations", "converged", "singular", "initialResidual", "finalResidual", "normFactor")
DIMS = [(1, 1, 1), (2, 1, 1), (70, 1, 1), (21, 17, 13), (40, 32, 24), "graph"]
PRECONDS = ["none", "diagonal", "DILU"]
# mi_ctx_stat: PBiCG through the multi-vector solver / pbicg_solve_device / host-stepped; PBiCGStab device / host-stepped / mid exit
S_MULTI, S_DEV, S_HOST, S_STAB_DEV, S_STAB_HOST, S_STAB_MID = 6, 7, 8, 9, 10, 11
STATS = (S_MULTI, S_DEV, S_HOST, S_STAB_DEV, S_STAB_HOST, S_STAB_MID)
BASE_ENV = dict(MI_PCG_BATCH="16", MI_MULTI_PIPE="1", MI_MULTI_TILE="1", MI_PBICG_MULTI="1", MI_PBICG_PAIR="1",
                MI_PBICG_HOST_STEPPED="0", MI_FUSE_PROLOGUE="1", MI_ENTRY16="0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _case(pkg, dims):
    return random_graph_case(pkg, 3000, symmetric=False) if dims == "graph" else pkg.synthetic.box_case(*dims, symmetric=False)


def _ctx(pkg, monkeypatch, env=(), **opts):
    """a context created under these switches.  csrc/switches.hpp says when each is read: most at mi_ctx_create, MI_ENTRY16 when the
    addressing is created, MI_MULTI_TILE and MI_PBICG_MULTI on every call -- so they stay set while the caller solves on this
    context (the next _ctx sets every switch again)"""
    for k, v in {**BASE_ENV, **dict(env)}.items():
        monkeypatch.setenv(k, v)
    ctx = pkg.engine.Context(0, torch.cuda.current_stream().cuda_stream)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _make(pkg, ctx, case):
    eng = pkg.engine
    if case.interfaces:
        fcs = [i.face_cells for i in case.interfaces]
        nbrs = [case.interfaces[i.nbr_patch].face_cells for i in case.interfaces]
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, fcs, nbrs)
    else:
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
    mat = eng.Matrix(addr)
    mat.set_coeffs(dev(case.diag), dev(case.upper), None if case.lower is None else dev(case.lower))
    for p, itf in enumerate(case.interfaces or ()):
        mat.set_interface_coeffs(p, dev(itf.bou_coeffs), None if case.lower is None else dev(itf.int_coeffs))
    return addr, mat


def _stats(ctx):
    return np.array([ctx.stat(k) for k in STATS])


def _starts(first, batch, upto=40):
    """first iteration of every batch of a loop whose batches grow first, 2 first, ... up to `batch`"""
    s, nb = [0], first
    while s[-1] < upto:
        s.append(s[-1] + nb)
        nb = min(2 * nb, batch)
    return s


def _edges(first, batch):
    """tolerance 0 runs iterations 0 .. maxIter: the last one ends a batch (maxIter = start - 1) or opens one (maxIter = start),
    at the first batch boundary from iteration 12 on"""
    b = next(s for s in _starts(first, batch) if s >= 12)
    return {b - 1, b}


def _controls(edges):
    """the reference's golden controls, maxIter 0 and 1, minIter > maxIter, and the batch-boundary maxIters"""
    out = [dict(kw) for kw in SOLVER_CONTROLS]
    out += [dict(tolerance=0.0, maxIter=0), dict(tolerance=0.0, maxIter=1), dict(tolerance=1e30, maxIter=2, minIter=5),
            dict(tolerance=1e-12, relTol=0.0, maxIter=3, minIter=6)]
    out += [dict(tolerance=0.0, maxIter=m) for m in sorted(edges)]
    return out


def _runs(case, orc_psi):
    """(name, psi0, source, controls): zero start, a non-zero start, a start the reference's loop finds converged (with and without
    minIter), a zero source with tolerance 0 (PBiCG: the wApT singular exit, PBiCGStab: the rA0rA one)"""
    n = case.n_cells
    guess = 0.5 - np.cos(np.arange(n) * 0.7)
    return [("zero", np.zeros(n), case.source, None),
            ("guess", guess, case.source, [dict(tolerance=1e-9, maxIter=500), dict(tolerance=0.0, maxIter=5),
                                           dict(tolerance=1e-30, relTol=1e-3, maxIter=500)]),
            ("converged", orc_psi, case.source, [dict(tolerance=1e-6, maxIter=50), dict(tolerance=1e-6, maxIter=50, minIter=2)]),
            ("zero source", np.zeros(n), np.zeros(n), [dict(tolerance=0.0, maxIter=5)])]


def _same_bits(a, b, what):
    (pa, xa), (pb, xb) = a, b
    for k in FIELDS:
        assert pa[k] == pb[k] or (np.isnan(pa[k]) and np.isnan(pb[k])), (what, k, pa[k], pb[k])
    assert np.array_equal(pa["history"], pb["history"], equal_nan=True), (what, "history")
    assert np.array_equal(xa, xb, equal_nan=True), (what, "psi", float(np.max(np.abs(xa - xb))))


ROUNDING = 1e-8   # (of the initial residual) below it a history entry is decided by rounding (test_pcg_paths.py)


def _vs_oracle(perf, psi, ref, ref_psi, what, rounding_decides=False, psi_rel=1e-9, psi_scale=None):
    """the bar of every run: counts and flags equal, normFactor to 1e-13, psi to 1e-9, the whole history within HIST_RTOL of the
    initial residual, and _check_hist (default rel) on the history up to the first entry the oracle puts below ROUNDING x the
    initial residual.  From there on the entries only have to stay within ROUNDING of the oracle's (test_pcg_paths.py's bar):
    a one- or two-cell system is solved exactly in its first iterations and goes on at 1e-17 .. 1e-125, and BiCGStab amplifies
    the different grouping of the sums to 1e-4 relative once its residual is below 1e-9 (measured).  rounding_decides: the
    unpreconditioned 70-cell line, whose solve ends by finite termination -- no per-entry relative bar (as in test_pcg_paths.py);
    psi_rel: the bar on psi, relative to psi_scale (default max|psi_ref|)."""
    assert (perf["nIterations"], perf["converged"], perf["singular"]) == (ref["nIterations"], ref["converged"], ref["singular"]), \
        (what, perf["nIterations"], ref["nIterations"], perf["converged"], ref["converged"], perf["singular"], ref["singular"])
    h, hr = perf["history"], ref["history"]
    assert h.shape == hr.shape, (what, h, hr)
    if hr[0] == 0.0:      # zero source: nothing to be relative to -- the history, normFactor and psi must be exactly the oracle's
        assert np.array_equal(h, hr) and perf["normFactor"] == ref["normFactor"] and np.array_equal(psi, ref_psi), what
        return
    assert np.max(np.abs(h - hr)) < HIST_RTOL * hr[0], (what, h, hr)
    k = int(np.argmax(hr < ROUNDING * hr[0])) if np.any(hr < ROUNDING * hr[0]) else hr.size
    assert np.all(np.abs(h[k:] - hr[k:]) < ROUNDING * hr[0]), (what, h, hr)
    try:
        _check_hist(dict(perf, history=h[:k]), dict(ref, history=hr[:k]), **(dict(rel=1.0) if rounding_decides else {}))
    except AssertionError as e:
        raise AssertionError((what, h, hr)) from e
    scale = np.max(np.abs(ref_psi)) if psi_scale is None else psi_scale
    assert np.max(np.abs(psi - ref_psi)) <= psi_rel * max(scale, 1e-300), (what, float(np.max(np.abs(psi - ref_psi))))


def _oracle_defined(case, ref_psi, ref, kw):
    """PBiCGStab on one or two cells with tolerance 0 solves the system exactly: sA == 0, so omega = tAsA / tAtA = 0 / 0 and the
    reference's own psi and residuals are NaN from there on -- nothing to compare.  Nothing else may be left out."""
    if np.all(np.isfinite(ref_psi)) and np.isfinite(ref["finalResidual"]):
        return True
    assert case.n_cells <= 2 and kw["tolerance"] == 0.0, ("the oracle is not finite", kw)
    return False


class Oracle:
    def __init__(self, orc, case):
        self.S, self.cache = orc.System([case]), {}

    def __call__(self, solver, psi0, source, precond, kw, **extra):
        key = (solver, psi0.tobytes(), source.tobytes(), precond, tuple(sorted(kw.items())), tuple(sorted(extra.items())))
        if key not in self.cache:
            if solver == "smooth":
                self.cache[key] = self.S.smooth_solve(psi0, source, **kw, **extra)
            else:
                self.cache[key] = getattr(self.S, solver)(psi0, source, "AINV" if precond == "DILU" else precond, **kw, **extra)
        return self.cache[key]


def _plan(case, oracle, solver, precond, edges, **extra):
    """(what, psi0, source, control) of every run, the converged start from a tight oracle solve"""
    tight = oracle(solver, np.zeros(case.n_cells), case.source, precond, dict(tolerance=1e-13, maxIter=1000), **extra)[0]
    out = []
    for name, psi0, src, ctls in _runs(case, tight):
        for kw in (ctls if ctls is not None else _controls(edges)):
            out.append(((name, tuple(sorted(kw.items()))), psi0, src, kw))
    return out


def _execute(mat, solver, precond, plan, **extra):
    res = {}
    for what, psi0, src, kw in plan:
        psi = dev(psi0)
        if solver == "pbicg":
            perf = mat.pbicg(psi, dev(src), precond, **kw)
        else:
            perf = mat.pbicgstab(psi, dev(src), precond, **kw, **extra)
        res[what] = (perf, host(psi))
    return res


# ---- PBiCG ----------------------------------------------------------------------------------------------------------------------
def _pbicg_pipelines():
    """name -> (environment, options, family, counter that must move, batch schedule: (first batch, cap) or None)"""
    p = {"M": ({}, {}, "fused", S_MULTI, (1, 16)),
         "M pipe=0": (dict(MI_MULTI_PIPE="0"), {}, "fused", S_MULTI, (1, 16)),
         "M fuse_prologue=0": ({}, dict(fuse_prologue=0), "fused", S_MULTI, (1, 16)),
         "M tile=0": (dict(MI_MULTI_TILE="0"), {}, "separate", S_MULTI, (1, 16)),
         "D pair=1": (dict(MI_PBICG_MULTI="0"), {}, "fused", S_DEV, (2, 16)),
         "D pair=0": (dict(MI_PBICG_MULTI="0", MI_PBICG_PAIR="0"), {}, "separate", S_DEV, (2, 16)),
         "D pair=0 batch=3": (dict(MI_PBICG_MULTI="0", MI_PBICG_PAIR="0", MI_PCG_BATCH="3"), {}, "separate", S_DEV, (2, 3)),
         "H": (dict(MI_PBICG_HOST_STEPPED="1"), {}, "separate", S_HOST, None)}
    for b in (1, 2, 3):
        p[f"M batch={b}"] = (dict(MI_PCG_BATCH=str(b)), {}, "fused", S_MULTI, (1, b))
        p[f"D pair=1 batch={b}"] = (dict(MI_PBICG_MULTI="0", MI_PCG_BATCH=str(b)), {}, "fused", S_DEV, (min(2, b), b))
    return p


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("dims", DIMS)
def test_pbicg_pipelines(pkg, orc, dims, precond, monkeypatch):
    case = _case(pkg, dims)
    oracle = Oracle(orc, case)
    pipes = _pbicg_pipelines()
    edges = set().union(*(_edges(*sched) for *_, sched in pipes.values() if sched))
    plan = _plan(case, oracle, "pbicg", precond, edges)
    out, family = {}, {}
    for name, (env, opts, fam, counter, _) in pipes.items():
        ctx = _ctx(pkg, monkeypatch, env, **opts)
        addr, mat = _make(pkg, ctx, case)
        s0 = _stats(ctx)
        out[name] = _execute(mat, "pbicg", precond, plan)
        grew = dict(zip(STATS, _stats(ctx) - s0))
        assert grew[counter] == len(plan) and sum(grew.values()) == len(plan), (name, grew)   # that loop and no other, every solve
        family[name] = fam
        del mat, addr, ctx
    for fam, first in (("fused", "M"), ("separate", "D pair=0")):
        for name in (k for k, f in family.items() if f == fam):
            for what in out[first]:
                _same_bits(out[first][what], out[name][what], (name, first, what))
    for what, psi0, src, kw in plan:
        ref_psi, ref = oracle("pbicg", psi0, src, precond, kw)
        for name in ("M", "D pair=0"):       # one member of each family; the others equal it bit for bit
            _vs_oracle(*out[name][what], ref, ref_psi, (name, what), rounding_decides=dims == (70, 1, 1) and precond == "none")
    zs = [out["M"][w][0] for w, *_ in plan if w[0] == "zero source"]
    assert zs and all(p["singular"] == 1 and p["nIterations"] == 0 for p in zs)      # the wApT exit was taken


def test_pbicg_compact_rows_and_cyclic_interfaces(pkg, orc, monkeypatch):
    """an asymmetric cyclic box: the default route stays on the multi-vector solver (cyclic patches are local, no cyclicAMI);
    with compact rows (MI_ENTRY16=1) mi_pbicg_solve hands it to pbicg_solve_device, whose paired pass falls back to the
    single-vector passes of the compact form -- the same bits as the separate passes on the explicit rows (D pair=0)"""
    syn = pkg.synthetic
    case = syn.add_cyclic_y(syn.box_case(18, 12, 10, symmetric=False), asym_shift=0.25)
    oracle = Oracle(orc, case)
    for precond in PRECONDS:
        plan = _plan(case, oracle, "pbicg", precond, _edges(2, 16) | _edges(1, 16))
        out = {}
        for name, env, counter in (("M", {}, S_MULTI), ("compact", dict(MI_ENTRY16="1"), S_DEV),
                                   ("D pair=0", dict(MI_PBICG_MULTI="0", MI_PBICG_PAIR="0"), S_DEV)):
            ctx = _ctx(pkg, monkeypatch, env)
            addr, mat = _make(pkg, ctx, case)
            if name == "compact":
                monkeypatch.setenv("MI_ENTRY16", "0")
                explicit = _make(pkg, ctx, case)[0]
                assert addr.stats()["entries"] < 0.6 * explicit.stats()["entries"]      # the 16-bit form is in use
                del explicit
            s0 = _stats(ctx)
            out[name] = _execute(mat, "pbicg", precond, plan)
            grew = dict(zip(STATS, _stats(ctx) - s0))
            assert grew[counter] == len(plan) and sum(grew.values()) == len(plan), (name, grew)
            del mat, addr, ctx
        for what, psi0, src, kw in plan:
            ref_psi, ref = oracle("pbicg", psi0, src, precond, kw)
            for name in out:
                _vs_oracle(*out[name][what], ref, ref_psi, (precond, name, what))
            _same_bits(out["D pair=0"][what], out["compact"][what], (precond, what))


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("dims", [(21, 17, 13), "graph"])
def test_pbicg_multi_components_end_differently(pkg, orc, dims, precond, monkeypatch):
    """mi_pbicg_solve_multi with 2 and 3 components whose loops end differently inside one solve: one converges (it starts from a
    partly solved psi), one stops at maxIter, one converges in the prologue (zero source) -- or, with tolerance 0, is singular at
    once while the others stop at maxIter.  Each component: the oracle's solve, and bit for bit the single-component solve (the
    same loop, M).  MI_PBICG_MULTI=0 runs the components one by one through pbicg_solve_device (the fused family: the same bits)."""
    case = _case(pkg, dims)
    n = case.n_cells
    oracle = Oracle(orc, case)
    z = np.zeros(n)
    full = oracle("pbicg", z, case.source, precond, dict(tolerance=1e-9, maxIter=500))[1]["nIterations"]
    A = (oracle("pbicg", z, case.source, precond, dict(tolerance=0.0, maxIter=full // 2))[0], case.source)
    B = (z, 3.0 * (pkg.synthetic.splitmix_uniform(41, n) - 0.5))
    Z = (z, z)
    its = [oracle("pbicg", *c, precond, dict(tolerance=1e-9, maxIter=500))[1]["nIterations"] for c in (A, B)]
    assert its[0] < its[1], its
    ctls = [dict(tolerance=1e-9, maxIter=(its[0] + its[1]) // 2), dict(tolerance=0.0, maxIter=6)]
    for env, counter in (({}, S_MULTI), (dict(MI_PBICG_MULTI="0"), S_DEV)):
        ctx = _ctx(pkg, monkeypatch, env)
        addr, mat = _make(pkg, ctx, case)
        for k, kw in enumerate(ctls):
            for comps in ((A, B, Z), (Z, B), (B, A)):
                psis = [dev(p0) for p0, _ in comps]
                s0 = _stats(ctx)
                got = mat.pbicg_multi(psis, [dev(b) for _, b in comps], precond, **kw)
                grew = dict(zip(STATS, _stats(ctx) - s0))
                assert grew[counter] == (1 if counter == S_MULTI else len(comps)) and sum(grew.values()) == grew[counter], (env, grew)
                ends = set()
                for c, (p0, b) in enumerate(comps):
                    what = (env, kw, len(comps), c)
                    ref_psi, ref = oracle("pbicg", p0, b, precond, kw)
                    _vs_oracle(got[c], host(psis[c]), ref, ref_psi, what)
                    ends.add((got[c]["converged"], got[c]["singular"], got[c]["nIterations"]))
                    psi = dev(p0)
                    single = mat.pbicg(psi, dev(b), precond, **kw)
                    _same_bits((got[c], host(psis[c])), (single, host(psi)), what)
                # every component ended its own way (with tolerance 0, A and B both stop at maxIter)
                assert len(ends) == (len(comps) if k == 0 else 1 + any(c is Z for c in comps)), (kw, ends)
        del mat, addr, ctx


# ---- PBiCGStab ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("dims", DIMS)
def test_pbicgstab_pipelines(pkg, orc, dims, precond, monkeypatch):
    case = _case(pkg, dims)
    oracle = Oracle(orc, case)
    pipes = {f"device batch={b}": (dict(MI_PCG_BATCH=str(b)), S_STAB_DEV, (min(2, b), b)) for b in (16, 1, 2, 3)}
    pipes["H"] = (dict(MI_PBICG_HOST_STEPPED="1"), S_STAB_HOST, None)
    edges = set().union(*(_edges(*sched) for _, _, sched in pipes.values() if sched))
    mids = {}
    for quirk in (True, False):
        plan = [r for r in _plan(case, oracle, "pbicgstab", precond, edges, replicate_quirk=quirk)
                if _oracle_defined(case, *oracle("pbicgstab", r[1], r[2], precond, r[3], replicate_quirk=quirk), r[3])]
        out = {}
        for name, (env, counter, _) in pipes.items():
            ctx = _ctx(pkg, monkeypatch, env)
            addr, mat = _make(pkg, ctx, case)
            res, mid = {}, {}
            for what, psi0, src, kw in plan:
                s0 = _stats(ctx)
                res.update(_execute(mat, "pbicgstab", precond, [(what, psi0, src, kw)], replicate_quirk=quirk))
                grew = dict(zip(STATS, _stats(ctx) - s0))
                assert grew[counter] == 1 and sum(grew.values()) == 1 + grew[S_STAB_MID], (name, what, grew)
                mid[what] = grew[S_STAB_MID]
            out[name], mids[quirk, name] = res, mid
            del mat, addr, ctx
        # one family: every pipeline the same bits, and the same exits (H counts the mid exit where it takes it, the device
        # loop reads it off the fetched state)
        for name in out:
            assert mids[quirk, name] == mids[quirk, "H"], name
            for what in out["H"]:
                _same_bits(out["H"][what], out[name][what], (quirk, name, what))
        for what, psi0, src, kw in plan:
            ref_psi, ref = oracle("pbicgstab", psi0, src, precond, kw, replicate_quirk=quirk)
            perf, psi = out["device batch=16"][what]
            # one or two cells, the 70-cell line: BiCGStab reaches finite termination, and a run that goes on below ROUNDING
            # divides rounding noise by rounding noise (omega, beta) -- per-entry history bars do not apply and psi moves by
            # up to 1.1e-7 of its size between two correct groupings of the sums, or of the start when the start is the larger
            # (the line from the non-zero guess: psi 3.7e-4, start 1.5, 5.3e-10 apart; measured); the family above still holds
            # these runs bit for bit
            rd = dims in ((1, 1, 1), (2, 1, 1), (70, 1, 1)) and np.min(ref["history"]) < ROUNDING * ref["history"][0]
            _vs_oracle(perf, psi, ref, ref_psi, (quirk, what), rounding_decides=rd, psi_rel=1e-6 if rd else 1e-9,
                       psi_scale=max(np.max(np.abs(ref_psi)), np.max(np.abs(psi0))) if rd else None)
            if mids[quirk, "H"][what]:      # the mid exit: converged on sA, counted as an iteration, sA's residual last
                assert perf["converged"] and perf["history"][-1] == perf["finalResidual"], what
        zs = [out["H"][w][0] for w, *_ in plan if w[0] == "zero source"]
        assert zs and all(p["singular"] == 1 and p["nIterations"] == 0 for p in zs)      # the rA0rA exit was taken
    if dims in ((1, 1, 1), (2, 1, 1)):
        # a one- or two-cell system is solved exactly in the first half step: the mid exit must have been taken
        assert all(sum(m.values()) > 0 for m in mids.values()), mids


# ---- smoothSolver ---------------------------------------------------------------------------------------------------------------
SWEEPS = (1, 2, 3, -3, -4)


@pytest.mark.parametrize("dims", DIMS)
def test_smooth_solver_sweeps_and_controls(pkg, orc, dims, monkeypatch):
    """n_sweeps odd and even (the result in either ping-pong buffer), negative (fixed sweeps, no residual: every perf field 0
    but nIterations, no history), two omegas, every control.  The Jacobi sweep is bit-exact (test_spmv_family_bit_exact), so
    psi equals the oracle's BIT FOR BIT"""
    case = _case(pkg, dims)
    n = case.n_cells
    oracle = Oracle(orc, case)
    ctx = _ctx(pkg, monkeypatch)
    addr, mat = _make(pkg, ctx, case)
    guess = 0.5 - np.cos(np.arange(n) * 0.7)
    conv = oracle("smooth", np.zeros(n), case.source, None, dict(n_sweeps=1, tolerance=1e-12, maxIter=20000))[0]
    ctls = [dict(kw) for kw in SMOOTH_CONTROLS]
    for sw in SWEEPS:
        for kw in (dict(tolerance=1e-4, maxIter=400), dict(tolerance=0.0, maxIter=10), dict(tolerance=0.0, maxIter=0),
                   dict(tolerance=1e30, maxIter=3, minIter=7), dict(tolerance=1e-30, relTol=0.05, maxIter=400)):
            ctls.append(dict(kw, n_sweeps=sw))
    runs = [("zero", np.zeros(n), case.source, ctls)]
    runs += [("guess", guess, case.source, [dict(n_sweeps=sw, tolerance=1e-5, maxIter=200) for sw in SWEEPS])]
    runs += [("converged", conv, case.source, [dict(n_sweeps=sw, tolerance=1e-6, maxIter=50, minIter=mi) for sw in (1, 2) for mi in (0, 1)])]
    runs += [("zero source", np.zeros(n), np.zeros(n), [dict(n_sweeps=3, tolerance=0.0, maxIter=5)])]
    for omega in (0.9, 0.6):
        for name, psi0, src, cl in runs:
            for kw in cl:
                what = (omega, name, kw)
                psi = dev(psi0)
                perf = mat.smooth_solve(psi, dev(src), omega=omega, **kw)
                ref_psi, ref = oracle("smooth", psi0, src, None, kw, omega=omega)
                got = host(psi)
                assert perf["nIterations"] == ref["nIterations"], what
                assert np.array_equal(got, ref_psi), (what, float(np.max(np.abs(got - ref_psi))))
                if kw["n_sweeps"] < 0:
                    assert all(perf[k] == ref[k] for k in FIELDS), (what, perf, ref)
                    assert perf["history"].size == 0 and ref["history"].size == 0, what
                    assert perf["nIterations"] == -kw["n_sweeps"], what
                else:
                    _vs_oracle(perf, got, ref, ref_psi, what)
    assert ctx.stat(S_MULTI) + ctx.stat(S_DEV) + ctx.stat(S_HOST) == 0


# ---- MI_PCG_BATCH --------------------------------------------------------------------------------------------------------------
def test_batch_below_one_is_batch_one(pkg, monkeypatch):
    """MI_PCG_BATCH=0 (or negative) is taken as 1 at mi_ctx_create: every batched loop ends, with batch 1's bits"""
    case = pkg.synthetic.box_case(21, 17, 13, symmetric=False)
    sym = pkg.synthetic.box_case(21, 17, 13)
    z = np.zeros(case.n_cells)
    kw = dict(tolerance=1e-9, maxIter=300)
    out = {}
    for batch in ("1", "0", "-4"):
        res = []
        for env in ({}, dict(MI_PBICG_MULTI="0")):
            ctx = _ctx(pkg, monkeypatch, dict(env, MI_PCG_BATCH=batch))
            addr, mat = _make(pkg, ctx, case)
            res.append(_execute(mat, "pbicg", "diagonal", [("pbicg", z, case.source, kw)]))
            res.append(_execute(mat, "pbicgstab", "diagonal", [("pbicgstab", z, case.source, kw)]))
            psis = [torch.zeros(case.n_cells, dtype=torch.float64, device="cuda:0") for _ in range(2)]
            got = mat.pbicg_multi(psis, [dev(case.source), dev(0.5 * case.source)], "diagonal", **kw)
            res.append({("multi", c): (g, host(p)) for c, (g, p) in enumerate(zip(got, psis))})
            del mat, addr, ctx
        ctx = _ctx(pkg, monkeypatch, dict(MI_PCG_BATCH=batch, MI_PCG_GRAPH="1", MI_PCG_PERSIST="0"))
        addr, mat = _make(pkg, ctx, sym)
        psi = dev(z)
        perf = mat.pcg(psi, dev(sym.source), "diagonal", **kw)
        res.append({"pcg": (perf, host(psi))})
        assert ctx.stat(5) > 0                     # the graph replay ran
        del mat, addr, ctx
        out[batch] = res
    for batch in ("0", "-4"):
        for a, b in zip(out["1"], out[batch]):
            for what in a:
                _same_bits(a[what], b[what], (batch, what))
    assert out["1"][0]["pbicg"][0]["converged"] == 1
