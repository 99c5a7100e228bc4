"""GPU (-m gpu): every single-rank PCG pipeline, and the hand-overs between them inside one session.

The engine picks a pipeline per mi_pcg_iterate call (engine.hip): the separate kernels with or without the deferred psi update,
the convergence test folded into the next p-update (MI_PCG_FUSE_FINAL), the fused residual / direction launch (pcg_fused.inc),
the hipGraph replay of mi_pcg_solve, and the persistent cooperative kernel (persist.inc) for untimed batches of small matrices.

(a) the five-launch family -- separate, no deferral, fuse-final, fused launch, graph replay, timed batches -- is the same kernels
    in the same order: results equal BIT FOR BIT, through mi_pcg_solve and through sessions with uneven batches; one member
    against the oracle.  AINV (= DIC) takes separate, no deferral and timed.
(b) the persistent kernel against the oracle (sums grouped per workgroup: to rounding).
(c) one session moving between pipelines from batch to batch -- P (persistent), S (separate), F (fused), Ts / Tf (timed, fused
    off / on) -- over all 20 ordered pairs, hand-overs at iteration 0, 1, odd and even; converging and stopping at maxIter inside
    a batch and exactly at a batch end, batches of every kind after the end.  Against the oracle; without P, bit for bit the
    single-pipeline S session; the counters say which pipeline ran.
(d) what a matrix and its context keep between solves (pA formed by the fused launch, barrier generations, the graph cache)
    changes nothing: the calls after a mixed session equal the same calls on a fresh context bit for bit."""
import numpy as np
import pytest
import torch

from conftest import random_graph_case
from test_gpu_parity import HIST_RTOL, PERSIST, _check_hist

pytestmark = pytest.mark.gpu

FIELDS = ("nIterations", "converged", "singular", "initialResidual", "finalResidual", "normFactor")
CONTROLS = (dict(tolerance=1e-9, maxIter=400), dict(tolerance=0.0, maxIter=7), dict(tolerance=1e-30, relTol=1e-3, maxIter=400),
            dict(tolerance=1e30, minIter=3, maxIter=400), dict(tolerance=0.0, maxIter=0), dict(tolerance=0.0, maxIter=1))
SESSION_BATCHES = (1, 2, 5, 3, 16)
# sessions of (a): stopped by the caller, maxIter reached inside a batch, converged (the batches after the end are no-ops)
SESSIONS = ((dict(tolerance=0.0, maxIter=30), SESSION_BATCHES), (dict(tolerance=0.0, maxIter=7), SESSION_BATCHES),
            (dict(tolerance=1e-9, maxIter=400), SESSION_BATCHES + (64, 128, 256)))
DIMS = [(1, 1, 1), (2, 1, 1), (70, 1, 1), (11, 9, 7), (40, 32, 24), "graph"]
STATS = (0, 4, 5)   # persistent launches, fused launches, graph replays (mi_ctx_stat)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _case(pkg, dims):
    return random_graph_case(pkg, 3000) if dims == "graph" else pkg.synthetic.box_case(*dims)


def _ctx(pkg, monkeypatch, env=(), **opts):
    """a context created under these switches (mi_ctx_create reads them once); persistent kernel and graph off unless asked"""
    base = dict(MI_PCG_GRAPH="0", MI_PCG_PERSIST="0", MI_PCG_BATCH="16", MI_PCG_DEFER_PSI="1", MI_PCG_FUSE_FINAL="0", MI_EVENT_ATTACH="1")
    for k, v in {**base, **dict(env)}.items():
        monkeypatch.setenv(k, v)
    ctx = pkg.engine.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("pcg_fuse_rp", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _make(pkg, ctx, case):
    eng = pkg.engine
    addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
    mat = eng.Matrix(addr)
    mat.set_coeffs(dev(case.diag), dev(case.upper), None)
    return addr, mat


def _stats(ctx):
    return np.array([ctx.stat(k) for k in STATS])


def _solve(mat, case, precond, kw, psi0=None):
    psi = torch.zeros(case.n_cells, dtype=torch.float64, device="cuda:0") if psi0 is None else dev(psi0)
    perf = mat.pcg(psi, dev(case.source), precond, **kw)
    return perf, host(psi)


def _session(mat, case, precond, kw, batches, timed=None):
    """mi_pcg_begin, one mi_pcg_iterate per batch, mi_pcg_end.  batches: lengths, or (kind, length) with kind set through
    `timed(kind)` -> (time_amul, event_stride) by the caller"""
    n = case.n_cells
    hl = kw["maxIter"] + 2
    mat.pcg_begin(dev(np.zeros(n)), dev(case.source), precond, history_len=hl, **kw)
    for b in batches:
        if isinstance(b, tuple):
            kind, k = b
            t, stride = timed(kind)
        else:
            k, (t, stride) = b, timed(None) if timed else (False, 1)
        mat.pcg_iterate(k, time_amul=t, event_stride=stride)
    pe = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    perf = mat.pcg_end(pe, hl)
    return perf, host(pe)


def _same_bits(a, b, what):
    (pa, xa), (pb, xb) = a, b
    for k in FIELDS:
        assert pa[k] == pb[k] or (np.isnan(pa[k]) and np.isnan(pb[k])), (what, k, pa[k], pb[k])
    assert np.array_equal(pa["history"], pb["history"], equal_nan=True), (what, "history")
    assert np.array_equal(xa, xb, equal_nan=True), (what, "psi", float(np.max(np.abs(xa - xb))))


def _psi_close(x, xr, what, rel=1e-9):
    assert np.max(np.abs(x - xr)) <= rel * max(np.max(np.abs(xr)), 1e-300), (what, float(np.max(np.abs(x - xr))))


ROUNDING = 1e-8   # (of the initial residual) below it a history entry is decided by rounding (see _near_oracle)


def _near_oracle(perf, psi, ref, ref_psi, what, history=True):
    """the bar of the persistent tests: same iteration count and flags, history within HIST_RTOL of the initial residual,
    psi to 1e-9.  Entries the oracle itself puts below ROUNDING x the initial residual only have to stay below it: a one- or
    two-cell system is solved exactly in its first iterations and goes on at 1e-17 .. 1e-65.  history=False: the
    unpreconditioned 70-cell line, which ends by finite termination (70 iterations for 70 unknowns): rounding decides its last
    residuals, 1.8e-9 of the initial residual apart between the oracle and every pipeline (measured), while the iteration
    counts, the flags and psi (2e-11) agree -- its histories are compared bit for bit between the pipelines only"""
    assert (perf["nIterations"], perf["converged"], perf["singular"]) == (ref["nIterations"], ref["converged"], ref["singular"]), \
        (what, perf["nIterations"], ref["nIterations"], perf["converged"], ref["converged"], perf["singular"], ref["singular"])
    h, hr = perf["history"], ref["history"]
    assert h.shape == hr.shape, (what, "history")
    if history:
        bar = np.where(np.abs(hr) < ROUNDING * hr[0], ROUNDING, HIST_RTOL) * hr[0]
        assert np.all(np.abs(h - hr) < bar), (what, "history", float(np.max(np.abs(h - hr) / hr[0])))
    _psi_close(psi, ref_psi, what)


def _rounding_decides(dims, precond):
    return dims == (70, 1, 1) and precond == "none"


def _vs_oracle(perf, psi, ref, ref_psi, dims, precond, persistent, what):
    """_check_hist of test_gpu_parity.py where its relative bars apply -- histories that stay clear of rounding (the persistent
    kernel, and the long unpreconditioned 40 x 32 x 24 solve that ends at 1e-9: its PERSIST floor); _near_oracle elsewhere"""
    if dims in ((11, 9, 7), (40, 32, 24), "graph"):
        _check_hist(perf, ref, **(PERSIST if persistent or (dims, precond) == ((40, 32, 24), "none") else {}))
        _psi_close(psi, ref_psi, what)
    else:
        _near_oracle(perf, psi, ref, ref_psi, what, history=not _rounding_decides(dims, precond))


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def _pipelines(precond):
    """name -> (environment, options, what it runs: 'solve' / 'session' / both, timed batches: (time_amul, event_stride))"""
    untimed = (False, 1)
    p = {"separate": ({}, {}, "both", untimed),
         "no deferral": (dict(MI_PCG_DEFER_PSI="0"), {}, "both", untimed)}
    for attach, stride, fuse in (("1", 1, 0), ("1", 3, 1), ("0", 1, 1), ("0", 3, 0)):
        p[f"timed attach={attach} stride={stride} fuse={fuse}"] = (dict(MI_EVENT_ATTACH=attach), dict(pcg_fuse_rp=fuse), "session", (True, stride))
    if precond != "AINV":
        p["fuse-final"] = (dict(MI_PCG_FUSE_FINAL="1"), {}, "both", untimed)
        p["fused launch"] = ({}, dict(pcg_fuse_rp=1), "both", untimed)
        for batch in ("3", "16"):
            p[f"graph batch={batch}"] = (dict(MI_PCG_GRAPH="1", MI_PCG_BATCH=batch), {}, "solve", untimed)
    return p


@pytest.mark.parametrize("precond", ["diagonal", "none", "AINV"])
@pytest.mark.parametrize("dims", DIMS)
def test_five_launch_family_is_bit_identical(pkg, orc, dims, precond, monkeypatch):
    case = _case(pkg, dims)
    n = case.n_cells
    out = {}
    for name, (env, opts, runs, timed) in _pipelines(precond).items():
        ctx = _ctx(pkg, monkeypatch, env, **opts)
        addr, mat = _make(pkg, ctx, case)
        s0 = _stats(ctx)
        res = {}
        if runs in ("solve", "both"):
            for i, kw in enumerate(CONTROLS):
                res["solve", i] = _solve(mat, case, precond, kw)
        if runs in ("session", "both"):
            for i, (kw, batches) in enumerate(SESSIONS):
                res["session", i] = _session(mat, case, precond, kw, batches, timed=lambda kind: timed)
        d0, d4, d5 = _stats(ctx) - s0
        assert d0 == 0, (name, "persistent kernel ran")
        assert (d4 > 0) == (name == "fused launch" or (precond != "AINV" and "fuse=1" in name)), (name, d4)
        assert (d5 > 0) == name.startswith("graph"), (name, d5)      # the graph replay ran exactly where asked
        out[name] = res
        del mat, addr, ctx
    ref = out["separate"]
    for name, res in out.items():
        for key, r in res.items():
            _same_bits(ref[key], r, (name, key))
    # the family against the oracle (PCG.C:105-204): a bug they all share must not pass
    S = orc.System([case])
    for i, kw in enumerate(CONTROLS):
        ref_psi, r = S.pcg(np.zeros(n), case.source, precond, **kw)
        _vs_oracle(*ref["solve", i], r, ref_psi, dims, precond, False, kw)


@pytest.mark.parametrize("precond", ["diagonal", "none"])
def test_graph_pipeline_above_the_persistent_limit(pkg, orc, precond, monkeypatch):
    """120^3 = 1.73 M cells: too large for the persistent kernel, so mi_pcg_solve takes the graph replay (the counters say so);
    bit for bit the separate kernels and the fused launch, batch ends before, on and after maxIter"""
    case = pkg.synthetic.box_case(120, 120, 120)
    controls = (dict(tolerance=0.0, maxIter=7), dict(tolerance=0.0, maxIter=0), dict(tolerance=0.0, maxIter=1),
                dict(tolerance=1e30, minIter=3, maxIter=400), dict(tolerance=1e-30, relTol=1e-2, maxIter=400))
    out = {}
    for name, env, opts in (("separate", {}, {}), ("fused launch", {}, dict(pcg_fuse_rp=1)),
                            ("graph batch=3", dict(MI_PCG_GRAPH="-1", MI_PCG_PERSIST="1", MI_PCG_BATCH="3"), dict(pcg_fuse_rp=1)),
                            ("graph batch=16", dict(MI_PCG_GRAPH="-1", MI_PCG_PERSIST="1"), dict(pcg_fuse_rp=1))):
        ctx = _ctx(pkg, monkeypatch, env, **opts)
        addr, mat = _make(pkg, ctx, case)
        res = []
        for kw in controls:
            s0 = _stats(ctx)
            res.append(_solve(mat, case, precond, kw))
            d0, d4, d5 = _stats(ctx) - s0
            assert d0 == 0 and (d5 > 0) == name.startswith("graph") and (d4 > 0) == (name == "fused launch"), (name, kw, d0, d4, d5)
        out[name] = res
        del mat, addr, ctx
    for name, res in out.items():
        for kw, a, b in zip(controls, out["separate"], res):
            _same_bits(a, b, (name, kw))
    ref_psi, ref = orc.System([case]).pcg(np.zeros(case.n_cells), case.source, precond, tolerance=0.0, maxIter=7)
    _near_oracle(*out["graph batch=16"][0], ref, ref_psi, "graph vs oracle")


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["diagonal", "none"])
@pytest.mark.parametrize("dims", DIMS)
def test_persistent_kernel_against_the_oracle(pkg, orc, dims, precond, monkeypatch):
    case = _case(pkg, dims)
    n = case.n_cells
    ctx = _ctx(pkg, monkeypatch, dict(MI_PCG_PERSIST="1"), pcg_fuse_rp=1)
    addr, mat = _make(pkg, ctx, case)
    S = orc.System([case])
    for kw in CONTROLS:
        s0 = _stats(ctx)
        perf, psi = _solve(mat, case, precond, kw)
        d0, d4, d5 = _stats(ctx) - s0
        assert d0 > 0 and d4 == 0 and d5 == 0, (kw, d0, d4, d5)
        ref_psi, ref = S.pcg(np.zeros(n), case.source, precond, **kw)
        _vs_oracle(perf, psi, ref, ref_psi, dims, precond, True, kw)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
# P: untimed, persistent kernel on (fused launch on, as a context starts); S: untimed, persistent off, fused off; F: untimed,
# persistent off, fused on; Ts / Tf: timed (mi_pcg_iterate_sampled), fused off / on.  Every ordered pair of the five follows each
# other at least once, P -> X with a P batch that really ran the persistent kernel (see _expected).
SEQ = "S F S Ts S Tf S P S F Ts F Tf F P S Ts Tf Ts P Tf P S P Ts P F".split()
LENS = (1, 2, 3, 5)
KINDS = ("P", "S", "F", "Ts", "Tf")


def _switch(ctx, kind):
    ctx.set_option("pcg_persist", int(kind == "P"))
    ctx.set_option("pcg_fuse_rp", int(kind in ("P", "F", "Tf")))
    return (kind in ("Ts", "Tf"), 1 + (kind == "Tf"))


def _expected(batches):
    """counter growth per batch (persistent launches, fused launches).  A P batch after a batch that ended in the fused launch
    (pA of the next iteration formed already) stays with pcg_enqueue -- the fused launch here, since P keeps it on"""
    ready, out = False, []
    for kind, k in batches:
        if kind == "P" and not ready:
            out.append((1, 0))
        else:
            fused = kind in ("P", "F", "Tf")
            out.append((0, k if fused else 0))
            ready = fused
    return out


def _sequence(seq, n_iters):
    lens = [LENS[i % len(LENS)] for i in range(len(seq))]
    reps = 1
    while reps * sum(lens) < n_iters:
        reps += 1
    return [(kind, k) for _ in range(reps) for kind, k in zip(seq, lens)]


def _mixed_session(ctx, mat, case, precond, kw, batches):
    """the session, and the counter growth of each batch"""
    n = case.n_cells
    hl = kw["maxIter"] + 2
    mat.pcg_begin(dev(np.zeros(n)), dev(case.source), precond, history_len=hl, **kw)
    grew = []
    for kind, k in batches:
        t, stride = _switch(ctx, kind)
        s0 = _stats(ctx)
        mat.pcg_iterate(k, time_amul=t, event_stride=stride)
        d = _stats(ctx) - s0
        grew.append((int(d[0]), int(d[1])))
    pe = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    perf = mat.pcg_end(pe, hl)
    return (perf, host(pe)), grew


def _oracle(S, case, precond, kw, n_iters, cache):
    """the reference's loop stopped after n_iters bodies at most (a session that ends earlier ends where the solve would)"""
    kw2 = dict(kw, maxIter=min(kw["maxIter"], n_iters - 1))
    key = tuple(sorted(kw2.items()))
    if key not in cache:
        ref_psi, ref = S.pcg(np.zeros(case.n_cells), case.source, precond, **kw2)
        cache[key] = (ref, ref_psi)
    return cache[key]


@pytest.mark.parametrize("precond", ["diagonal", "none"])
@pytest.mark.parametrize("dims", DIMS)
def test_pipeline_hand_overs_inside_one_session(pkg, orc, dims, precond, monkeypatch):
    case = _case(pkg, dims)
    S = orc.System([case])
    n_conv = S.pcg(np.zeros(case.n_cells), case.source, precond, tolerance=1e-9, maxIter=400)[1]["nIterations"]
    ctx = _ctx(pkg, monkeypatch, dict(MI_PCG_PERSIST="1"))
    addr, mat = _make(pkg, ctx, case)
    no_p = [k for k in SEQ if k != "P"]
    no_p = [k for i, k in enumerate(no_p) if i == 0 or k != no_p[i - 1]]
    cache = {}
    for kw, total in ((dict(tolerance=0.0, maxIter=80), 1), (dict(tolerance=1e-9, maxIter=400), n_conv + 1), (dict(tolerance=0.0, maxIter=40), 41)):
        for seq in (SEQ, no_p):
            full = _sequence(seq, total) + _sequence(seq, 1)[: len(seq)] if total > 1 else _sequence(seq, 1)
            # end after the last batch of every kind, and after the last batch
            ends = sorted({max(i for i, (kd, _) in enumerate(full) if kd == kind) + 1 for kind in set(seq)} | {len(full)})
            done_at, after_done = None, None
            for e in ends:
                batches = full[:e]
                n_it = sum(k for _, k in batches)
                got, grew = _mixed_session(ctx, mat, case, precond, kw, batches)
                what = (kw, " ".join(seq) == " ".join(SEQ), e, batches[-1][0])
                ref, ref_psi = _oracle(S, case, precond, kw, n_it, cache)
                _near_oracle(*got, ref, ref_psi, what, history=not _rounding_decides(dims, precond))
                if "P" not in seq:   # the same kernels as the single-pipeline S session: the same bits
                    untimed = _switch(ctx, "S")
                    plain = _session(mat, case, precond, kw, [k for _, k in batches], timed=lambda kind: untimed)
                    _same_bits(plain, got, what)
                # once the device reports done, psi and the history do not move whatever the later batches run
                if got[0]["nIterations"] < n_it:   # (the device stopped before the last batch: converged, maxIter or singular)
                    if after_done is None:
                        after_done = got
                    else:
                        _same_bits(after_done, got, what + ("after the end",))
                assert grew == _expected(batches), (what, grew, _expected(batches))
            if kw["tolerance"] > 0:
                assert after_done is not None, "the converging session must go on after convergence"


@pytest.mark.parametrize("stop", ["converged", "maxIter"])
@pytest.mark.parametrize("precond", ["diagonal", "none"])
@pytest.mark.parametrize("dims", [(11, 9, 7), "graph"])
def test_hand_over_exactly_at_the_end_of_the_solve(pkg, orc, dims, precond, stop, monkeypatch):
    """the batch of kind X ends with the iteration that ends the solve, a batch of kind Y follows: nothing may move (a psi term
    the deferred update still owes is added exactly once); every ordered pair, and ending right after X as the reference"""
    case = _case(pkg, dims)
    S = orc.System([case])
    if stop == "converged":
        kw = dict(tolerance=1e-9, maxIter=400)
        n_end = S.pcg(np.zeros(case.n_cells), case.source, precond, **kw)[1]["nIterations"]
    else:
        kw = dict(tolerance=0.0, maxIter=12)
        n_end = 13
    ref_psi, ref = S.pcg(np.zeros(case.n_cells), case.source, precond, **kw)
    ctx = _ctx(pkg, monkeypatch, dict(MI_PCG_PERSIST="1"))
    addr, mat = _make(pkg, ctx, case)
    for x in KINDS:
        alone, _ = _mixed_session(ctx, mat, case, precond, kw, [(x, n_end - 1), (x, 1)])
        _near_oracle(*alone, ref, ref_psi, (x, "alone"))
        for y in KINDS:
            if y == x:
                continue
            batches = [(x, n_end - 1), (x, 1), (y, 2), (y, 1)]
            got, grew = _mixed_session(ctx, mat, case, precond, kw, batches)
            _same_bits(alone, got, (x, y))
            assert grew == _expected(batches), (x, y, grew)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["diagonal", "none"])
@pytest.mark.parametrize("dims", [(40, 32, 24), "graph"])
def test_state_carried_across_solves(pkg, dims, precond, monkeypatch):
    """a mixed session leaves pcgPReady set (it ends in the fused launch), the fused barrier at some generation, the persistent
    kernel's barrier words at another and a graph in the cache: the solves and the session after it equal the same calls on a
    fresh context bit for bit"""
    case = _case(pkg, dims)
    env = dict(MI_PCG_PERSIST="1", MI_PCG_GRAPH="1")
    kw = dict(tolerance=1e-9, maxIter=400)
    later = [("F", 2), ("P", 3), ("S", 1), ("Tf", 2), ("P", 1)]

    def after(ctx, mat):
        res, grew = [], []
        for persist, fuse in ((0, 1), (1, 1), (0, 0)):   # graph replay, persistent kernel, graph replay again
            ctx.set_option("pcg_persist", persist)
            ctx.set_option("pcg_fuse_rp", fuse)
            s0 = _stats(ctx)
            res.append(_solve(mat, case, precond, kw))
            grew.append(tuple(int(v > 0) for v in _stats(ctx) - s0))
        r, g = _mixed_session(ctx, mat, case, precond, dict(tolerance=0.0, maxIter=30), later)
        return res + [r], grew + g

    ctx = _ctx(pkg, monkeypatch, env)
    addr, mat = _make(pkg, ctx, case)
    ctx.set_option("pcg_persist", 0)
    _solve(mat, case, precond, kw)                                                 # a graph in the cache (the key of the solves below)
    _mixed_session(ctx, mat, case, precond, dict(tolerance=0.0, maxIter=60), _sequence(SEQ, 1)[:-1] + [("F", 3)])
    got, grew = after(ctx, mat)
    ctx2 = _ctx(pkg, monkeypatch, env)
    addr2, mat2 = _make(pkg, ctx2, case)
    fresh, grew2 = after(ctx2, mat2)
    for i, (a, b) in enumerate(zip(fresh, got)):
        _same_bits(a, b, i)
    assert grew[:3] == grew2[:3] == [(0, 0, 1), (1, 0, 0), (0, 0, 1)], (grew, grew2)
