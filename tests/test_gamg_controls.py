"""GAMG: mi_gamg_solve at every control edge of its host-driven V-cycle -- sweep schedules and their caps, the pre-smoothing branch,
levels with and without post sweeps in one cycle, no finest sweeps, omega, relTol, the maxIter / minIter loop, a history longer than the
caller's buffer, converged starts, forced cycles on exact and all-zero systems, hierarchies of one to three levels, coupled patches, and one
hierarchy's cached cycle graph across changing controls and matrices.  The reference of every GPU test is the oracle's V-cycle; the CPU
tests pin that V-cycle, bit for bit, to the reference's compiled GAMGSolver::solve (tests/golden/golden_ref_gamg_controls.npz)."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_ref as mg  # noqa: E402

ROWS = mg.GAMG_CONTROL_ROWS
SYM = [True, False]
N_LEVELS_F = 6                                    # 960 cells -> coarse levels of 480, 240, 120, 60, 30, 15: five of them are smoothed


def _schedule(kw, which, n_levels=N_LEVELS_F):
    """sweeps on coarse levels 0 .. coarsest-1: min(n + multiplier*l, max) (GAMGSolverSolve.C:221-225, 402-406)"""
    ctl = dict(nPreSweeps=0, preSweepsLevelMultiplier=1, maxPreSweeps=4, nPostSweeps=2, postSweepsLevelMultiplier=1, maxPostSweeps=4)
    ctl.update({k: v for k, v in kw.items() if k in ctl})
    n, m, cap = (ctl[f"n{which}Sweeps"], ctl[f"{which.lower()}SweepsLevelMultiplier"], ctl[f"max{which}Sweeps"])
    if which == "Pre" and n == 0:                 # `if (nPreSweeps_)`: the whole pre-smoothing branch is off
        return [0] * (n_levels - 1)
    return [min(n + m * l, cap) for l in range(n_levels - 1)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def _c_fields(text, opening, closing):
    """[(type, name)] of the struct between `opening` and `closing` in a C source text"""
    body = text[text.index(opening) + len(opening):]
    body = body[:body.index(closing)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip().lstrip("{").strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        out += [({"scalar": "double"}.get(typ, typ), n.strip()) for n in names.split(",")]
    return out


def test_gamg_controls_structures_agree_and_the_table_reaches_its_edges(pkg, orc):
    """The engine's and the oracle's GamgControls (ctypes), mi_gamg_controls of include/mi_ldu.h, the oracle's C struct and the struct the
    reference's solver is driven through list the same fields in the same order with the same types, and both gamg_controls() give the
    defaults of GAMGSolver.C:67-77.  Then the sweep schedules the table of control rows is there for are derived from its controls by the
    min(n + multiplier*l, max) rule: an edit of a row cannot silently stop reaching its edge."""
    root = os.path.dirname(HERE)
    read = lambda *p: open(os.path.join(root, *p)).read()
    header = read("include", "mi_ldu.h")
    header = header[:header.index("} mi_gamg_controls;") + len("} mi_gamg_controls;")]
    h = _c_fields(header[header.rindex("typedef struct {"):], "typedef struct {", "} mi_gamg_controls;")
    o_src = read("oracle", "gamg_oracle.c")
    o_src = o_src[:o_src.index("} gamg_controls;") + len("} gamg_controls;")]
    o = _c_fields(o_src[o_src.rindex("typedef struct {"):], "typedef struct {", "} gamg_controls;")
    r = _c_fields(read("oracle", "ref_shim", "ref_gamg_tu.cpp"), "struct gamg_controls_c {", "};")
    ctype = {C.c_double: "double", C.c_int32: "int32_t"}
    e_py = [(ctype[t], n) for n, t in pkg.engine.GamgControls._fields_]
    o_py = [(ctype[t], n) for n, t in orc.GamgControls._fields_]
    assert len(h) == 15 and h == o == r == e_py == o_py
    assert C.sizeof(pkg.engine.GamgControls) == C.sizeof(orc.GamgControls) == 72
    defaults = dict(tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0, nPreSweeps=0, preSweepsLevelMultiplier=1, maxPreSweeps=4, nPostSweeps=2,
                    postSweepsLevelMultiplier=1, maxPostSweeps=4, nFinestSweeps=2, scaleCorrection=-1, omega=0.9, directSolveCoarsest=1, reserved=0)
    for make in (pkg.engine.gamg_controls, orc.gamg_controls):
        d = make()
        assert {n: getattr(d, n) for _, n in e_py} == defaults
        # keyword by keyword into its own field (a transposed pair in the positional constructor would pass the defaults)
        for k, (_, n) in enumerate(e_py[:-1]):
            v = 0.25 + k if n in ("tolerance", "relTol", "omega") else 20 + k
            got = make(**{n: v})
            want = dict(defaults); want[n] = 1 if n == "directSolveCoarsest" else v
            assert {f: getattr(got, f) for _, f in e_py} == want, n

    assert sorted(ROWS) == sorted([f"S{i}" for i in range(1, 13)] + ["X1", "X2"] + [f"C{i}" for i in range(1, 9)])
    pre, post = (lambda i: _schedule(ROWS[i], "Pre")), (lambda i: _schedule(ROWS[i], "Post"))
    assert post("X1") == [2, 3, 4, 4, 4] and pre("X1") == [0] * 5            # the defaults reach their cap on the 6 levels of F
    assert pre("S1") == [2, 4, 5, 5, 5] and {s % 2 for s in pre("S1")} == {0, 1}
    assert pre("S2") == [1] * 5
    assert ROWS["S3"]["nPreSweeps"] >= 1 and pre("S3") == [0] * 5            # the branch is taken (nPreSweeps != 0) with zero sweeps
    assert post("S4") == [0, 1, 2, 3, 4]                                       # level 0 unfused, the others fused
    assert post("S5") == [0] * 5 and ROWS["S5"].get("nFinestSweeps", 2) == 2
    assert post("S6") == [1] * 5 and ROWS["S6"].get("nPostSweeps", 2) > ROWS["S6"]["maxPostSweeps"]
    assert post("S7") == [0] * 5 and ROWS["S7"].get("nPostSweeps", 2) > 0
    assert post("S8") == [1, 3, 3, 3, 3] and ROWS["S8"]["nFinestSweeps"] % 2 == 1
    assert ROWS["S9"]["nFinestSweeps"] == 0 and post("S9") == [2, 3, 4, 4, 4]
    assert ROWS["S10"]["nFinestSweeps"] == 0 and post("S10") == [0] * 5 and pre("S10") == [0] * 5
    assert ROWS["S11"]["omega"] == 1.0 and ROWS["S12"]["omega"] == 0.6
    assert (ROWS["X1"]["scaleCorrection"], ROWS["X2"]["scaleCorrection"]) == (1, 0)
    assert ROWS["C1"]["relTol"] > 0 and ROWS["C2"]["relTol"] > 0 and ROWS["C2"]["tolerance"] == 0.0
    assert (ROWS["C3"]["maxIter"], ROWS["C4"]["maxIter"]) == (0, 1)
    assert ROWS["C7"]["minIter"] == ROWS["C7"]["maxIter"] + 1 and ROWS["C8"]["minIter"] + 1 > ROWS["C8"]["maxIter"] + 2   # history entries > buffer

    # the inputs have the depths the rows are written for
    for sym in SYM:
        case = mg.gamg_case_F(pkg, sym)
        H = orc.GamgHierarchy(case, orc.box_face_weights(case), 10)
        assert [H.level(l)["n_coarse"] for l in range(H.n_levels)] == [480, 240, 120, 60, 30, 15] and H.level(0)["n_fine"] == 960 and H.n_levels == N_LEVELS_F
        for dims, depth in zip(mg.GAMG_SHALLOW_DIMS, (1, 2, 3)):
            sc = pkg.synthetic.box_case(*dims, symmetric=sym)
            assert orc.GamgHierarchy(sc, orc.box_face_weights(sc), 12).n_levels == depth
        cc = mg.gamg_case_coupled(pkg, sym)
        assert orc.GamgSysHierarchy(orc.System([cc]), [orc.box_face_weights(cc)], 10).n_levels == 7
        nl = pkg.synthetic.box_case(3, 2, 2, symmetric=sym)
        assert orc.GamgHierarchy(nl, orc.box_face_weights(nl), 50).n_levels == 0


def test_oracle_vcycle_equals_the_reference_at_every_control_edge(pkg, orc):
    """tests/golden/golden_ref_gamg_controls.npz holds psi and solverPerformance of the reference's GAMGSolver::solve (GAMGSolverSolve.C
    compiled from the reference tree against oracle/ref_shim, generator tests/golden/make_golden_ref.py build_gamg_controls) for every row
    of the control table on the 6-level box, the exact and all-zero systems, the 1-, 2- and 3-level boxes and the cyclic box, symmetric
    and asymmetric.  The oracle's own V-cycle gives the same bits for every key -- so the GPU tests below, which compare the engine with
    the oracle, are pinned to the reference.  (directSolveCoarsest=False is not in the fixture: the reference's ICCG / BICCG are not
    compiled.)"""
    G = np.load(os.path.join(HERE, "golden", "golden_ref_gamg_controls.npz"))
    n = 0
    for key, S, H, start, src, kw in mg.gamg_control_runs(pkg, orc):
        x, p = H.solve(start, src, **kw)
        ref = G[key + "/perf"]
        assert np.array_equal(x, G[key + "/psi"]), key
        assert p["initialResidual"] == ref[0] and p["finalResidual"] == ref[1] and p["nIterations"] == int(ref[2]) and bool(p["converged"]) == bool(ref[3]), key
        n += 1
    assert n == 2 * (len(ROWS) + 2 * len(mg.GAMG_FORCED_CONTROLS) + len(mg.GAMG_SHALLOW_DIMS) * len(mg.GAMG_SHALLOW_CONTROLS) + len(mg.GAMG_COUPLED_ROWS)) == 98
    assert len(G.files) == 2 * n
    if orc.ref_gamg_available():      # and live, where the reference build is present
        now = mg.build_gamg_controls(pkg, orc)
        assert sorted(now) == sorted(G.files)
        for k in G.files:
            assert np.array_equal(now[k], G[k]), k


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(pkg, orc, name, sym):
    """(case, weights, oracle hierarchy) of a named input, built once"""
    key = (name, sym)
    if key not in _ORACLE:
        if name == "F":
            case = mg.gamg_case_F(pkg, sym); nc = 10
        elif name == "coupled":
            case = mg.gamg_case_coupled(pkg, sym); nc = 10
        else:
            case = pkg.synthetic.box_case(*name, symmetric=sym); nc = 12
        w = orc.box_face_weights(case)
        H = orc.GamgSysHierarchy(orc.System([case]), [w], nc) if name == "coupled" else orc.GamgHierarchy(case, w, nc)
        _ORACLE[key] = (case, w, H, nc, {})
    return _ORACLE[key]


def _ref(pkg, orc, name, sym, args, start=None, source=None, tag="zero"):
    """the oracle's solve of a named input, computed once per (input, start, controls)"""
    case, w, H, nc, solves = _oracle(pkg, orc, name, sym)
    key = (tag, tuple(sorted(args.items())))
    if key not in solves:
        solves[key] = H.solve(np.zeros(case.n_cells) if start is None else start, case.source if source is None else source, **args)
    return solves[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _engine(pkg, case, w, nc, mode=None):
    """context, addressing, bound matrix and hierarchy; mode 'cyclic' / 'processor_to_self' as in test_engine_gamg_coupled_patches"""
    import torch
    eng = pkg.engine
    ctx = eng.Context(0, torch.cuda.current_stream().cuda_stream)
    fcs = [i.face_cells for i in case.interfaces]
    if mode == "cyclic":
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, fcs, [case.interfaces[i.nbr_patch].face_cells for i in case.interfaces])
    elif mode == "processor_to_self":
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, fcs)
    else:
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
    mat = _matrix(pkg, addr, case)
    comm = None
    if mode == "processor_to_self":
        comm = eng.Comm(ctx, 1, 0, eng.Comm.unique_id())
        mat.attach_comm(comm, comm, [0, 0], [1, 0], n_global=case.n_cells)
        G = eng.Gamg(addr, w, nc, comms=(comm, comm), patch_rank=[0, 0], patch_nbr_patch=[1, 0])
    else:
        G = eng.Gamg(addr, w, nc)
    return ctx, addr, mat, G, comm


def _matrix(pkg, addr, case):
    mat = pkg.engine.Matrix(addr)
    mat.set_coeffs(_dev(case.diag), _dev(case.upper), None if case.lower is None else _dev(case.lower))
    for p, itf in enumerate(case.interfaces):
        mat.set_interface_coeffs(p, _dev(itf.bou_coeffs), None if case.lower is None else _dev(itf.int_coeffs))
    return mat


def _check(perf, psi, ref_psi, ref, label=""):
    """test_engine_gamg_history's bars: counts and flags equal, history within 1e-10 of the initial residual, psi within 1e-9"""
    h, hr = perf["history"], ref["history"]
    print(f"{label}: nIterations {perf['nIterations']} / {ref['nIterations']}, converged {perf['converged']} / {ref['converged']}, history {h.shape} / {hr.shape}"
          + (f", max|h - hr| / hr[0] = {np.max(np.abs(h - hr)) / hr[0]:.3e}" if h.shape == hr.shape and hr[0] > 0 else "")
          + f", max|psi - ref| / max|ref| = {np.max(np.abs(psi - ref_psi)) / max(np.max(np.abs(ref_psi)), 1e-300):.3e}")
    assert perf["nIterations"] == ref["nIterations"] and bool(perf["converged"]) == bool(ref["converged"])
    assert h.shape == hr.shape
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(psi))
    assert np.max(np.abs(h - hr)) < 1e-10 * hr[0]
    if np.max(np.abs(ref_psi)) == 0.0:               # (a zero solution has no scale to be relative to: the same bits)
        assert np.array_equal(psi, ref_psi)
    else:
        assert np.max(np.abs(psi - ref_psi)) < 1e-9 * np.max(np.abs(ref_psi))


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("rid", list(ROWS))
def test_engine_gamg_control_rows(pkg, orc, rid, sym):
    """Every row of the control table on the 6-level box, zero start: levels, cycle count, converged flag, history shape, history and
    psi follow the oracle (hr[0] is 1 with a zero start: normFactor is the initial residual's own sum)."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", sym)
    args = mg.gamg_args(ROWS[rid])
    ref_psi, ref = _ref(pkg, orc, "F", sym, args)
    ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
    assert G.n_levels == H.n_levels
    start = np.zeros(case.n_cells)
    psi = _dev(start)
    b = _dev(case.source)
    perf = G.solve(mat, psi, b, **args)
    x = _host(psi)
    assert abs(ref["history"][0] - 1.0) < 1e-12
    _check(perf, x, ref_psi, ref, f"{rid} sym={sym}")
    if rid in ("C3", "C4"):
        assert perf["nIterations"] == 1 and not perf["converged"]          # ++nIterations < maxIter: one cycle before the test
    if rid == "C5":
        assert perf["nIterations"] == 0 and perf["converged"] and np.array_equal(x, start) and perf["history"].shape == (1,)
    if rid == "C6":
        assert perf["nIterations"] == 3 and perf["converged"]
    if rid == "C7":
        assert perf["nIterations"] == 3 and not perf["converged"]
    if rid == "C8":
        # 7 history entries against the wrapper's buffer of maxIter + 2 = 4: the first four, and nothing behind them
        assert perf["nIterations"] == 6 and perf["history"].shape == (4,)
        eng = pkg.engine
        ctl = eng.gamg_controls(**args)
        hist_len = ctl.maxIter + 2
        guard = np.full(hist_len + 12, np.nan)
        psi2 = _dev(start)
        p2 = eng.SolverPerf()
        eng._chk(eng.lib().mi_gamg_solve(G.h, mat.h, eng._ptr(psi2), eng._ptr(b), C.byref(ctl), C.byref(p2),
                                         guard.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(hist_len)))
        assert p2.nIterations == 6
        assert np.array_equal(guard[:hist_len], perf["history"]) and np.all(np.isnan(guard[hist_len:]))
        assert np.array_equal(_host(psi2), x)


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("rid", ["S1", "S4", "S8", "S9"])
def test_engine_gamg_control_rows_without_graph_and_without_fusion(pkg, orc, rid, sym, monkeypatch):
    """Odd and even pre sweeps, fused beside unfused levels, an odd finest count and no finest sweep: the eagerly enqueued cycles
    (MI_GAMG_GRAPH=0) and the cycle of separate transfer kernels (MI_GAMG_FUSE=0) give the default run's bits, history and psi."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", sym)
    args = mg.gamg_args(ROWS[rid])
    got = {}
    for name, env in (("default", {}), ("eager", {"MI_GAMG_GRAPH": "0"}), ("unfused", {"MI_GAMG_FUSE": "0"})):
        for k in ("MI_GAMG_GRAPH", "MI_GAMG_FUSE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
        psi = _dev(np.zeros(case.n_cells))
        perf = G.solve(mat, psi, _dev(case.source), **args)
        got[name] = (perf["history"], _host(psi), perf["nIterations"])
    assert got["default"][2] >= 3                       # a replayed cycle really ran
    for name in ("eager", "unfused"):
        assert got[name][2] == got["default"][2], name
        assert np.array_equal(got[name][0], got["default"][0]) and np.array_equal(got[name][1], got["default"][1]), name


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("rid", ["S1", "S4"])
def test_engine_gamg_iterative_coarsest_with_control_rows(pkg, orc, rid, sym):
    """directSolveCoarsest=False (PCG / PBiCG on the coarsest level, GAMGSolverSolve.C:572-613) with pre-smoothing and with an
    unsmoothed level.  Against the oracle's restatement ONLY: the reference's ICCG / BICCG are not compiled, so the fixture of
    the reference's own solve has no such run.  relTol stays 0: a loose inner solve would make its iteration count a rounding question."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", sym)
    args = mg.gamg_args(dict(ROWS[rid], directSolveCoarsest=False))
    assert args.get("relTol", 0.0) == 0.0
    ref_psi, ref = _ref(pkg, orc, "F", sym, args)
    ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
    psi = _dev(np.zeros(case.n_cells))
    perf = G.solve(mat, psi, _dev(case.source), **args)
    _check(perf, _host(psi), ref_psi, ref, f"iterative {rid} sym={sym}")
    assert ref["converged"]


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("k", range(len(mg.GAMG_FORCED_CONTROLS)))
@pytest.mark.parametrize("kind", ["exact", "zero"])
def test_engine_gamg_exact_and_zero_systems(pkg, orc, kind, k, sym):
    """A start that solves the system exactly (initial residual 0) and the all-zero system (normFactor = SMALL = 1e-20): no cycle
    without minIter, and forced cycles -- the scaling factor is 0/stabilise(0, VSMALL) or a quotient of rounding noise -- stay finite
    and follow the oracle.  hr[0] is 0 here, so the history bar is absolute: 1e-10 in units of the normalised residual."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", sym)
    kw = mg.GAMG_FORCED_CONTROLS[k]
    args = mg.gamg_args(kw)
    if kind == "exact":
        start, source = mg.gamg_exact_system(pkg, orc, case)
    else:
        start = source = np.zeros(case.n_cells)
    ref_psi, ref = _ref(pkg, orc, "F", sym, args, start, source, tag=kind)
    ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
    psi = _dev(start)
    perf = G.solve(mat, psi, _dev(source), **args)
    x = _host(psi)
    h, hr = perf["history"], ref["history"]
    print(f"{kind} {kw} sym={sym}: nIterations {perf['nIterations']} / {ref['nIterations']}, history {h} / {hr}, normFactor {perf['normFactor']}, "
          f"max|psi - ref| = {np.max(np.abs(x - ref_psi)):.3e}")
    assert hr[0] == 0.0
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(x)) and np.isfinite(perf["finalResidual"]) and np.isfinite(perf["normFactor"])
    assert perf["nIterations"] == ref["nIterations"] and bool(perf["converged"]) == bool(ref["converged"])
    assert perf["nIterations"] == {0: 0, 1: 1, 2: 3, 3: 2}[k]
    assert h.shape == hr.shape and np.max(np.abs(h - hr)) < 1e-10
    if not kw:
        assert np.array_equal(x, start)                                   # untouched bit for bit
    if kind == "exact":
        assert np.max(np.abs(x - ref_psi)) < 1e-9 * np.max(np.abs(ref_psi))
    else:
        assert perf["normFactor"] == 1e-20 == ref["normFactor"]
        assert np.all(h == 0.0) and np.all(x == 0.0) and np.all(ref_psi == 0.0)


SHALLOW_CONTROLS = mg.GAMG_SHALLOW_CONTROLS + [dict(directSolveCoarsest=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("k", range(len(SHALLOW_CONTROLS)))
@pytest.mark.parametrize("dims", mg.GAMG_SHALLOW_DIMS)
def test_engine_gamg_shallow_hierarchies(pkg, orc, dims, k, sym):
    """Hierarchies of one, two and three levels: with one level lev[0] is the coarsest (no restriction between levels, no level is
    smoothed), with two `l < coarsest - 1` never holds (no level is scaled), with three exactly one level is.  The last control set,
    directSolveCoarsest=False, rests on the oracle's restatement alone (the reference's ICCG / BICCG are not compiled)."""
    case, w, H, nc, _ = _oracle(pkg, orc, dims, sym)
    args = mg.gamg_args(SHALLOW_CONTROLS[k])
    ref_psi, ref = _ref(pkg, orc, dims, sym, args)
    ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
    assert G.n_levels == H.n_levels == mg.GAMG_SHALLOW_DIMS.index(dims) + 1
    for l in range(H.n_levels):
        lv = H.level(l)
        assert G.level_sizes(l) == {q: lv[q] for q in ("n_fine", "n_fine_faces", "n_coarse", "n_coarse_faces")}
    psi = _dev(np.zeros(case.n_cells))
    perf = G.solve(mat, psi, _dev(case.source), **args)
    _check(perf, _host(psi), ref_psi, ref, f"shallow {dims} {SHALLOW_CONTROLS[k]} sym={sym}")
    assert ref["converged"] and ref["nIterations"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("sym", SYM)
def test_engine_gamg_without_coarse_levels_is_an_error(pkg, orc, sym):
    """GAMGSolver.C:175-190: a mesh that agglomerates to no level at all is a FatalError naming the missing coarse levels"""
    import torch
    eng = pkg.engine
    case = pkg.synthetic.box_case(3, 2, 2, symmetric=sym)
    ctx = eng.Context(0, torch.cuda.current_stream().cuda_stream)
    addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
    with pytest.raises(eng.MiError, match="No coarse levels created"):
        eng.Gamg(addr, orc.box_face_weights(case), 50)


COUPLED_CONTROLS = [ROWS[r] for r in mg.GAMG_COUPLED_ROWS] + [dict(directSolveCoarsest=False, nPreSweeps=1)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cyclic", "processor_to_self"])
@pytest.mark.parametrize("sym", SYM)
@pytest.mark.parametrize("k", range(len(COUPLED_CONTROLS)))
def test_engine_gamg_coupled_patches_control_rows(pkg, orc, mode, sym, k):
    """Rows S1, S4, C1, S9 and the iterative coarsest solve after pre-smoothing on the periodic box: local cyclic patches, and the same
    box posed with processor patches to this rank itself on a 1-rank communicator (attached matrix and hierarchy: per-level halo
    exchange, all-reduced scaling factors, the global coarsest system).  One process."""
    case, w, H, nc, _ = _oracle(pkg, orc, "coupled", sym)
    args = mg.gamg_args(COUPLED_CONTROLS[k])
    ref_psi, ref = _ref(pkg, orc, "coupled", sym, args)
    ctx, addr, mat, G, comm = _engine(pkg, case, w, nc, mode)
    assert G.n_levels == H.n_levels == 7
    for l in range(G.n_levels):
        o, e = H.level(0, l), G.level_sizes(l)
        assert (o["n_coarse"], o["n_coarse_faces"]) == (e["n_coarse"], e["n_coarse_faces"])
    psi = _dev(np.zeros(case.n_cells))
    perf = G.solve(mat, psi, _dev(case.source), **args)
    _check(perf, _host(psi), ref_psi, ref, f"coupled {mode} {COUPLED_CONTROLS[k]} sym={sym}")


@pytest.mark.gpu
def test_one_hierarchy_follows_changing_controls(pkg, orc):
    """One hierarchy, one matrix, solves with changing controls: the cached cycle graph is keyed on the controls that shape a cycle, so
    every solve is its own controls' solve, and a return to the defaults gives the first solve's bits.  tolerance 1e-10: every solve
    has at least three cycles, so a captured cycle is replayed each time."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", True)
    ctx, addr, mat, G, _c = _engine(pkg, case, w, nc)
    b = _dev(case.source)
    got = []
    for k, rid in enumerate([None, "S1", None, "S8", "X2", None]):
        args = mg.gamg_args(dict(ROWS[rid] if rid else {}, tolerance=1e-10))
        ref_psi, ref = _ref(pkg, orc, "F", True, args)
        psi = _dev(np.zeros(case.n_cells))
        perf = G.solve(mat, psi, b, **args)
        x = _host(psi)
        _check(perf, x, ref_psi, ref, f"solve {k} ({rid or 'default'})")
        assert perf["nIterations"] >= 3
        got.append((perf["history"], x))
    for k in (2, 5):
        assert np.array_equal(got[k][0], got[0][0]) and np.array_equal(got[k][1], got[0][1]), k


@pytest.mark.gpu
def test_one_hierarchy_follows_two_matrices(pkg, orc):
    """Two matrices on one addressing solved alternately through one hierarchy: level matrices and the cached cycle belong to the
    matrix of the solve at hand; each solve matches its own oracle hierarchy and the repeats give the same bits."""
    case, w, H, nc, _ = _oracle(pkg, orc, "F", True)
    case2 = copy.copy(case); case2.diag = case.diag * 1.07
    H2 = orc.GamgHierarchy(case2, w, nc)
    ctx, addr, m1, G, _c = _engine(pkg, case, w, nc)
    m2 = _matrix(pkg, addr, case2)
    args = mg.gamg_args(dict(tolerance=1e-10))
    refs = [H.solve(np.zeros(case.n_cells), case.source, **args), H2.solve(np.zeros(case.n_cells), case.source, **args)]
    assert not np.array_equal(refs[0][1]["history"], refs[1][1]["history"])
    b = _dev(case.source)
    got = []
    for k, (m, r) in enumerate([(m1, 0), (m2, 1), (m1, 0), (m2, 1)]):
        psi = _dev(np.zeros(case.n_cells))
        perf = G.solve(m, psi, b, **args)
        x = _host(psi)
        _check(perf, x, refs[r][0], refs[r][1], f"solve {k} (matrix {r + 1})")
        assert perf["nIterations"] >= 3
        got.append((perf["history"], x))
    for k in (2, 3):
        assert np.array_equal(got[k][0], got[k - 2][0]) and np.array_equal(got[k][1], got[k - 2][1]), k
