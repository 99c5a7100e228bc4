"""GPU (-m gpu): the kernel forms behind the same-bits switches of csrc/switches.hpp that no default run reaches -- forced
workgroup sizes of the tile kernels (MI_AMUL_BS), the staging flags (MI_TILE_FLAGS), the persistent tile walk (MI_TILE_PERSIST),
the caller-order operators without the folded permutation (MI_FUSE_PERM=0), the layout caps (MI_TILE_SLOTS, MI_SMALL_TILES) and
the hierarchy forms (MI_GAMG_PIPELINE, MI_GAMG_ALWAYS_AGGLOMERATE, MI_GAMG_INHERIT_TILES).  Every form against the oracle, bit for
bit where the default form is, and against the default form where the switch promises the same bits.

A switch acts when its row of the table says (CTX: mi_ctx_create, ADDR: the addressing, HIER: the hierarchy), so every run here
sets its variables first and then creates a context of its own.  The oracle's results are computed once per case and shared."""
import numpy as np
import pytest
import torch

from conftest import random_graph_case
from test_gpu_fuzz import cyclic_pair, dev, host

pytestmark = pytest.mark.gpu

SWITCHES = ("MI_AMUL_BS", "MI_TILE_FLAGS", "MI_TILE_PERSIST", "MI_FUSE_PERM", "MI_TILE_SLOTS", "MI_SMALL_TILES", "MI_TILE_CELLS", "MI_ENTRY16",
            "MI_GAMG_PIPELINE", "MI_GAMG_ALWAYS_AGGLOMERATE", "MI_GAMG_INHERIT_TILES", "MI_GAMG_INVERT_OVERLAP", "MI_PCG_PERSIST", "MI_DPCG_FUSED")


def _env(monkeypatch, **kw):
    """exactly these switches of SWITCHES set, the others unset"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in kw.items():
        assert name in SWITCHES
        monkeypatch.setenv(name, str(v))


def _ctx(eng):
    return eng.Context(0, torch.cuda.current_stream().cuda_stream)


# ---- cases and their oracle results (computed once) -----------------------------------------------------------------------------
_CASES = {}


def _case(pkg, orc, key):
    """key: ("box", nx, ny, nz, sym) or ("graph", seed, n, extra, sym, pair divisor) -> dict(case, patches, S, x, ref)"""
    if key in _CASES:
        return _CASES[key]
    syn = pkg.synthetic
    if key[0] == "box":
        _, nx, ny, nz, sym = key
        case, patches, seed = syn.box_case(nx, ny, nz, symmetric=sym), ([], []), nx + ny + nz
    else:
        _, seed, n, extra, sym, div = key
        case, a, b = cyclic_pair(pkg, random_graph_case(pkg, n, extra=extra, seed=seed, symmetric=sym), seed, sym, div)
        patches = ([a, b], [b, a])
    n = case.n_cells
    S = orc.System([case])
    x = syn.splitmix_uniform(seed + 7, n) - 0.5
    ref = dict(amul=S.amul(x), tmul=S.tmul(x), sumA=S.sumA(), residual=S.residual(x, case.source), H=S.H(x), H1=S.H1(), faceH=S.faceH(x),
               ainv=S.precondition("AINV", x), ainvT=S.precondition("AINV", x, transpose=True), diagonal=S.precondition("diagonal", x),
               jacobi1=S.jacobi_smooth(x, case.source, 1), jacobi3=S.jacobi_smooth(x, case.source, 3))
    _, pref = S.pcg(x.copy(), case.source, "diagonal", tolerance=0.0, maxIter=1) if sym else S.pbicg(x.copy(), case.source, "diagonal", tolerance=0.0, maxIter=1)
    ref["normFactor"] = pref["normFactor"]
    _CASES[key] = dict(case=case, patches=patches, S=S, x=x, ref=ref, sym=sym, w=0.5 + syn.splitmix_uniform(seed + 5, case.n_faces))
    return _CASES[key]


def _krylov_ref(C):
    if "krylov" not in C:
        case, n = C["case"], C["case"].n_cells
        C["krylov"] = (C["S"].pcg(np.zeros(n), case.source, "AINV", tolerance=1e-10, maxIter=40) if C["sym"]
                       else C["S"].pbicgstab(np.zeros(n), case.source, "AINV", tolerance=1e-10, maxIter=25))
    return C["krylov"]


def _gamg_ref(orc, C, **kw):
    """the oracle's hierarchy and solve (tolerance 1e-9, 40 cycles at most) of a case, once per set of controls"""
    k = ("gamg",) + tuple(sorted(kw.items()))
    if k not in C:
        case = C["case"]
        H = orc.GamgSysHierarchy(C["S"], [C["w"]], 8, merge_levels=1)
        psi, perf = H.solve(np.zeros(case.n_cells), case.source, tolerance=1e-9, maxIter=40, **kw)
        C[k] = (H, psi, perf)
    return C[k]


def _bind(eng, ctx, C):
    case, (fcs, nbrs) = C["case"], C["patches"]
    addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, fcs, nbrs)
    mat = eng.Matrix(addr)
    mat.set_coeffs(dev(case.diag), dev(case.upper), None if C["sym"] else dev(case.lower))
    for p, itf in enumerate(case.interfaces):
        mat.set_interface_coeffs(p, dev(itf.bou_coeffs), None if C["sym"] else dev(itf.int_coeffs))
    return addr, mat


def _operators(mat, C, which=None):
    """the operator set of tests/test_gpu_fuzz.py as numpy arrays (name -> result), in the caller's order"""
    case, x = C["case"], C["x"]
    n = case.n_cells
    xd, bd = dev(x), dev(case.source)
    new = lambda m=n: torch.empty(m, dtype=torch.float64, device="cuda:0")
    got = {}
    out = new(); mat.amul(xd, out); got["amul"] = host(out)
    out = new(); mat.tmul(xd, out); got["tmul"] = host(out)
    out = new(); mat.sumA(out); got["sumA"] = host(out)
    out = new(); mat.residual(xd, bd, out); got["residual"] = host(out)
    out = new(); mat.H(xd, out); got["H"] = host(out)
    out = new(); mat.H1(out); got["H1"] = host(out)
    out = new(); mat.precondition("AINV", xd, out); got["ainv"] = host(out)
    out = new(); mat.precondition("diagonal", xd, out); got["diagonal"] = host(out)
    if which == "caller":          # the operators with a caller-order form (MI_FUSE_PERM)
        return got
    out = new(case.n_faces); mat.faceH(xd, out); got["faceH"] = host(out)
    out = new(); mat.precondition("AINV", xd, out, transpose=True); got["ainvT"] = host(out)
    for sweeps in (1, 3):
        psi = dev(x.copy()); mat.jacobi_smooth(psi, bd, sweeps); got[f"jacobi{sweeps}"] = host(psi)
    got["normFactor"] = mat.norm_factor(xd, bd, dev(C["ref"]["amul"]))
    return got


def _check_operators(got, ref):
    """bit for bit against the oracle (the normalisation factor, a sum, within its bar)"""
    for name, v in got.items():
        if name == "normFactor":
            assert abs(v - ref[name]) <= 1e-12 * ref[name]
        else:
            assert np.array_equal(v, ref[name]), name


def _krylov(mat, C):
    """a short AINV-PCG (symmetric) / AINV-PBiCGStab (asymmetric) from zero: (perf, psi)"""
    case = C["case"]
    psi = torch.zeros(case.n_cells, dtype=torch.float64, device="cuda:0")
    if C["sym"]:
        perf = mat.pcg(psi, dev(case.source), "AINV", tolerance=1e-10, maxIter=40)
    else:
        perf = mat.pbicgstab(psi, dev(case.source), "AINV", tolerance=1e-10, maxIter=25)
    return perf, host(psi)


def _check_krylov(perf, psi, C):
    """the bar of the fuzz sweep: equal iteration counts, history within 1e-9 of the initial residual, psi within 1e-8"""
    ref_psi, ref = _krylov_ref(C)
    assert perf["nIterations"] == ref["nIterations"]
    h, hr = perf["history"], ref["history"]
    assert h.shape == hr.shape and np.max(np.abs(h - hr)) <= 1e-9 * hr[0]
    assert np.max(np.abs(psi - ref_psi)) <= 1e-8 * np.max(np.abs(ref_psi))


def _gamg(eng, addr, mat, C, solves=1, **kw):
    """hierarchy + `solves` solves from zero: (Gamg, [(perf, psi)])"""
    case = C["case"]
    G = eng.Gamg(addr, C["w"], 8, merge_levels=1)
    runs = []
    for _ in range(solves):
        psi = torch.zeros(case.n_cells, dtype=torch.float64, device="cuda:0")
        perf = G.solve(mat, psi, dev(case.source), tolerance=1e-9, maxIter=40, **kw)
        runs.append((perf, host(psi)))
    return G, runs


def _check_gamg(orc, G, runs, C, **kw):
    """the bar of test_random_coupled_matrices_gamg: the oracle's levels, its iteration count, history within 1e-9, psi within 1e-8"""
    H, ref_psi, ref = _gamg_ref(orc, C, **kw)
    assert G.n_levels == H.n_levels
    for l in range(G.n_levels):
        o, e = H.level(0, l), G.level_sizes(l)
        assert (o["n_coarse"], o["n_coarse_faces"]) == (e["n_coarse"], e["n_coarse_faces"])
    for perf, psi in runs:
        assert perf["nIterations"] == ref["nIterations"] and perf["converged"] == ref["converged"]
        h, hr = perf["history"], ref["history"]
        assert h.shape == hr.shape and np.max(np.abs(h - hr)) <= 1e-9 * hr[0]
        assert np.max(np.abs(psi - ref_psi)) <= 1e-8 * np.max(np.abs(ref_psi))


def _same_runs(a, b):
    """two lists of (perf, psi): the same bits"""
    assert len(a) == len(b)
    for (pa, xa), (pb, xb) in zip(a, b):
        assert pa["nIterations"] == pb["nIterations"] and pa["converged"] == pb["converged"]
        assert np.array_equal(pa["history"], pb["history"]) and np.array_equal(xa, xb)


def _permutes(addr):
    return not np.array_equal(addr.cell_perm(), np.arange(addr.n_cells))


# ---- A1: forced workgroup sizes -------------------------------------------------------------------------------------------------
# shape -> (case key without the symmetry, MI_TILE_CELLS, what the layout must look like for the shape to mean what it says)
BS_SHAPES = {
    "box10_one_tile_16_slices": (("box", 10, 10, 10), 1024, lambda st: st["tiles"] == 1 and st["max_cells"] == 1000),   # the last slice: 40 live rows
    "box13x11x9_cut_faces": (("box", 13, 11, 9), 1024, lambda st: st["tiles"] == 3 and st["halo"] > 0),
    "graph257_tile64": (("graph", 2, 257, 2.0), 64, lambda st: st["tiles"] > 4 and st["max_cells"] <= 64),
    "graph40_one_slice_tiles": (("graph", 1, 40, 1.0), 8, lambda st: st["tiles"] >= 5 and st["max_cells"] <= 8),
}


def _key(base, sym):
    return base + (sym,) if base[0] == "box" else base + (sym, 15)


@pytest.mark.parametrize("entry16", [0, 1])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("bs", [256, 512, 1024])
@pytest.mark.parametrize("shape", sorted(BS_SHAPES))
def test_forced_block_sizes(pkg, orc, monkeypatch, shape, bs, sym, entry16):
    """MI_AMUL_BS: every tile shape under every workgroup size, not only the one the launch would choose -- 256 threads over a
    16-slice tile (each wave walks four slices with the one-slice-ahead prefetch), 1024 threads over one-slice tiles (15 waves on
    the pad branch), both row-entry formats.  With explicit entries the caller-order operators run without the folded permutation
    (MI_FUSE_PERM=0): tile_kernel_perm picks its size itself, tile_kernel takes the forced one."""
    eng = pkg.engine
    base, tile, looks_right = BS_SHAPES[shape]
    C = _case(pkg, orc, _key(base, sym))
    kw = dict(MI_AMUL_BS=bs, MI_TILE_CELLS=tile, MI_ENTRY16=entry16)
    if not entry16:
        kw["MI_FUSE_PERM"] = 0
    _env(monkeypatch, **kw)
    ctx = _ctx(eng)
    addr, mat = _bind(eng, ctx, C)
    assert looks_right(addr.stats()), addr.stats()
    assert mat.occupancy()["block_size"] == bs
    if entry16:   # every shape here keeps the compact form: fewer entry words than the explicit form
        _env(monkeypatch, MI_TILE_CELLS=tile)
        explicit, _ = _bind(eng, ctx, C)
        assert addr.stats()["entries"] < explicit.stats()["entries"]
    _check_operators(_operators(mat, C), C["ref"])
    _check_krylov(*_krylov(mat, C), C)


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("bs", [256, 512, 1024])
def test_forced_block_sizes_gamg(pkg, orc, monkeypatch, bs, sym):
    """the V-cycle's fused transfers (tile_kernel_fx) under every workgroup size: 128-cell tiles on every level"""
    eng = pkg.engine
    C = _case(pkg, orc, ("box", 16, 16, 16, sym))
    _env(monkeypatch, MI_AMUL_BS=bs, MI_TILE_CELLS=128)
    ctx = _ctx(eng)
    addr, mat = _bind(eng, ctx, C)
    assert mat.occupancy()["block_size"] == bs and addr.stats()["tiles"] >= 32
    G, runs = _gamg(eng, addr, mat, C)
    _check_gamg(orc, G, runs, C)


# ---- A2: staging flags ----------------------------------------------------------------------------------------------------------
FLAG_SHAPES = {"box13x11x9": (("box", 13, 11, 9), 0), "graph900_tile128": (("graph", 3, 900, 3.0), 128)}


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", sorted(FLAG_SHAPES))
def test_staging_flags_change_no_bit(pkg, orc, monkeypatch, shape, sym):
    """MI_TILE_FLAGS bits 0..3 (non-temporal coefficient staging, entry loads, result stores, diagonal loads) are cache policy
    only: every operator, the residual history and psi of a Krylov run are the bits of the default (1), on a permuting addressing --
    tile_kernel_perm under mi_amul, the engine-order kernels inside the solvers."""
    eng = pkg.engine
    base, tile = FLAG_SHAPES[shape]
    C = _case(pkg, orc, _key(base, sym))
    runs = {}
    for flags in (1, 0, 2, 4, 8, 15):
        _env(monkeypatch, MI_TILE_FLAGS=flags, **(dict(MI_TILE_CELLS=tile) if tile else {}))
        ctx = _ctx(eng)
        addr, mat = _bind(eng, ctx, C)
        assert _permutes(addr) and addr.n_tiles >= 2
        ops = _operators(mat, C)
        _check_operators(ops, C["ref"])
        perf, psi = _krylov(mat, C)
        runs[flags] = (ops, perf, psi)
    _check_krylov(runs[1][1], runs[1][2], C)
    ops1, perf1, psi1 = runs[1]
    for flags, (ops, perf, psi) in runs.items():
        for name in ops1:
            assert np.array_equal(ops[name], ops1[name]), (flags, name)
        assert perf["nIterations"] == perf1["nIterations"] and np.array_equal(perf["history"], perf1["history"]), flags
        assert np.array_equal(psi, psi1), flags


def test_staging_flags_change_no_bit_gamg(pkg, orc, monkeypatch):
    """... and the V-cycle (tile_kernel_fx, the smoothers) with every flag set against the default"""
    eng = pkg.engine
    C = _case(pkg, orc, ("box", 16, 16, 16, True))
    runs = {}
    for flags in (1, 15):
        _env(monkeypatch, MI_TILE_FLAGS=flags, MI_TILE_CELLS=128)
        ctx = _ctx(eng)
        addr, mat = _bind(eng, ctx, C)
        G, runs[flags] = _gamg(eng, addr, mat, C)
        _check_gamg(orc, G, runs[flags], C)
    _same_runs(runs[15], runs[1])


# ---- A3: persistent tile launch -------------------------------------------------------------------------------------------------
def test_persistent_tile_walk(pkg, orc, monkeypatch):
    """MI_TILE_PERSIST=1: as many workgroups as the device holds at once, each walking a run p0..p1 of its XCD's tile positions.
    The walk is taken only with more than two tiles per resident slot, so the case is sized from the device: 64-cell tiles, the
    resident workgroups of the Amul kernel or what the CU's 32 wavefronts allow if that is more, the smallest cubic box with more than 2 * slots + 8 tiles and a tile count that is no multiple of 8 (uneven per-XCD ranges).  The
    context counts the launches that took the walk (mi_ctx_stat 12); MI_FUSE_PERM=0 sends the caller-order operators through the
    same launch (tile_kernel_perm has no persistent form).  Operators bit for bit against the oracle; a 20-iteration
    diagonal PCG (the tile kernels, not the persistent PCG kernel) has the history of the one-workgroup-per-tile launch bit for
    bit: the tile partials land at the same positions."""
    eng, syn = pkg.engine, pkg.synthetic
    STAT_TILE_PERSIST = 12
    _env(monkeypatch, MI_TILE_PERSIST=1, MI_TILE_CELLS=64, MI_PCG_PERSIST=0, MI_FUSE_PERM=0)
    ctx = _ctx(eng)
    probe = syn.box_case(8, 8, 8)
    paddr = eng.Addressing(ctx, probe.n_cells, probe.lower_addr, probe.upper_addr)
    pmat = eng.Matrix(paddr)
    pmat.set_coeffs(dev(probe.diag), dev(probe.upper), None)
    probe_occ = pmat.occupancy()
    # every launch counts its slots from the occupancy of its own kernel: the Amul's (7 where this was written) is no upper bound
    # for the lighter passes (sumA, H1), the 32 wavefronts a CU holds are
    occ = max(probe_occ["blocks_per_cu"], 32 // (probe_occ["block_size"] // 64))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    slots = (occ * ncu // 8) * 8
    assert slots >= 8
    m = int(np.ceil(((2 * slots + 9) * 64) ** (1.0 / 3.0)))
    while True:
        case = syn.box_case(m, m, m)
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
        if addr.n_tiles > 2 * slots + 8 and addr.n_tiles % 8 != 0:
            break
        addr.close()
        m += 1
    print(f"persistent walk: occ {occ}, {ncu} CUs, {slots} slots, box {m}^3 = {case.n_cells} cells in {addr.n_tiles} tiles")
    n = case.n_cells
    x = syn.splitmix_uniform(41, n) - 0.5
    for sym in (True, False):
        cs = case if sym else syn.box_case(m, m, m, symmetric=False)
        S = orc.System([cs])
        ref = dict(amul=S.amul(x), tmul=S.tmul(x), sumA=S.sumA(), residual=S.residual(x, cs.source), H=S.H(x), H1=S.H1(), faceH=S.faceH(x),
                   ainv=S.precondition("AINV", x), ainvT=S.precondition("AINV", x, transpose=True), diagonal=S.precondition("diagonal", x),
                   jacobi1=S.jacobi_smooth(x, cs.source, 1), jacobi3=S.jacobi_smooth(x, cs.source, 3))
        C = dict(case=cs, x=x, ref=ref, sym=sym)
        mat = eng.Matrix(addr)
        mat.set_coeffs(dev(cs.diag), dev(cs.upper), None if sym else dev(cs.lower))
        before = ctx.stat(STAT_TILE_PERSIST)
        got = _operators(mat, C)
        got.pop("normFactor")
        assert ctx.stat(STAT_TILE_PERSIST) >= before + 12, "a tile launch did not take the persistent walk"   # six caller-order operators, AINV twice, four Jacobi sweeps
        _check_operators(got, ref)
        if sym:
            pmat1 = mat
    before = ctx.stat(STAT_TILE_PERSIST)
    psi1 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    perf1 = pmat1.pcg(psi1, dev(case.source), "diagonal", tolerance=0.0, maxIter=20)
    assert ctx.stat(STAT_TILE_PERSIST) > before, "the Amul of the PCG iterations did not take the persistent walk"
    _env(monkeypatch, MI_TILE_PERSIST=0, MI_TILE_CELLS=64, MI_PCG_PERSIST=0, MI_FUSE_PERM=0)
    ctx0 = _ctx(eng)
    addr0 = eng.Addressing(ctx0, n, case.lower_addr, case.upper_addr)
    assert addr0.n_tiles == addr.n_tiles and np.array_equal(addr0.cell_perm(), addr.cell_perm())
    mat0 = eng.Matrix(addr0)
    mat0.set_coeffs(dev(case.diag), dev(case.upper), None)
    psi0 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    perf0 = mat0.pcg(psi0, dev(case.source), "diagonal", tolerance=0.0, maxIter=20)
    assert ctx0.stat(STAT_TILE_PERSIST) == 0
    assert perf1["nIterations"] == perf0["nIterations"] and perf1["history"].shape[0] >= 21    # the initial residual and 20 iterations
    assert np.array_equal(perf1["history"], perf0["history"]) and np.array_equal(host(psi1), host(psi0))


# ---- A4: caller-order forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", sorted(FLAG_SHAPES))
def test_caller_order_operators_without_the_folded_permutation(pkg, orc, monkeypatch, shape, sym):
    """MI_FUSE_PERM=0: gather, engine-order tile pass, scatter instead of tile_kernel_perm and k_mul_perm, on a permuting
    addressing with explicit row entries -- the same bits as the folded form and as the oracle"""
    eng = pkg.engine
    base, tile = FLAG_SHAPES[shape]
    C = _case(pkg, orc, _key(base, sym))
    got = {}
    for fuse in (1, 0):
        _env(monkeypatch, MI_FUSE_PERM=fuse, **(dict(MI_TILE_CELLS=tile) if tile else {}))
        ctx = _ctx(eng)
        addr, mat = _bind(eng, ctx, C)
        assert _permutes(addr) and addr.n_tiles >= 2
        got[fuse] = _operators(mat, C, which="caller")
        _check_operators(got[fuse], C["ref"])
    for name in got[1]:
        assert np.array_equal(got[0][name], got[1][name]), name


# ---- A5: layout caps ------------------------------------------------------------------------------------------------------------
SLOT_CAP_TILES = {64: (113, 10), 257: (28, 40), 1000: (9, 128)}   # MI_TILE_SLOTS -> (tiles, most cells of a tile): tests/test_layout.py


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("cap", sorted(SLOT_CAP_TILES))
def test_slot_cap_cuts_the_tiles(pkg, orc, monkeypatch, cap, sym):
    """MI_TILE_SLOTS below what 128 cells of the ragged graph need (858 slots): at 64 and 257 the slot cap, not the cell cap, ends
    the tiles; 1000 is above it and leaves the nine 128-cell tiles"""
    eng = pkg.engine
    C = _case(pkg, orc, ("graph", 3, 900, 3.0, sym, 15))
    _env(monkeypatch, MI_TILE_SLOTS=cap, MI_TILE_CELLS=128)
    ctx = _ctx(eng)
    addr, mat = _bind(eng, ctx, C)
    st = addr.stats()
    assert st["max_slots"] <= cap + 2
    assert (st["tiles"], st["max_cells"]) == SLOT_CAP_TILES[cap]
    _check_operators(_operators(mat, C), C["ref"])
    _check_krylov(*_krylov(mat, C), C)


def test_slot_cap_below_one_cell_is_refused(pkg, orc, monkeypatch):
    eng = pkg.engine
    C = _case(pkg, orc, ("graph", 3, 900, 3.0, True, 15))
    _env(monkeypatch, MI_TILE_SLOTS=16, MI_TILE_CELLS=128)
    ctx = _ctx(eng)
    with pytest.raises(eng.MiError, match="a single cell has more faces than a tile can hold"):
        _bind(eng, ctx, C)       # refused while the layout is built on the host: nothing was launched


def test_gamg_without_small_coarse_tiles(pkg, orc, monkeypatch):
    """MI_SMALL_TILES=0: the coarse levels keep 1024-cell tiles instead of one tile per CU down to 128 cells"""
    eng = pkg.engine
    C = _case(pkg, orc, ("box", 24, 24, 24, True))
    _env(monkeypatch, MI_SMALL_TILES=0)
    ctx = _ctx(eng)
    addr, mat = _bind(eng, ctx, C)
    G, runs = _gamg(eng, addr, mat, C)
    _check_gamg(orc, G, runs, C)


# ---- A6: hierarchy forms --------------------------------------------------------------------------------------------------------
HIER_SHAPES = {"box20": (("box", 20, 20, 20, True), {}), "graph1200": (("graph", 26, 1200, 2.5, True, 20), dict(nFinestSweeps=3, nPostSweeps=1))}
_DEFAULT_HIER_RUNS = {}


def _hier_runs(pkg, orc, monkeypatch, shape, **env):
    eng = pkg.engine
    key, kw = HIER_SHAPES[shape]
    C = _case(pkg, orc, key)
    _env(monkeypatch, **env)
    ctx = _ctx(eng)
    addr, mat = _bind(eng, ctx, C)
    G, runs = _gamg(eng, addr, mat, C, solves=2, **kw)
    _check_gamg(orc, G, runs, C, **kw)
    return runs


def _default_hier_runs(pkg, orc, monkeypatch, shape):
    if shape not in _DEFAULT_HIER_RUNS:
        _DEFAULT_HIER_RUNS[shape] = _hier_runs(pkg, orc, monkeypatch, shape)
    return _DEFAULT_HIER_RUNS[shape]


@pytest.mark.parametrize("switch,value", [("MI_GAMG_PIPELINE", 0), ("MI_GAMG_ALWAYS_AGGLOMERATE", 1), ("MI_GAMG_INVERT_OVERLAP", 0)])
@pytest.mark.parametrize("shape", sorted(HIER_SHAPES))
def test_hierarchy_forms_same_bits(pkg, orc, monkeypatch, shape, switch, value):
    """level layouts built one after the other instead of on other threads; level matrices agglomerated again at every solve; the
    coarsest level inverted on the solve's own stream instead of beside its prologue (read at every solve): two solves in a row with the bits of the default run's two solves (and the oracle's levels and history within the GAMG bar)"""
    ref = _default_hier_runs(pkg, orc, monkeypatch, shape)
    _same_runs(_hier_runs(pkg, orc, monkeypatch, shape, **{switch: value}), ref)


@pytest.mark.parametrize("shape", sorted(HIER_SHAPES))
def test_hierarchy_with_inherited_tiles(pkg, orc, monkeypatch, shape):
    """MI_GAMG_INHERIT_TILES=1 (it acts on levels of 1024-cell tiles): other tiles, so other sums -- the oracle's levels, its
    iteration count and the GAMG bar"""
    _hier_runs(pkg, orc, monkeypatch, shape, MI_GAMG_INHERIT_TILES=1, MI_TILE_CELLS=1024)


# ---- distributed PCG without its fused iteration --------------------------------------------------------------------------------
def test_attached_pcg_without_the_fused_iteration(pkg, orc, monkeypatch):
    """MI_DPCG_FUSED=0 on the one-rank self-exchange communicator with peer windows: the phase loop (exchange, Amul, all-reduce as
    separate steps) instead of the launches that carry the exchange and the sums inside -- the sums are formed in the same order,
    so the history and psi have the fused iteration's bits, and both are within the bar of the self-exchange sweep of the oracle.
    MI_PCG_PERSIST=0: otherwise the persistent kernel takes the solve before either form is asked."""
    eng, syn = pkg.engine, pkg.synthetic
    case = syn.add_cyclic_y(syn.box_case(18, 12, 10))
    n = case.n_cells
    ref_psi, ref = orc.System([case]).pcg(np.zeros(n), case.source, "diagonal", tolerance=1e-9, maxIter=500)
    runs = {}
    for fused in (1, 0):
        _env(monkeypatch, MI_DPCG_FUSED=fused, MI_PCG_PERSIST=0)
        ctx = _ctx(eng)
        addr = eng.Addressing(ctx, n, case.lower_addr, case.upper_addr, [i.face_cells for i in case.interfaces])   # processor patches to this rank
        mat = eng.Matrix(addr)
        mat.set_coeffs(dev(case.diag), dev(case.upper), None)
        for p, itf in enumerate(case.interfaces):
            mat.set_interface_coeffs(p, dev(itf.bou_coeffs), None)
        comm = eng.Comm(ctx, 1, 0, eng.Comm.unique_id())
        assert comm.peer_auto()
        mat.attach_comm(comm, comm, [0, 0], [1, 0], n_global=n)
        assert mat.peer_halo_status() == (True, 0)
        psi = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        perf = mat.pcg(psi, dev(case.source), "diagonal", tolerance=1e-9, maxIter=500)
        assert ctx.stat(1) == 0 and mat.peer_halo_status() == (True, 0) and comm.peer_status()[0] == 0
        runs[fused] = (perf, host(psi))
        assert perf["nIterations"] == ref["nIterations"]
        assert np.max(np.abs(perf["history"] - ref["history"])) <= 1e-9 * ref["history"][0]
        assert np.max(np.abs(runs[fused][1] - ref_psi)) <= 1e-8 * np.max(np.abs(ref_psi))
        mat.detach_comm(); comm.close()
    _same_runs([runs[0]], [runs[1]])
