"""Shared by the scheme tests that pin the engine to the reference bit for bit: the device helpers, the row-plan shapes, the exact
arithmetic, and the fused-assembly check (mi_fvm_assemble* against the engine's own scheme-by-scheme sequence and against a restatement).

Functions and constants only; `monkeypatch` comes from the calling test.  A new scheme's row-shape test starts from set_row_tables /
set_row_blocks / shaped_addressing, its fused-assembly test from FusedCase (tests/test_backward_ddt.py is the shortest user)."""
from fractions import Fraction

import numpy as np


# ---- device helpers --------------------------------------------------------------------------------------------------------------
def gpu_env(pkg, fill=None):
    """-> eng, ctx, dev (host array -> float64 device tensor), host (device tensor -> array, after a synchronize), E (m -> an output
    tensor: uninitialised, or filled with `fill` where a test asserts that a refused call launched nothing)"""
    import torch
    eng = pkg.engine
    ctx = eng.Context(0, torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    host = lambda t: (torch.cuda.synchronize(), t.cpu().numpy())[1]
    if fill is None:
        E = lambda m: torch.empty(m, dtype=torch.float64, device="cuda:0")
    else:
        E = lambda m: torch.full((m,), fill, dtype=torch.float64, device="cuda:0")
    return eng, ctx, dev, host, E


# ---- row-plan shapes ---------------------------------------------------------------------------------------------------------------
ROW_MODES = ("fixed256", "fixed1024", "tiles", "tiles_unstaged", "fixed_unstaged")
# the forms of the row tables and of the block mapping that the defaults never take: (tables, mode)
OTHER_TABLES = ([("row32", m) for m in ROW_MODES] + [("noxcd", m) for m in ("fixed256", "tiles")])
# (mesh, mode, tables) of the time schemes' fused-assembly tests
SHAPES = ([(name, mode, "default") for name in ("box", "graph") for mode in ROW_MODES[:4]]
          + [("box", "fixed256", "row32"), ("graph", "tiles", "noxcd")])


def set_row_tables(monkeypatch, tables):
    """"default" | "row32" | "noxcd".  Call it BEFORE gpu_env: MI_XCD_ROWS is read by mi_ctx_create, MI_ROW16 when an addressing makes
    its row plans (ensure_caller_tables, at its first caller-order operator).  Set later, the test passes and tests the default."""
    monkeypatch.delenv("MI_ROW16", raising=False); monkeypatch.delenv("MI_XCD_ROWS", raising=False)
    if tables == "row32":       # the 32-bit row tables: also what a block that does not fit 16 bits falls back to
        monkeypatch.setenv("MI_ROW16", "0")
    elif tables == "noxcd":     # blockIdx.x as it comes, in every row pass, face pass and gradient pass
        monkeypatch.setenv("MI_XCD_ROWS", "0")
    else:
        assert tables == "default"


def set_row_blocks(monkeypatch, mode, grad=False):
    """the block shape of a ROW_MODES entry: cells per block under the caller's numbering (MI_ROW_BS; grad: MI_GRAD_BS too, the plan of
    the gradient passes) and, for the *_unstaged modes, a staging capacity no block fits (MI_ROW_CAP=64).  Call it before creating the
    addressing the test runs on: the three are read when that addressing makes its row plans."""
    bs = "1024" if mode == "fixed1024" else "256"
    monkeypatch.setenv("MI_ROW_BS", bs)
    if grad:
        monkeypatch.setenv("MI_GRAD_BS", bs)
    if mode.endswith("unstaged"):
        monkeypatch.setenv("MI_ROW_CAP", "64")


def set_face_grid(monkeypatch, blocks):
    """the most workgroups a face pass or a unique-cell patch pass is launched with (MI_FACE_GRID; None: the default, 8192).  Call it
    BEFORE gpu_env: the switch is read by mi_ctx_create.  A small value makes every such kernel walk its grid-stride or block_chunk loop
    on a small mesh (tests/test_launch_grids.py)"""
    if blocks is None:
        monkeypatch.delenv("MI_FACE_GRID", raising=False)
    else:
        monkeypatch.setenv("MI_FACE_GRID", str(blocks))


def shaped_addressing(eng, ctx, syn, case, mode):
    """-> (case, addr).  tiles*: the case renumbered into the tile order of a probe addressing, under ordered addressing on the probe's
    tile starts (the row passes own the layout's tiles); otherwise the case as it is (fixed ranges of cells)"""
    if mode.startswith("tiles"):
        a0 = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
        case = syn.renumber(case, a0.cell_perm())
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
        assert addr.is_ordered
        return case, addr
    return case, eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)


def shape_case(pkg, name, symmetric=False):
    """"box" / "graph": the two meshes of the shape tests, the smallest with several tiles and several 1024-cell blocks with cut faces on
    both sides; every other name: a mesh of DEGENERATE_MESHES"""
    from conftest import random_graph_case
    if name == "box":
        return pkg.synthetic.box_case(31, 23, 19, symmetric=symmetric)
    if name == "graph":
        return random_graph_case(pkg, 9000, extra=3.0, seed=5, symmetric=symmetric)
    return degenerate_case(pkg, name, symmetric=symmetric)


# ---- the degenerate meshes (tests/test_degenerate_meshes.py) ---------------------------------------------------------------------------
# legal lduAddressing a polyhedral or agglomerated mesh brings and a box never does: cells without faces, a block of cells without faces,
# rows of thousands of faces, cell counts around a block boundary, blocks at and past the limits of the 16-bit row tables
EDGE_SIZES = (255, 256, 257, 1023, 1024, 1025)
DEGENERATE_MESHES = (("one_cell", "no_faces", "isolated", "hub_first", "hub_last") + tuple(f"edge_{n}" for n in EDGE_SIZES)
                     + ("dense_fits", "dense_fallback", "own_32767", "own_32768"))
ROW16_LIMITS = (32768, 32768, 65536)        # own faces, cut faces, neighbour-list entries of one block (ensure_caller_tables)
HUB_SPOKES = 3000                           # the tiling takes at most 4 094 faces on one cell
ISOLATED_N, ISOLATED_EMPTY = 1500, (512, 768)


def case_from_pairs(pkg, n, lo, up, seed, symmetric=False):
    """an LduCase on the faces (lo[i], up[i]), lo < up, already sorted by (lo, up) without duplicates; coefficients as
    conftest.random_graph_case forms them: upper = -(0.2 + u), an independent lower, a dominant diag (0.05 + u on a cell without faces)"""
    syn = pkg.synthetic
    lo, up = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(up, dtype=np.int32)
    nf = lo.shape[0]
    assert up.shape[0] == nf and (nf == 0 or (lo.min() >= 0 and up.max() < n and np.all(lo < up)))
    key = lo.astype(np.int64) * n + up
    assert np.all(key[1:] > key[:-1]), "faces sorted by (lower, upper), no duplicate pair"
    c = syn.splitmix_uniform(seed + 1, 2 * nf)
    upper = -(0.2 + c[:nf])
    lower = None if symmetric else -(0.2 + c[nf:])
    diag = np.zeros(n)
    np.subtract.at(diag, lo, upper if symmetric else lower)
    np.subtract.at(diag, up, upper)
    diag += 0.05 + syn.splitmix_uniform(seed + 2, n)
    return syn.LduCase(n, lo, up, diag, upper, lower, syn.splitmix_uniform(seed + 3, n) - 0.5)


def isolated_labels(pkg):
    """the kept labels of "isolated", sorted: all of 0..1499 but the block 512..767 and 37 single cells -- the first and the last cell, the
    cells on both sides of the 256- and 1024-cell block boundaries, and 31 seeded ones"""
    a, b = ISOLATED_EMPTY
    drop = {0, 255, 256, 1023, 1024, ISOLATED_N - 1}
    for x in (pkg.synthetic.splitmix_uniform(91, 400) * ISOLATED_N).astype(np.int64).tolist():
        if len(drop) < 37 and not a <= x < b:
            drop.add(x)
    assert len(drop) == 37
    keep = np.ones(ISOLATED_N, bool)
    keep[a:b] = False
    keep[sorted(drop)] = False
    return np.nonzero(keep)[0]


def hub_pairs(first):
    """hub_first: cell 0 joins every cell 1..3000, plus the chain i-(i+1) for i >= 1; hub_last: every cell 0..2999 joins cell 3000, plus
    the chain -- 5 999 faces each"""
    m = HUB_SPOKES
    if first:
        lo = np.concatenate([np.zeros(m, np.int64), np.arange(1, m)])
        up = np.concatenate([np.arange(1, m + 1), np.arange(2, m + 1)])
    else:
        lo = np.concatenate([np.arange(m), np.arange(m - 1)])
        up = np.concatenate([np.full(m, m), np.arange(1, m)])
    order = np.lexsort((up, lo))
    return m + 1, lo[order], up[order]


def own_pairs(drop_last):
    """cells 0..1023 own 32 faces each into the cells 1024..3071, cell i joining 1024 + (32 i + j) mod 2048 for j < 32: 32 768 own faces in
    the first 1024-cell block, exactly the limit of the 16-bit tables; drop_last: one fewer"""
    i, j = np.repeat(np.arange(1024), 32), np.tile(np.arange(32), 1024)
    lo, up = i, 1024 + (32 * i + j) % 2048
    if drop_last:
        lo, up = lo[:-1], up[:-1]
    return 3072, lo, up


def degenerate_case(pkg, name, symmetric=False):
    from conftest import random_graph_case
    none = np.zeros(0, np.int32)
    if name == "one_cell":
        return case_from_pairs(pkg, 1, none, none, 21, symmetric)
    if name == "no_faces":
        return case_from_pairs(pkg, 300, none, none, 23, symmetric)
    if name == "isolated":
        g = random_graph_case(pkg, ISOLATED_N - 37 - (ISOLATED_EMPTY[1] - ISOLATED_EMPTY[0]), extra=2.5, seed=25)
        labels = isolated_labels(pkg)                        # sorted: the map is monotone, so the faces stay in upper-triangular order
        return case_from_pairs(pkg, ISOLATED_N, labels[g.lower_addr], labels[g.upper_addr], 27, symmetric)
    if name in ("hub_first", "hub_last"):
        return case_from_pairs(pkg, *hub_pairs(name == "hub_first"), 29, symmetric)
    if name.startswith("edge_"):
        return random_graph_case(pkg, int(name[5:]), extra=2.5, symmetric=symmetric)
    if name == "dense_fits":
        return random_graph_case(pkg, 2048, extra=12, symmetric=symmetric)
    if name == "dense_fallback":
        return random_graph_case(pkg, 2048, extra=40, symmetric=symmetric)
    if name in ("own_32767", "own_32768"):
        return case_from_pairs(pkg, *own_pairs(name == "own_32767"), 31, symmetric)
    raise KeyError(name)


def block_counts(case, bs):
    """host only -> (own faces, cut faces, neighbour-list entries) per block of consecutive cells, the three counts ensure_caller_tables
    holds against ROW16_LIMITS; a cut face: a neighbour-side face owned by a cell of an earlier block.  bs: cells per block (256, 1024), or
    the blocks' first cells followed by n_cells (the layout's tiles)"""
    n = case.n_cells
    starts = np.append(np.arange(0, n, bs), n) if np.isscalar(bs) else np.asarray(bs, dtype=np.int64)
    nb = len(starts) - 1
    bo = np.searchsorted(starts, case.lower_addr, side="right") - 1
    bn = np.searchsorted(starts, case.upper_addr, side="right") - 1
    return np.bincount(bo, minlength=nb), np.bincount(bn[bo != bn], minlength=nb), np.bincount(bn, minlength=nb)


def fits_row16(case, bs):
    """every block below the three limits: the addressing keeps the 16-bit row tables"""
    return all(int(c.max()) < lim for c, lim in zip(block_counts(case, bs), ROW16_LIMITS))


def row_blocks(addr, case, bs):
    """the cell ranges the row passes of this addressing own (ensure_caller_tables): the layout's tiles where the numbering is
    tile-contiguous and no tile has more than 1024 cells, fixed ranges of bs cells otherwise -> the blocks' first cells followed by n_cells"""
    if addr.is_ordered:
        ts = np.asarray(addr.tile_starts(), dtype=np.int64)
        if int(np.diff(ts).max()) <= 1024:
            return ts
    return np.append(np.arange(0, case.n_cells, bs), case.n_cells)


def row_passes_bit_exact(eng, orc, syn, case, addr, dev, host, E):
    """The row passes (row face ops, fvm::laplacian, fvm::div, surfaceIntegrate, Gauss grad, the interpolated flux with its surfaceIntegrate,
    fvc::div) on one mesh under one addressing against the oracle, bit for bit, and face_interpolate; where the mesh has faces, the
    refusals of an output aliasing an input.  -> the engine's results by name, for a caller that compares two runs array by array"""
    import pytest
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    asm = eng.Assembly(addr)
    got = {}
    lower = case.upper if case.lower is None else case.lower
    for kind in (0, 1, 2):
        start = syn.splitmix_uniform(kind, n)
        io = dev(start)
        asm.row_face_op(kind, dev(lower), dev(case.upper), io)
        got[f"row_face_op{kind}/asymmetric"] = host(io)
        assert np.array_equal(host(io), orc.row_face_op(kind, n, lo, up, lower, case.upper, start)), kind
        io = dev(start)
        asm.row_face_op(kind, None, dev(case.upper), io)
        got[f"row_face_op{kind}/symmetric"] = host(io)
        assert np.array_equal(host(io), orc.row_face_op(kind, n, lo, up, None, case.upper, start)), kind
    delta, gam = 1.0 + syn.splitmix_uniform(7, nf), 0.5 + syn.splitmix_uniform(8, nf)
    uo, do = E(nf), E(n)
    asm.fvm_laplacian(dev(delta), dev(gam), uo, do)
    ru, rd = orc.fvm_laplacian(n, lo, up, delta, gam)
    got["laplacian/upper"], got["laplacian/diag"] = host(uo), host(do)
    assert np.array_equal(host(uo), ru) and np.array_equal(host(do), rd)
    w, phi = syn.splitmix_uniform(9, nf), syn.splitmix_uniform(10, nf) - 0.5
    lo_o, uo, do = E(nf), E(nf), E(n)
    asm.fvm_div(dev(w), dev(phi), lo_o, uo, do)
    rl, ru, rd = orc.fvm_div(n, lo, up, w, phi)
    got["div/lower"], got["div/upper"], got["div/diag"] = host(lo_o), host(uo), host(do)
    assert np.array_equal(host(lo_o), rl) and np.array_equal(host(uo), ru) and np.array_equal(host(do), rd)
    vol = 0.5 + syn.splitmix_uniform(11, n)
    out = E(n)
    asm.surface_integrate(dev(phi), None, out); assert np.array_equal(host(out), orc.surface_integrate(n, lo, up, phi))
    got["surface_integrate"] = host(out)
    asm.surface_integrate(dev(phi), dev(vol), out); assert np.array_equal(host(out), orc.surface_integrate(n, lo, up, phi, vol))
    got["surface_integrate/vol"] = host(out)
    Sf = [syn.splitmix_uniform(20 + k, nf) - 0.5 for k in range(3)]
    g = [E(n) for _ in range(3)]
    asm.gauss_grad([dev(x) for x in Sf], dev(phi), dev(vol), g)
    for k, (a, b) in enumerate(zip(g, orc.gauss_grad(n, lo, up, Sf, phi, vol))):
        got[f"gauss_grad/{k}"] = host(a)
        assert np.array_equal(host(a), b)
    # round 5: the flux of an interpolated (scaled) cell vector and its surfaceIntegrate in one row pass (pEqn.H:49-71)
    lam = syn.splitmix_uniform(30, nf)
    V = [syn.splitmix_uniform(31 + k, n) - 0.5 for k in range(3)]
    rho, aA, aB = 0.8 + syn.splitmix_uniform(35, n), syn.splitmix_uniform(36, nf) - 0.5, syn.splitmix_uniform(37, nf)
    po, dv = E(nf), E(n)
    for kw in (dict(), dict(scale=rho), dict(scale=rho, add_a=aA, add_b=aB, vol=vol), dict(add_a=aA)):
        asm.flux_div(dev(lam), [dev(x) for x in Sf], [dev(x) for x in V], po, dv, cell_scale=dev(kw["scale"]) if "scale" in kw else None,
                     add_a=dev(kw["add_a"]) if "add_a" in kw else None, add_b=dev(kw["add_b"]) if "add_b" in kw else None,
                     vol=dev(kw["vol"]) if "vol" in kw else None)
        rp, rd = orc.flux_div(n, lo, up, lam, Sf, V, **kw)
        got["flux_div/" + "+".join(sorted(kw)) + "/phi"], got["flux_div/" + "+".join(sorted(kw)) + "/div"] = host(po), host(dv)
        assert np.array_equal(host(po), rp) and np.array_equal(host(dv), rd), sorted(kw)
    # fvc::interpolate and fvc::div(faceFlux, vf) (gaussConvectionScheme::fvcDiv): upwind and given weights
    cellf = syn.splitmix_uniform(12, n)
    sf = E(nf)
    asm.face_interpolate(dev(w), dev(cellf), sf)
    got["face_interpolate"] = host(sf)
    assert np.array_equal(host(sf), orc.face_interpolate(lo, up, w, cellf))
    Kf, dv = E(nf), E(n)
    for wts in (None, w):
        asm.fvc_div(dev(phi), None if wts is None else dev(wts), dev(cellf), dev(vol), Kf, dv)
        ref_f = phi * orc.face_interpolate(lo, up, orc.upwind_weights(phi) if wts is None else wts, cellf)
        tag = "fvc_div/" + ("upwind" if wts is None else "weights")
        got[tag + "/face"], got[tag + "/div"] = host(Kf), host(dv)
        assert np.array_equal(host(Kf), ref_f) and np.array_equal(host(dv), orc.surface_integrate(n, lo, up, ref_f, vol)), tag
    if nf == 0:
        return got
    # the fused passes recompute cut faces from their inputs: an output aliasing an input is refused
    d = dev(delta)
    with pytest.raises(eng.MiError):
        asm.fvm_laplacian(d, dev(gam), d, do)
    l = dev(lam)
    with pytest.raises(eng.MiError):
        asm.flux_div(l, [dev(x) for x in Sf], [dev(x) for x in V], l, dv)
    return got


# ---- exact arithmetic --------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, signed zeros included"""
    return np.array_equal(bits(a), bits(b))


def fma(a, b, c):
    """one rounding: exact rational arithmetic, then float() rounds to nearest even"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma_each(a, b, c):
    """element-wise fma with ONE rounding (non-finite operands: a*b + c)"""
    out = np.empty(a.shape[0])
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        out[i] = float(Fraction(x) * Fraction(y) + Fraction(z)) if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) else x * y + z
    return out


def dot_contracted(ax, ay, az, bx, by, bz):
    """Vector & Vector as the compiled reference contracts it and as every face pass of the engine does: fma(az, bz, fma(ax, bx, ay*by)).
    Pinned by the oracle's flux_face against the compiled reference (tests/test_oracle.py)"""
    return fma(az, bz, fma(ax, bx, ay * by))


def rmax(a, b):
    """doubleScalar max (label.H:285-298 MAXMIN): (s1 > s2) ? s1 : s2 -- max(-0.0, 0.0) is +0.0"""
    return a if a > b else b


def rmin(a, b):
    """(s1 < s2) ? s1 : s2"""
    return a if a < b else b


def box_centres(dims):
    """cell centres of the uniform lexicographic box"""
    nx, ny, nz = dims
    h = 1.0 / nx
    c = np.arange(nx * ny * nz)
    return [(c % nx + 0.5) * h, ((c // nx) % ny + 0.5) * h, (c // (nx * ny) + 0.5) * h]


def signed_flux(u, neg_zero=True):
    """a face flux of both signs from uniform numbers, with exact zeros -- of both signs unless neg_zero is False"""
    f = u - 0.45
    f[::7] = 0.0
    if neg_zero:
        f[3::11] = -0.0
    return f


# ---- restatements shared by a scheme's own test and tests/test_streaming_passes.py -------------------------------------------------
# the sizes of the streaming (double2) kernels: 1 and 3 an unpaired element, 1027 many one-pair blocks and a tail, 1 050 625 the first
# size at which a thread walks more than one pair (chunk 1028 > 2*256) with an odd last chunk, 5 243 907 five to six pairs per thread
# (the unroll-by-4 body and its remainder)
STREAM_SIZES = (1, 2, 3, 1027, 1050625, 5243907)


def lust_weights(cdw, flux):
    """0.75*w_linear + 0.25*pos(faceFlux): three field operations (numpy evaluates them one by one, no contraction)"""
    return 0.75 * cdw + 0.25 * (flux >= 0).astype(np.float64)


def co_face(dc, phi, mag_sf, dt, max_co, rho_f=None):
    """CofrDeltaT (CoEulerDdtScheme.C:125-167): max(a, b) = (a > b) ? a : b"""
    den = mag_sf if rho_f is None else rho_f * mag_sf
    co = (dc * (np.abs(phi) / den)) * dt
    q = co / max_co
    return np.where(q > 1.0, q, 1.0) / dt


# ---- the fused-assembly check -------------------------------------------------------------------------------------------------------
# n_rhs, density, convection weights (None: upwind; "w": given; False: no convection), Sp and the two explicit terms, the correction
VARIANTS = [
    dict(tag="momentum", n_rhs=3, field=True, div=None, extras=True, corr=False),
    dict(tag="scalar", n_rhs=1, field=False, div="w", extras=False, corr=False),
    dict(tag="symmetric", n_rhs=1, field=False, div=False, extras=True, corr=False),
    dict(tag="corrected", n_rhs=3, field=True, div=None, extras=True, corr=True),
    dict(tag="corrected_scalar", n_rhs=1, field=False, div=None, extras=False, corr=True),
]


def fused_inputs(pkg, n, nf):
    u = pkg.synthetic.splitmix_uniform
    return dict(flux=signed_flux(u(110, nf), neg_zero=False), w=0.3 + 0.4 * u(140, nf), vol=0.5 + u(111, n), delta=1.0 + u(107, nf),
                gamma=0.5 + u(108, nf), rho=0.8 + u(135, n), rho0=0.7 + u(136, n), rho00=0.6 + u(137, n), sp=u(153, n),
                psi0=[u(131 + k, n) - 0.5 for k in range(3)], psi00=[u(171 + k, n) - 0.5 for k in range(3)],
                su=[u(154 + k, n) - 0.5 for k in range(3)], su2=[u(158 + k, n) - 0.5 for k in range(3)],
                C=[u(144 + k, n) for k in range(3)], cf=[u(147 + k, nf) for k in range(3)],
                grad=[[4.0 * (u(200 + 3 * r + k, n) - 0.5) for k in range(3)] for r in range(3)])


def euler_ddt_call(A, r_delta_t, vol, psi_old, rho_value=None, rho=None, rho_old=None):
    """the ddt_call of unfused_sequence for the Euler scheme: fvm::ddt(rho, vf) with a density field, or with the constant rho_value"""
    if rho is not None:
        return lambda r, dd, ds: A.fvm_ddt_euler_rho(r_delta_t, rho, rho_old, vol, psi_old[r], dd, ds)
    return lambda r, dd, ds: A.fvm_ddt_euler(r_delta_t, rho_value, vol, psi_old[r], dd, ds)


def unfused_sequence(A, E, vol, ddt_call, n_rhs, lap, div=None, sp=None, su=()):
    """The engine's scheme-by-scheme calls for  ddt + [div] - laplacian [- Sp] == [- su + su2], combined with mi_vec_axpby the way
    fvMatrix::operator+ / - combine them (fvMatrix.C:1693-2030) -- what one mi_fvm_assemble* call must equal bit for bit.  div, lap, sp
    and su as Assembly.assemble takes them (device arrays; div["weights"] None: upwind; su: () or the pair [(1.0, su), (-1.0, su2)]);
    ddt_call(r, diag_out, source_out) issues the time scheme's one launch for right-hand side r.  -> dict(lower, upper, diag, src, t):
    t the correction's face fields"""
    n, nf = vol.numel(), lap["delta_coeffs"].numel()
    corr = div.get("correction") if div else None
    cl, cu, cd, lu, ld, dd, ds = E(nf), E(nf), E(n), E(nf), E(n), E(n), [E(n) for _ in range(n_rhs)]
    t = [E(nf) for _ in range(n_rhs)]
    if div:
        flux, wts = div["flux"], div.get("weights")
        if wts is None:
            wts = E(nf); A.upwind_weights(flux, wts)
        A.fvm_div(wts, flux, cl, cu, cd)
        if corr:
            A.linear_upwind_correction(flux, corr["cf"], corr["c"], corr["grad"], t)
    A.fvm_laplacian(lap["delta_coeffs"], lap["gamma_magsf"], lu, ld)
    for r in range(n_rhs):
        ddt_call(r, dd, ds[r])
        if corr:
            ivf = E(n); A.surface_integrate(t[r], vol, ivf); A.submul(vol, ivf, ds[r])
        if su:
            A.fvm_su(vol, su[0][1][r], ds[r])                           # + su: source -= V*su
            p = vol * su[1][1][r]; ds[r].add_(p)                        # == su2: source += V*su2
    if div:
        A.axpby(1.0, cl, -1.0, lu, cl); A.axpby(1.0, cu, -1.0, lu, cu)
        A.axpby(1.0, dd, 1.0, cd, dd)
    else:
        A.axpby(-1.0, lu, 0.0, lu, cu)
    A.axpby(1.0, dd, -1.0, ld, dd)
    if sp is not None:
        p = vol * sp[0]; dd.sub_(p)
    return dict(lower=cl if div else None, upper=cu, diag=dd, src=ds, t=t)


class FusedCase:
    """one (mesh, mode, tables) of SHAPES: the row tables and blocks, the device, the mesh under its addressing, fused_inputs, the
    Assembly, and what every variant shares"""

    def __init__(self, pkg, orc, monkeypatch, name, mode, tables):
        set_row_tables(monkeypatch, tables)
        set_row_blocks(monkeypatch, mode)
        self.orc = orc
        self.eng, self.ctx, self.dev, self.host, self.E = gpu_env(pkg)
        self.case, self.addr = shaped_addressing(self.eng, self.ctx, pkg.synthetic, shape_case(pkg, name), mode)
        self.n, self.nf, self.lo, self.up = self.case.n_cells, self.case.n_faces, self.case.lower_addr, self.case.upper_addr
        self.q = fused_inputs(pkg, self.n, self.nf)
        self.A = self.eng.Assembly(self.addr)
        self.vol, self.flux = self.dev(self.q["vol"]), self.dev(self.q["flux"])
        self.lap = dict(delta_coeffs=self.dev(self.q["delta"]), gamma_magsf=self.dev(self.q["gamma"]))
        self.uL, self.dL = orc.fvm_laplacian(self.n, self.lo, self.up, self.q["delta"], self.q["gamma"])

    def variant(self, v):
        return FusedVariant(self, v)


class FusedVariant:
    """one entry of VARIANTS on a FusedCase: the arguments of Assembly.assemble on the device --
      ddt   vol, psi_old and the density (rho + rho_old, or rho_value); the scheme's test adds r_delta_t and its own key
      rho   the density part of ddt alone, as the keywords of the unfused ddt calls
      div, sp, su, and the case's lap
    -- and psi_old_old / rho_old_old (None without a density field) for the schemes that read them"""

    def __init__(self, case, v):
        q, dev = case.q, case.dev
        self.case, self.v, self.tag, self.R = case, v, v["tag"], v["n_rhs"]
        R = self.R
        self.psi_old = [dev(x) for x in q["psi0"][:R]]
        self.psi_old_old = [dev(x) for x in q["psi00"][:R]]
        if v["field"]:
            self.rho, self.rho_old_old = dict(rho=dev(q["rho"]), rho_old=dev(q["rho0"])), dev(q["rho00"])
        else:
            self.rho, self.rho_old_old = dict(rho_value=1.2), None
        self.ddt = dict(vol=case.vol, psi_old=self.psi_old, **self.rho)
        self.div = None
        if v["div"] is not False:
            self.div = dict(flux=case.flux, weights=dev(q["w"]) if v["div"] == "w" else None)
            if v["corr"]:
                grads = [[dev(x) for x in g] for g in q["grad"][:R]]
                self.div["correction"] = dict(scale=1.0, cf=[dev(x) for x in q["cf"]], c=[dev(x) for x in q["C"]], grad=grads)
        self.sp = (dev(q["sp"]), -1.0) if v["extras"] else None
        self.su = [(1.0, [dev(x) for x in q["su"][:R]]), (-1.0, [dev(x) for x in q["su2"][:R]])] if v["extras"] else []

    def fused(self, ddt_arg):
        """one Assembly.assemble call -> its outputs (lower None without convection)"""
        c, E = self.case, self.case.E
        o = dict(lower=E(c.nf) if self.div else None, upper=E(c.nf), diag=E(c.n), mag=E(c.n), src=[E(c.n) for _ in range(self.R)])
        c.A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=ddt_arg, div=self.div, laplacian=c.lap, sp=self.sp,
                     su=self.su, sum_mag_out=o["mag"])
        return o

    def unfused(self, ddt_call):
        c = self.case
        return unfused_sequence(c.A, c.E, c.vol, ddt_call, self.R, c.lap, div=self.div, sp=self.sp, su=self.su)

    def euler(self, r_delta_t):
        """the Euler scheme's ddt_call on this variant's fields"""
        return euler_ddt_call(self.case.A, r_delta_t, self.case.vol, self.psi_old, **self.rho)

    def assert_same(self, got, seq, what):
        """(a) a fused call's coefficients and every source against an unfused sequence's"""
        host = self.case.host
        for key in ("lower", "upper", "diag"):
            if got[key] is not None:
                assert np.array_equal(host(got[key]), host(seq[key])), (self.tag, what, key)
        for r in range(self.R):
            assert np.array_equal(host(got["src"][r]), host(seq["src"][r])), (self.tag, what, r)

    def assert_restated(self, got, seq, restated_ddt):
        """(b) a fused call against the restatement: restated_ddt(r) -> (diag, source) of the time scheme for right-hand side r in numpy,
        the rest by the oracle's sweeps and numpy field operations, one rounding each; the corrected variants take the correction's face
        field from the engine's own face pass (seq["t"]), which tests/test_linear_upwind.py pins"""
        c, v, q, orc, host = self.case, self.v, self.case.q, self.case.orc, self.case.host
        n, lo, up = c.n, c.lo, c.up
        if self.div:
            wh = orc.upwind_weights(q["flux"]) if v["div"] is None else q["w"]
            lB, uB, dB = orc.fvm_div(n, lo, up, wh, q["flux"])
            lower, upper = lB - c.uL, uB - c.uL
        else:
            lower, upper = None, -c.uL
        for r in range(self.R):
            dD, s = restated_ddt(r)
            if v["corr"]:
                ivf = orc.surface_integrate(n, lo, up, host(seq["t"][r]), q["vol"])
                s = s - q["vol"] * ivf
            if v["extras"]:
                s = s - q["vol"] * q["su"][r]
                s = s + q["vol"] * q["su2"][r]
            assert np.array_equal(host(got["src"][r]), s), (self.tag, r)
        diag = ((dD + dB) - c.dL) if self.div else (dD - c.dL)
        if v["extras"]:
            diag = diag - q["vol"] * q["sp"]
        assert np.array_equal(host(got["diag"]), diag) and np.array_equal(host(got["upper"]), upper), self.tag
        if self.div:
            assert np.array_equal(host(got["lower"]), lower), self.tag
        assert np.array_equal(host(got["mag"]), orc.row_face_op(2, n, lo, up, lower, upper, np.zeros(n))), self.tag
