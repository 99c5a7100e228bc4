"""The row-pass skeleton (k_row_pass, k_row_assemble, k_gauss_grad, k_limited_grad, k_co_r_delta_t, k_row_sum3) and the tile kernel on the
meshes a box never brings: a cell without faces, a block of cells without faces, rows of thousands of faces, cell counts one short of, on
and one past a block boundary, and blocks below, at and past the limits of the block-local 16-bit row tables (assembly_support.py:
DEGENERATE_MESHES, block_counts).

CPU: every builder built what it claims (the three counts per block against the limits of ensure_caller_tables); the oracle's own results on
these meshes against a plain per-cell Python loop -- own faces ascending, then the neighbour-side faces in ascending face order, one rounded
operation per step -- bit for bit, so the reference is known to be right here before the device is held against it.
GPU: everything bit for bit."""
import numpy as np
import pytest

from assembly_support import (DEGENERATE_MESHES, EDGE_SIZES, HUB_SPOKES, ISOLATED_EMPTY, ISOLATED_N, ROW16_LIMITS, ROW_MODES, VARIANTS, FusedCase, bits,
                              block_counts, degenerate_case, fits_row16, fma, fma_each, gpu_env, row_blocks, row_passes_bit_exact, same,
                              set_row_blocks, set_row_tables, shaped_addressing, signed_flux)

LOOP_MESHES = tuple(m for m in DEGENERATE_MESHES if not m.startswith("dense_"))        # below 10 000 faces, and the two own_* meshes
_CASES = {}


def mesh(pkg, name, symmetric=False):
    """built once per session, shared and never written to"""
    key = (name, symmetric)
    if key not in _CASES:
        c = degenerate_case(pkg, name, symmetric=symmetric)
        _CASES[key] = c
    return _CASES[key]


# ---- CPU: the builders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_builder_gives_legal_upper_triangular_addressing(pkg, name):
    """owner < neighbour, faces sorted by (owner, neighbour), no pair twice; small enough for a few seconds per case (3 100 cells, 83 000 faces); coefficients of both
    forms, a dominant diagonal"""
    c, s = mesh(pkg, name), mesh(pkg, name, symmetric=True)
    n, nf, lo, up = c.n_cells, c.n_faces, c.lower_addr.astype(np.int64), c.upper_addr.astype(np.int64)
    assert n <= 3100 and nf <= 83000
    assert lo.dtype == up.dtype and c.lower_addr.dtype == np.int32 and lo.shape == up.shape == (nf,)
    if nf:
        assert lo.min() >= 0 and up.max() < n and np.all(lo < up)
        key = lo * n + up
        assert np.all(key[1:] > key[:-1])
        assert max(np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)) <= 4094          # what the tiling takes on one cell
    assert c.lower is not None and s.lower is None and np.array_equal(c.lower_addr, s.lower_addr) and np.array_equal(c.upper, s.upper)
    assert c.upper.shape == c.lower.shape == (nf,) and c.diag.shape == c.source.shape == (n,)
    assert np.all(c.upper <= -0.2) and np.all(c.lower <= -0.2) and (nf == 0 or not np.array_equal(c.upper, c.lower))
    off = np.zeros(n); np.add.at(off, lo, np.abs(c.lower)); np.add.at(off, up, np.abs(c.upper))
    assert np.all(c.diag >= off + 0.05 - 1e-12) and np.all(c.diag < off + 1.05 + 1e-12)


def test_faceless_meshes(pkg):
    one, none = mesh(pkg, "one_cell"), mesh(pkg, "no_faces")
    assert (one.n_cells, one.n_faces) == (1, 0) and (none.n_cells, none.n_faces) == (300, 0)
    assert len(block_counts(none, 256)[0]) == 2                                               # two 256-cell blocks
    assert all(int(x.sum()) == 0 for x in block_counts(none, 256))


def test_isolated_has_faceless_cells_and_a_faceless_block(pkg):
    c = mesh(pkg, "isolated")
    n, lo, up = c.n_cells, c.lower_addr, c.upper_addr
    assert n == ISOLATED_N == 1500
    deg = np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)
    a, b = ISOLATED_EMPTY
    assert (a, b) == (512, 768) and a % 256 == 0 and b - a == 256
    faceless = np.nonzero(deg == 0)[0]
    single = faceless[(faceless < a) | (faceless >= b)]
    assert len(single) == 37 and {0, 255, 256, 1023, 1024, n - 1} <= set(single.tolist()) and np.all(deg[a:b] == 0)
    own, cut, nbr = block_counts(c, 256)
    assert (own[2], cut[2], nbr[2]) == (0, 0, 0)                                              # the block 512..767: nothing staged, nothing walked
    assert all(own[k] > 0 and cut[k] > 0 for k in (3, 4, 5)) and own[0] > 0 and cut[0] == 0  # ... between blocks that have both
    # the kept labels carry a connected graph: a chain through all of them
    kept = np.nonzero(deg > 0)[0]
    pairs = set(zip(lo.tolist(), up.tolist()))
    assert len(kept) == n - 37 - 256 and all((int(p), int(q)) in pairs for p, q in zip(kept[:-1], kept[1:]))


def test_hubs_have_the_long_rows_where_they_claim(pkg):
    first, last = mesh(pkg, "hub_first"), mesh(pkg, "hub_last")
    m = HUB_SPOKES
    for c in (first, last):
        assert c.n_cells == m + 1 == 3001 and c.n_faces == 2 * m - 1
    # hub_first: block 0 owns more than 3 000 faces; every later block's first neighbour-side face is a cut face (owned by cell 0)
    own, cut, nbr = block_counts(first, 256)
    assert own[0] > 3000 and np.sum(first.lower_addr == 0) == m
    for bs in (256, 1024):
        for c0 in range(bs, m + 1, bs):
            f = np.nonzero(first.upper_addr == c0)[0]
            assert first.lower_addr[f[0]] == 0 and len(f) == 2                               # (0, c0) first, then (c0 - 1, c0): both cut
    # hub_last: the last cell walks 3 000 neighbour-side faces; all but those its own block owns are cut
    f = np.nonzero(last.upper_addr == m)[0]
    assert len(f) == m and np.sum(last.lower_addr == m) == 0
    for bs, least in ((256, 2700), (1024, 2000)):
        cut_of_last = int(np.sum(last.lower_addr[f] // bs != m // bs))
        assert cut_of_last >= least, (bs, cut_of_last)
        assert block_counts(last, bs)[1][-1] >= cut_of_last
    assert int(np.sum(last.lower_addr[f] // 256 != m // 256)) == 2816


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_edge_meshes_sit_on_the_block_boundaries(pkg, n):
    c = mesh(pkg, f"edge_{n}")
    assert c.n_cells == n and n in (255, 256, 257, 1023, 1024, 1025)
    bs = 256 if n < 1000 else 1024
    blocks = len(block_counts(c, bs)[0])
    assert blocks == (1 if n <= bs else 2) and (n - bs) in (-1, 0, 1)
    if n > bs:                                                                               # one past: a last block of ONE cell, all its faces cut
        own, cut, nbr = block_counts(c, bs)
        assert own[1] == 0 and cut[1] == nbr[1] >= 1


@pytest.mark.parametrize("name,fits", [("dense_fits", True), ("own_32767", True), ("dense_fallback", False), ("own_32768", False)])
def test_row16_threshold_meshes_are_on_their_side_of_the_limits(pkg, name, fits):
    """own faces < 32 768, cut faces < 32 768 and neighbour-list entries < 65 536 in every 1024-cell block -- or not: what
    ensure_caller_tables decides by under MI_ROW_BS=1024 (the default), stated on the host"""
    c = mesh(pkg, name)
    own, cut, nbr = block_counts(c, 1024)
    assert ROW16_LIMITS == (32768, 32768, 65536)
    assert fits_row16(c, 1024) == fits, (own, cut, nbr)
    if name == "dense_fits":                                                                 # the 15-bit fields run well past 2^14
        assert 16384 < own[0] < 32768 and max(int(nbr.max()), int(own.max())) > 16384
    if name == "dense_fallback":
        assert own[0] >= 32768 and c.n_faces <= 83000
    if name.startswith("own_"):
        assert own[0] == int(name[4:]) and own[1] == own[2] == 0 and c.n_cells == 3072
        assert cut[1] + cut[2] == own[0] and nbr[0] == 0 and cut.max() < 32768 and nbr.max() < 65536      # the own faces alone decide
        assert fits_row16(c, 256)                                                           # 8 192 own faces per 256-cell block: always 16-bit


def test_block_counts_on_a_mesh_counted_by_hand(pkg):
    """cells 0..5 in blocks of 2: faces (0,1) (0,4) (1,2) (2,3) (3,5) (4,5)"""
    from assembly_support import case_from_pairs
    c = case_from_pairs(pkg, 6, [0, 0, 1, 2, 3, 4], [1, 4, 2, 3, 5, 5], 3)
    own, cut, nbr = block_counts(c, 2)
    assert own.tolist() == [3, 2, 1] and nbr.tolist() == [1, 2, 3] and cut.tolist() == [0, 1, 2]


# ---- CPU: the oracle against plain per-cell loops ----------------------------------------------------------------------------------------
def rows(c):
    """own[c], nei[c]: every cell's own faces and its neighbour-side faces, both in ascending face order"""
    own, nei = [[] for _ in range(c.n_cells)], [[] for _ in range(c.n_cells)]
    for f, (p, q) in enumerate(zip(c.lower_addr.tolist(), c.upper_addr.tolist())):
        own[p].append(f); nei[q].append(f)
    return own, nei


def row_loop(own, nei, start, own_term, nei_term):
    out = []
    for c, x in enumerate(start):
        for f in own[c]:
            x = x + own_term[f]
        for f in nei[c]:
            x = x + nei_term[f]
        out.append(x)
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("name", LOOP_MESHES)
def test_oracle_row_sweeps_against_plain_loops(pkg, orc, name):
    """row_face_op 0/1/2 symmetric and asymmetric, fvm_laplacian, fvm_div, surface_integrate with and without volumes, gauss_grad"""
    syn = pkg.synthetic
    c = mesh(pkg, name)
    n, nf, lo, up = c.n_cells, c.n_faces, c.lower_addr, c.upper_addr
    own, nei = rows(c)
    for lower in (c.lower, None):
        L = c.upper if lower is None else lower
        for kind in (0, 1, 2):
            start = syn.splitmix_uniform(kind, n)
            o, q = ((L, c.upper), (-L, -c.upper), (np.abs(c.upper), np.abs(L)))[kind]
            want = row_loop(own, nei, start.tolist(), o.tolist(), q.tolist())
            assert same(orc.row_face_op(kind, n, lo, up, lower, c.upper, start), want), (kind, lower is None)
    zero = [0.0] * n
    delta, gam = 1.0 + syn.splitmix_uniform(7, nf), 0.5 + syn.splitmix_uniform(8, nf)
    ru, rd = orc.fvm_laplacian(n, lo, up, delta, gam)
    u = delta * gam
    assert same(ru, u) and same(rd, row_loop(own, nei, zero, (-u).tolist(), (-u).tolist()))
    w, phi = syn.splitmix_uniform(9, nf), syn.splitmix_uniform(10, nf) - 0.5
    rl, ru, rd = orc.fvm_div(n, lo, up, w, phi)
    l = -w * phi
    u = l + phi
    assert same(rl, l) and same(ru, u) and same(rd, row_loop(own, nei, zero, (-l).tolist(), (-u).tolist()))
    vol = 0.5 + syn.splitmix_uniform(11, n)
    s = row_loop(own, nei, zero, phi.tolist(), (-phi).tolist())
    assert same(orc.surface_integrate(n, lo, up, phi), s) and same(orc.surface_integrate(n, lo, up, phi, vol), s / vol)
    Sf = [syn.splitmix_uniform(20 + k, nf) - 0.5 for k in range(3)]
    got = orc.gauss_grad(n, lo, up, Sf, phi, vol)
    ph = phi.tolist()
    for k in range(3):
        sk, want = Sf[k].tolist(), []
        for cell in range(n):
            x = 0.0
            for f in own[cell]:
                x = fma(sk[f], ph[f], x)
            for f in nei[cell]:
                x = fma(-sk[f], ph[f], x)
            want.append(x)
        assert same(got[k], np.array(want, dtype=np.float64) / vol), k
    if nf == 0:
        assert all(np.all(bits(x) == 0) for x in (rd, s, *got))                              # empty sums: +0.0


@pytest.mark.parametrize("name", LOOP_MESHES)
def test_oracle_matrix_products_against_plain_loops(pkg, orc, name):
    """System.amul / tmul / sumA, symmetric and asymmetric: diag*psi, then one fma per face in row order"""
    syn = pkg.synthetic
    for symmetric in (False, True):
        c = mesh(pkg, name, symmetric)
        n, lo, up = c.n_cells, c.lower_addr.tolist(), c.upper_addr.tolist()
        own, nei = rows(c)
        S = orc.System([c])
        psi = syn.splitmix_uniform(61, n) - 0.5
        x, d = psi.tolist(), c.diag.tolist()
        U, L = c.upper.tolist(), (c.upper if symmetric else c.lower).tolist()
        for fn, A, B in ((S.amul, U, L), (S.tmul, L, U)):                                    # A: the own faces' coefficients, B: the neighbour side's
            want = []
            for cell in range(n):
                out = d[cell] * x[cell]
                for f in own[cell]:
                    out = fma(A[f], x[up[f]], out)
                for f in nei[cell]:
                    out = fma(B[f], x[lo[f]], out)
                want.append(out)
            assert same(fn(psi), np.array(want, dtype=np.float64)), (symmetric, fn.__name__)
        assert same(S.sumA(), row_loop(own, nei, d, U, L)), symmetric


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
MODE_MESHES = ("isolated", "hub_first", "hub_last", "edge_1025", "dense_fits")
ROW32_MESHES = ("hub_first", "hub_last", "dense_fits")
THRESHOLD_MESHES = (("own_32767", True), ("own_32768", False), ("dense_fits", True), ("dense_fallback", False))
FUSED_MESHES = ("isolated", "hub_first", "hub_last", "no_faces", "one_cell", "edge_257")
GRAD_MESHES = ("isolated", "hub_first", "hub_last", "one_cell")
TILE_MESHES = ("no_faces", "isolated", "hub_first", "hub_last", "dense_fallback")
ROW_ENV = ("MI_ROW_BS", "MI_GRAD_BS", "MI_ROW_CAP", "MI_TILE_CELLS")


def shaped(pkg, monkeypatch, name, mode, tables, grad=True):
    """the mesh under the row tables and the block shape of one ROW_MODES entry (mode None: every default) -> eng, ctx, dev, host, E, case,
    addr, the cells per fixed block.  The fixed modes also cut the layout's tiles to the block's size: a numbering that is tile-contiguous
    as it stands (hub_first, the edge meshes) is owned tile by tile, whatever MI_ROW_BS says"""
    for k in ROW_ENV:
        monkeypatch.delenv(k, raising=False)
    set_row_tables(monkeypatch, tables)
    bs = 1024
    if mode is not None:
        set_row_blocks(monkeypatch, mode, grad=grad)
        bs = 1024 if mode == "fixed1024" else 256
        if mode.startswith("fixed"):
            monkeypatch.setenv("MI_TILE_CELLS", str(bs))
    eng, ctx, dev, host, E = gpu_env(pkg)
    case, addr = shaped_addressing(eng, ctx, pkg.synthetic, mesh(pkg, name), mode or "fixed1024")
    assert bool(addr.is_ordered) or not (mode or "").startswith("tiles")
    return eng, ctx, dev, host, E, case, addr, bs


def assert_block_shape(name, case, blocks):
    """the shape a mesh is here for, on the blocks the row passes really own under this addressing (assembly_support.row_blocks)"""
    own, cut, nbr = block_counts(case, blocks)
    cells = np.diff(blocks)
    last = len(own) - 1
    if name == "hub_first":                                  # block 0 stages the hub's row; every cell of a later block starts with a cut face
        assert own[0] > 3000 and np.all(cut[1:] >= cells[1:])
    if name == "hub_last":
        assert nbr[last] >= HUB_SPOKES and cut[last] >= HUB_SPOKES - 1024
    if name == "isolated" and int(cells.max()) <= 256:       # a whole block that stages nothing and walks nothing, between blocks that do
        assert np.any((own == 0) & (nbr == 0) & (cells == 256)) and np.any(cut > 0)


def run_rows(pkg, orc, monkeypatch, name, mode, tables):
    eng, ctx, dev, host, E, case, addr, bs = shaped(pkg, monkeypatch, name, mode, tables)
    got = row_passes_bit_exact(eng, orc, pkg.synthetic, case, addr, dev, host, E)
    if mode is not None and not mode.startswith("tiles"):
        assert_block_shape(name, case, row_blocks(addr, case, bs))
    return got, case, addr


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_row_passes_on_every_mesh(pkg, orc, monkeypatch, name):
    """(a) every row pass against the oracle under the default tables and blocks"""
    run_rows(pkg, orc, monkeypatch, name, None, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ROW_MODES)
@pytest.mark.parametrize("name", MODE_MESHES)
def test_row_passes_in_every_block_shape(pkg, orc, monkeypatch, name, mode):
    """(a) 256- and 1024-cell blocks, the layout's tiles under ordered addressing, and the unstaged path of a block that does not fit"""
    run_rows(pkg, orc, monkeypatch, name, mode, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ROW_MODES)
@pytest.mark.parametrize("name", ROW32_MESHES)
def test_row_passes_with_the_32_bit_tables(pkg, orc, monkeypatch, name, mode):
    """(a) ... and with the forced 32-bit row tables (MI_ROW16=0)"""
    run_rows(pkg, orc, monkeypatch, name, mode, "row32")


@pytest.mark.gpu
@pytest.mark.parametrize("name,fits", THRESHOLD_MESHES)
def test_row16_threshold(pkg, orc, monkeypatch, name, fits):
    """(b) under MI_ROW_BS=1024 a block at the limit of the 16-bit row tables sends the whole addressing to the 32-bit ones, a block one
    face short of it does not: the oracle's bits on both sides, and where the tables fell back by themselves, array by array the bits of
    the forced MI_ROW16=0.  Which form was taken is stated by the host-side counts: the blocks are fixed ranges (the layout permutes
    these meshes), and ensure_caller_tables decides by exactly these three counts"""
    got, case, addr = run_rows(pkg, orc, monkeypatch, name, "fixed1024", "default")
    assert not addr.is_ordered and fits_row16(case, 1024) == fits
    if fits:
        return
    forced, _, addr32 = run_rows(pkg, orc, monkeypatch, name, "fixed1024", "row32")
    assert not addr32.is_ordered and sorted(forced) == sorted(got)
    for k in sorted(got):
        assert same(got[k], forced[k]), k


# ---- (c) the fused assembly ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed256", "tiles"])
@pytest.mark.parametrize("name", FUSED_MESHES)
def test_fused_assembly_in_every_time_form(pkg, orc, monkeypatch, name, mode):
    """mi_fvm_assemble* -- Euler, backward, CrankNicolson, local (rDeltaT per cell) with and without the bounded convection -- against the
    engine's own scheme-by-scheme sequence over every entry of VARIANTS, and the Euler form against the restatement"""
    import test_backward_ddt as bw
    from test_bounded_steady import unfused_bounded
    from test_local_ddt import local_ddt_call
    for k in ROW_ENV:
        monkeypatch.delenv(k, raising=False)
    if mode == "fixed256":
        monkeypatch.setenv("MI_TILE_CELLS", "256")
    F = FusedCase(pkg, orc, monkeypatch, name, mode, "default")
    dev, host, A, q, n = F.dev, F.host, F.A, F.q, F.n
    assert bool(F.addr.is_ordered) or mode != "tiles"
    if mode == "fixed256":
        assert_block_shape(name, F.case, row_blocks(F.addr, F.case, 256))
    u = pkg.synthetic.splitmix_uniform
    rdt, rdt_cn, oc = 1.0 / 0.004, 1.9 / 0.004, 0.9
    cb = bw.coeffs(0.004, 0.01)
    ddt0 = [40.0 * (u(181 + k, n) - 0.5) for k in range(3)]
    r = dev(50.0 + 400.0 * u(185, n))
    dph = orc.surface_integrate(n, F.lo, F.up, q["flux"], q["vol"])
    dph[::9] = 0.0
    div_phi = dev(dph)
    for v in VARIANTS:
        V = F.variant(v)
        eul = V.fused(dict(V.ddt, r_delta_t=rdt))
        seq = V.unfused(V.euler(rdt))
        V.assert_same(eul, seq, "euler")
        rho, rho0 = (q["rho"], q["rho0"]) if v["field"] else (1.2, 1.2)
        V.assert_restated(eul, seq, lambda k: ((rdt * rho) * q["vol"], ((rdt * rho0) * q["psi0"][k]) * q["vol"]))
        got = V.fused(dict(V.ddt, r_delta_t=rdt, backward=bw.backward_arg(V, cb)))
        V.assert_same(got, V.unfused(bw.backward_ddt_call(V, rdt, cb)), "backward")
        cn = dict(oc=oc, ddt0=[dev(x) for x in ddt0[:V.R]])
        got = V.fused(dict(V.ddt, r_delta_t=rdt_cn, crank_nicolson=cn))
        V.assert_same(got, V.unfused(lambda k, dd, ds: A.fvm_ddt_cn(rdt_cn, oc, F.vol, V.psi_old[k], cn["ddt0"][k], dd, ds, **V.rho)), "cn")
        got = V.fused(dict(V.ddt, local=dict(r_delta_t=r)))
        V.assert_same(got, V.unfused(local_ddt_call(V, r)), "local")
        if V.div is None:                                    # bounded needs a convection term (tests/test_bounded_steady.py has the refusal)
            continue
        V.div["bounded"] = div_phi
        got = V.fused(dict(V.ddt, local=dict(r_delta_t=r)))
        del V.div["bounded"]
        V.assert_same(got, unfused_bounded(V, local_ddt_call(V, r), div_phi), "local + bounded")


# ---- (d) the gradient plan's passes and CoEuler's ----------------------------------------------------------------------------------------------
_RESTATED = {}


def grad_case(pkg, name, nc):
    """synthetic centres and face centres as tests/test_limited_grad.py's random-graph case takes them, no patches; the fields"""
    import test_limited_grad as lg
    c = mesh(pkg, name)
    M = lg.random_geometry(pkg.synthetic, c.n_cells, c.lower_addr, c.upper_addr, 70, n_patches=0)
    return (M,) + lg.fields(pkg.synthetic, M, nc, 80 + nc, gscale=4.0)


def restated_grad(pkg, name, kind, nc, k):
    """tests/test_limited_grad.py's vectorised restatement, once per (mesh, kind, components, k)"""
    import test_limited_grad as lg
    key = (name, kind, nc, k)
    if key not in _RESTATED:
        M, vf, grad, bv = grad_case(pkg, name, nc)
        _RESTATED[key] = lg.restate(kind, k, M["n"], M["lo"], M["up"], M["C"], M["Cf"], vf, grad)        # no patches: no boundary arguments
    return _RESTATED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cellLimited", "cellMDLimited", "faceLimited", "faceMDLimited"])
@pytest.mark.parametrize("mode", ["fixed256", "fixed1024"])
@pytest.mark.parametrize("name", GRAD_MESHES)
def test_limited_grad_on_degenerate_meshes(pkg, monkeypatch, name, mode, kind):
    """k_limited_grad in gradient-plan blocks of 256 and 1024 cells: scalar and vector, k = 1 and 0.5, against the restatement"""
    import test_limited_grad as lg
    eng, ctx, dev, host, E, case, addr, bs = shaped(pkg, monkeypatch, name, mode, "default")
    assert_block_shape(name, case, row_blocks(addr, case, bs))
    A = eng.Assembly(addr)
    for nc in (1, 3):
        M, vf, grad, bv = grad_case(pkg, name, nc)
        for k in (1.0, 0.5):
            g, lim = lg._engine_run(eng, A, None, kind, k, M, vf, grad, bv, dev, host)
            rg, rlim = restated_grad(pkg, name, kind, nc, k)
            for i in range(3 * nc):
                assert same(g[i], rg[i]), (kind, nc, k, "grad", i, int(np.sum(bits(g[i]) != bits(rg[i]))))
            for j in range(len(rlim or ())):
                assert same(lim[j], rlim[j]), (kind, nc, k, "limiter", j)
            if case.n_faces:
                assert not all(same(x, y) for x, y in zip(g, grad)), (kind, nc, k)             # the data reach the limiter


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed256", "fixed1024"])
@pytest.mark.parametrize("name", GRAD_MESHES)
def test_co_r_delta_t_and_div_dev_tgrad_on_degenerate_meshes(pkg, orc, monkeypatch, name, mode):
    """k_co_r_delta_t against the restatement of tests/test_local_ddt.py (volumetric and mass flux; a cell without faces keeps 0.0), and
    mi_fvc_div_dev_tgrad (k_row_sum3) against three mi_flux_div calls on glue-formed tensors and against the oracle, as
    tests/test_div_dev_tgrad.py states it"""
    from test_div_dev_tgrad import COEFF, x_of
    from test_local_ddt import co_cells, co_face
    eng, ctx, dev, host, E, case, addr, bs = shaped(pkg, monkeypatch, name, mode, "default")
    u = pkg.synthetic.splitmix_uniform
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    A = eng.Assembly(addr)
    dc, mag_sf, phi = 1.0 + u(40, nf), 0.5 + u(41, nf), 31.0 * signed_flux(u(42, nf))
    lam, rho0 = 0.001 + 0.998 * u(43, nf), 0.7 + u(44, n)
    dt, max_co = 0.02, 0.5
    out = E(n)
    for mass in (False, True):
        rho_f = fma_each(lam, rho0[lo] - rho0[up], rho0[up]) if mass else None
        phis = phi * (1.2 if mass else 1.0)
        want = co_cells(n, lo, up, co_face(dc, phis, mag_sf, dt, max_co, rho_f=rho_f))
        deg = np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)
        assert np.all(want[deg == 0] == 0.0) and np.all(want[deg > 0] >= 1.0 / dt)
        if nf:
            assert np.any(want > 1.0 / dt) and np.any(want == 1.0 / dt)                        # both branches of the max
        kw = dict(lam=dev(lam), rho_old=dev(rho0)) if mass else {}
        A.co_r_delta_t(dev(dc), dev(mag_sf), dev(phis), dt, max_co, out, **kw)
        assert same(host(out), want), (mass, int(np.sum(host(out) != want)))
    g = [128.0 * (u(90 + i, n) - 0.5) for i in range(9)]
    visc, vol = 0.5 + u(99, n), 0.5 + u(100, n)
    sf = [u(101 + k, nf) - 0.5 for k in range(3)]
    lamd, sfd, viscd, gd, vold = dev(lam), [dev(x) for x in sf], dev(visc), [dev(x) for x in g], dev(vol)
    for kind in ("dev", "dev2"):
        for with_vol in (True, False):
            face, div = [E(nf) for _ in range(3)], [E(n) for _ in range(3)]
            A.div_dev_tgrad(kind, lamd, sfd, viscd, gd, face, div, vold if with_vol else None)
            tr = (gd[0] + gd[4]) + gd[8]
            ii = COEFF[kind] * tr
            x = [gd[i] - ii if i % 4 == 0 else gd[i] for i in range(9)]
            xh, _ = x_of(kind, g)
            for j in range(3):
                p, d = E(nf), E(n)
                A.flux_div(lamd, sfd, [x[j], x[3 + j], x[6 + j]], p, d, cell_scale=viscd, vol=vold if with_vol else None)
                assert same(host(face[j]), host(p)) and same(host(div[j]), host(d)), (kind, with_vol, j)
                rp, rd = orc.flux_div(n, lo, up, lam, sf, [xh[j], xh[3 + j], xh[6 + j]], scale=visc, vol=vol if with_vol else None)
                assert same(host(face[j]), rp) and same(host(div[j]), rd), (kind, with_vol, j)


# ---- (e) the same meshes through the tile kernel ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("name,ordered", [(m, False) for m in TILE_MESHES] + [("isolated", True)])
def test_tile_kernel_on_degenerate_meshes(pkg, orc, monkeypatch, name, ordered, symmetric):
    """amul, tmul, sumA, residual, H, H1, faceH, the diagonal and DILU preconditioners and the Jacobi smoother against the oracle's System"""
    for k in ROW_ENV:
        monkeypatch.delenv(k, raising=False)
    eng, ctx, dev, host, E = gpu_env(pkg)
    case = mesh(pkg, name, symmetric)
    n, nf = case.n_cells, case.n_faces
    addr = eng.Addressing(ctx, n, case.lower_addr, case.upper_addr, ordered=ordered)
    assert bool(addr.is_ordered) or not ordered
    mat = eng.Matrix(addr)
    mat.set_coeffs(dev(case.diag), dev(case.upper), None if case.lower is None else dev(case.lower))
    S = orc.System([case])
    x = pkg.synthetic.splitmix_uniform(99, n) - 0.5
    xd, bd, out = dev(x), dev(case.source), E(n)
    mat.amul(xd, out); assert same(host(out), S.amul(x))
    mat.tmul(xd, out); assert same(host(out), S.tmul(x))
    mat.sumA(out); assert same(host(out), S.sumA())
    mat.residual(xd, bd, out); assert same(host(out), S.residual(x, case.source))
    mat.H(xd, out); assert same(host(out), S.H(x))
    mat.H1(out); assert same(host(out), S.H1())
    fh = E(nf)
    mat.faceH(xd, fh); assert same(host(fh), S.faceH(x))
    for kind in ("diagonal", "DILU"):
        for tr in (False, True):
            mat.precondition(kind, xd, out, transpose=tr)
            assert same(host(out), S.precondition(kind, x, transpose=tr)), (kind, tr)
    psi = dev(x.copy())
    mat.jacobi_smooth(psi, bd, 3, omega=0.9)
    assert same(host(psi), S.jacobi_smooth(x, case.source, 3, omega=0.9))
    assert same(host(xd), x)                                                                   # the operators did not write to their input
