"""fvc::div(nuEff*dev(T(fvc::grad(U)))) / fvc::div(muEff*dev2(T(fvc::grad(U)))): the explicit term of divDevReff / divDevRhoReff
(incompressible laminar.C:202-225, compressible laminar.C:197) -- mi_fvc_div_dev_tgrad on the internal faces, mi_patch_gauss_grad_correct
for the boundary values of the gradient, mi_patch_dev_tgrad_flux for the boundary faces, and the whole term into a source.

The expected values are a restatement written here from the pinned oracle, one numpy operator per field operator of the reference and
each rounded, so every comparison with the engine is bit for bit.  grad[3*j + k] = d(U_j)/dx_k; per cell
    tr = (grad[0] + grad[4]) + grad[8]                TensorI.H:465-468
    ii = coeff*tr                                     coeff 1.0/3.0 (dev) | 2.0/3.0 (dev2), TensorI.H:534-546
    X_kj = grad[3*k + j] - (k == j ? ii : 0)          T(...) keeps the diagonal; x[3*k + j]
    Y_kj = visc*X_kj
internal faces: component j is orc.flux_div(v = column j of X = (x[j], x[3 + j], x[6 + j]), scale = visc) -- the oracle's flux_face and
orc_surface_integrate.  The patch forms are written out with the exact-rational fma for the contracted dots
(fma(I_zj, Sf_z, fma(I_xj, Sf_x, I_yj*Sf_y)), the engine's dot rule: DESIGN 3.5a)."""
import ctypes as C
import functools

import numpy as np
import pytest

from assembly_support import ROW_MODES, fma_each, gpu_env, set_row_blocks

EPS = np.finfo(np.float64).eps
COEFF = {"dev": 1.0 / 3.0, "dev2": 2.0 / 3.0}
MESHES = [(3, 2, 2), (9, 8, 7), (13, 11, 9)]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def x_of(kind, g):
    """dev[2](T(grad)) of nine arrays -> (x[3*k + j] = X_kj, ii)"""
    tr = (g[0] + g[4]) + g[8]
    ii = COEFF[kind] * tr
    return [g[i] - ii if i % 4 == 0 else g[i].copy() for i in range(9)], ii


def y_of(kind, visc, g):
    return [visc * x for x in x_of(kind, g)[0]]


def dot_col(t, j, s):
    """Sf & column j of the tensor t (t[3*k + j]): fma(t_zj, Sf_z, fma(t_xj, Sf_x, t_yj*Sf_y))"""
    return fma_each(t[6 + j], s[2], fma_each(t[j], s[0], t[3 + j] * s[1]))


def internal(orc, M, kind, visc, g, vol):
    """-> (three face arrays, three cell arrays)"""
    n, nI, lo, up, G = M["n"], M["nI"], M["lo"], M["up"], M["G"]
    sf = [np.ascontiguousarray(G["Sf"][:nI, k]) for k in range(3)]
    x, _ = x_of(kind, g)
    res = [orc.flux_div(n, lo, up, G["weights"], sf, [x[j], x[3 + j], x[6 + j]], scale=visc, vol=vol) for j in range(3)]
    return [r[0] for r in res], [r[1] for r in res]


def patch_flux_boundary(kind, s, visc_b, g_b):
    """a patch that is not coupled: Sf_b & (visc_b*dev[2](T(G_b))) from the patch's own boundary values"""
    y = y_of(kind, visc_b, g_b)
    return [dot_col(y, j, s) for j in range(3)]


def patch_flux_coupled(kind, fc, s, w, visc, g, nvisc, ng):
    """a coupled patch: Y on each side, I = (w*Y_P) + ((1 - w)*Y_N) uncontracted, then the dot"""
    yp, yn = y_of(kind, visc[fc], [a[fc] for a in g]), y_of(kind, nvisc, ng)
    m = 1.0 - w
    t = [(w * p) + (m * q) for p, q in zip(yp, yn)]
    return [dot_col(t, j, s) for j in range(3)]


def gauss_grad_correct(fc, s, mag, sn, g):
    """gaussGrad.C:277-303: gb_k = g_k + n_k*(sn_j - (n & g)), n = Sf/magSf; sn one array per component, g three per component"""
    nh = [s[k] / mag for k in range(3)]
    out = []
    for j in range(len(sn)):
        gc = [g[3 * j + k][fc] for k in range(3)]
        d = sn[j] - fma_each(nh[2], gc[2], fma_each(nh[0], gc[0], nh[1] * gc[1]))
        out += [gc[k] + (nh[k] * d) for k in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def mesh(dims):
    from test_assembly import skewed_mesh
    return skewed_mesh(dims)


@functools.lru_cache(maxsize=None)
def fields(dims):
    """`gradients` in [-64, 64) (not a Gauss gradient: every component matters), a viscosity in [0.5, 1.5) that varies per cell"""
    import __graft_entry__ as graft
    syn = graft.load_package().synthetic
    n = mesh(dims)["n"]
    g = (syn.splitmix_uniform(21, 9 * n) - 0.5) * 128
    visc = 0.5 + syn.splitmix_uniform(22, n)
    return [np.ascontiguousarray(g[i * n:(i + 1) * n]) for i in range(9)], visc


@functools.lru_cache(maxsize=None)
def expected(dims, kind, with_vol):
    from oracle import oracle as orc
    M = mesh(dims)
    g, visc = fields(dims)
    return internal(orc, M, kind, visc, g, M["G"]["V"] if with_vol else None)


def patch_geometry(M, name):
    """faceCells and the Sf components / magSf / deltaCoeffs of one boundary patch of the box"""
    (cnt, start), = [(c, s) for nm, _, c, s in M["patches"] if nm == name]
    G, nI = M["G"], M["nI"]
    return (M["owner"][start:start + cnt].astype(np.int32), [np.ascontiguousarray(G["Sf"][start:start + cnt, k]) for k in range(3)],
            np.ascontiguousarray(G["magSf"][start:start + cnt]), np.ascontiguousarray(G["delta_b"][start - nI:start - nI + cnt]))


def uniform(seed, m, lo, hi):
    import __graft_entry__ as graft
    return lo + (hi - lo) * graft.load_package().synthetic.splitmix_uniform(seed, m)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_symbols_kinds_and_the_refusals_that_need_no_device(pkg):
    eng = pkg.engine
    lib = eng.lib()
    names = ("mi_fvc_div_dev_tgrad", "mi_patch_gauss_grad_correct", "mi_patch_dev_tgrad_flux")
    for name in names:
        assert name in eng.SYMBOLS and hasattr(lib, name)
    assert eng.DEV_KINDS == ("dev", "dev2")
    null, tab = C.c_void_p(0), (C.c_void_p * 9)()
    err = lambda: lib.mi_last_error().decode()
    for kind in (0, 1):                                                       # a NULL handle
        assert lib.mi_fvc_div_dev_tgrad(null, C.c_int32(kind), null, null, null, null, null, tab, null, tab, tab) != 0 and names[0] in err()
        assert lib.mi_patch_dev_tgrad_flux(null, C.c_int32(kind), null, null, null, null, null, tab, null, tab, tab) != 0 and names[2] in err()
    for n_comp in (1, 3):
        assert lib.mi_patch_gauss_grad_correct(null, C.c_int32(n_comp), null, null, null, null, tab, tab, tab) != 0 and names[1] in err()
    for kind in (-1, 2, 7):                                                   # a kind other than the two
        assert lib.mi_fvc_div_dev_tgrad(null, C.c_int32(kind), null, null, null, null, null, tab, null, tab, tab) != 0
        assert names[0] in err() and "kind" in err()
        assert lib.mi_patch_dev_tgrad_flux(null, C.c_int32(kind), null, null, null, null, null, tab, null, tab, tab) != 0
        assert names[2] in err() and "kind" in err()
    for n_comp in (0, 2, 4):
        assert lib.mi_patch_gauss_grad_correct(null, C.c_int32(n_comp), null, null, null, null, tab, tab, tab) != 0
        assert names[1] in err() and "n_comp" in err()


def test_restatement_dev_and_dev2_differ_by_ii_and_dev_has_no_trace(pkg):
    kinds = pkg.engine.DEV_KINDS
    g, _ = fields((9, 8, 7))
    (xd, iid), (x2, ii2) = x_of(kinds[0], g), x_of(kinds[1], g)
    for i in range(9):
        if i % 4:                                                              # off-diagonals: untouched, the transposed storage
            assert np.array_equal(xd[i], g[i]) and np.array_equal(x2[i], g[i])
        else:
            assert np.array_equal(xd[i], g[i] - iid) and np.array_equal(x2[i], g[i] - ii2) and not np.array_equal(xd[i], x2[i])
    # where tr is a multiple of 3 every step is exact: the two kinds differ by exactly ii(dev) on the diagonal, and ii(dev2) = 2 ii(dev)
    n = g[0].shape[0]
    gi = [np.round(a) for a in g]
    gi[8] = gi[8] + (3.0 * np.round(np.arange(n) % 5 - 2.0) - ((gi[0] + gi[4]) + gi[8])) % 3.0
    tr = (gi[0] + gi[4]) + gi[8]
    assert np.all(tr % 3.0 == 0) and np.any(tr != 0)
    (xd, iid), (x2, ii2) = x_of(kinds[0], gi), x_of(kinds[1], gi)
    assert np.array_equal(iid, tr / 3.0) and np.array_equal(ii2, 2.0 * iid)
    for i in (0, 4, 8):
        assert np.array_equal(xd[i] - x2[i], iid)
    assert np.all((xd[0] + xd[4]) + xd[8] == 0.0)
    # the trace of dev's X is zero to rounding.  With S = |g0| + |g4| + |g8| and u = EPS/2: tr carries 2uS, ii = fl(fl(1/3)*tr) is within
    # (4/3)uS of tr/3, the three differences add u(|g_d| + |ii|) <= 2uS in all, summing them 2u*2S: below 10uS = 5 EPS S; asserted at 8 EPS S
    g, _ = fields((13, 11, 9))
    xd, _ = x_of(kinds[0], g)
    S = np.abs(g[0]) + np.abs(g[4]) + np.abs(g[8])
    assert np.all(np.abs((xd[0] + xd[4]) + xd[8]) <= 8 * EPS * S)
    x2, _ = x_of(kinds[1], g)
    assert np.max(np.abs((x2[0] + x2[4]) + x2[8])) > 1.0                       # dev2 keeps -tr


def test_restatement_constant_stress_sums_to_zero_in_a_closed_cell(pkg, orc):
    """constant viscosity and the exact, constant gradient of a linear velocity field: Y is one tensor, every face flux is Sf & Y, and the
    faces of a closed cell sum to zero -- the raw sum of a fully interior cell is rounding only"""
    M = mesh((9, 8, 7))
    n, nI, G = M["n"], M["nI"], M["G"]
    b = np.array([[0.7, -1.3, 0.45], [0.2, 0.9, -0.4], [-1.1, 0.3, 0.8]])     # U_j = b[j] . x: grad[3*j + k] = b[j][k]
    g = [np.full(n, b[j][k]) for j in range(3) for k in range(3)]
    visc = np.full(n, 1.25)
    interior = np.ones(n, bool); interior[M["owner"][nI:]] = False
    assert interior.sum() == 7 * 6 * 5
    for kind in pkg.engine.DEV_KINDS:
        face, raw = internal(orc, M, kind, visc, g, None)
        y = np.array([a[0] for a in y_of(kind, visc, g)])
        bound = 64 * EPS * np.max(G["magSf"][:nI]) * np.sqrt(np.sum(y * y))
        for j in range(3):
            assert np.max(np.abs(face[j])) > 1e3 * bound                     # the fluxes themselves are not small
            assert np.max(np.abs(raw[j][interior])) < bound, (kind, j)
            assert np.max(np.abs(raw[j][~interior])) > 1e3 * bound           # an open cell keeps its sum: the boundary faces are the patches' part


def test_restatement_solenoidal_field_gives_both_kinds_the_same_bits(pkg, orc):
    M = mesh((9, 8, 7))
    n = M["n"]
    b = np.array([[1.5, -1.3, 0.45], [0.2, -0.25, -0.4], [-1.1, 0.3, -1.25]])  # tr = (1.5 - 0.25) - 1.25 == 0 exactly
    g = [np.full(n, b[j][k]) for j in range(3) for k in range(3)]
    visc = np.full(n, 0.75)
    kinds = pkg.engine.DEV_KINDS
    assert np.all(x_of(kinds[0], g)[1] == 0.0) and np.all(x_of(kinds[1], g)[1] == 0.0)
    (fa, da), (fb, db) = internal(orc, M, kinds[0], visc, g, M["G"]["V"]), internal(orc, M, kinds[1], visc, g, M["G"]["V"])
    for j in range(3):
        assert np.array_equal(fa[j], fb[j]) and np.array_equal(da[j], db[j]) and np.any(fa[j] != 0)
    # and with the varying fields they do differ
    (fa, _), (fb, _) = expected((9, 8, 7), kinds[0], True), expected((9, 8, 7), kinds[1], True)
    assert not np.array_equal(fa[0], fb[0])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _inputs(M, dims, dev):
    G, nI = M["G"], M["nI"]
    g, visc = fields(dims)
    return dev(G["weights"]), [dev(G["Sf"][:nI, k]) for k in range(3)], dev(visc), [dev(a) for a in g], dev(G["V"])


def _run(eng, addr, kind, lam, sf, visc, g, vol, E, host):
    A = eng.Assembly(addr)
    nI, n = lam.numel(), visc.numel()
    face, div = [E(nI) for _ in range(3)], [E(n) for _ in range(3)]
    A.div_dev_tgrad(kind, lam, sf, visc, g, face, div, vol)
    return [host(x) for x in face], [host(x) for x in div]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", MESHES)
@pytest.mark.parametrize("kind", ["dev", "dev2"])
def test_engine_internal_faces_bit_exact(pkg, orc, dims, kind):
    """(3, 2, 2): one partial block; (9, 8, 7): 504 cells, two 256-cell blocks of the gradient plan; (13, 11, 9): 1 287 cells.  face_out and
    div_out with and without vol against the restatement, and against three mi_flux_div calls on the engine"""
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    M = mesh(dims)
    n, nI, lo, up = M["n"], M["nI"], M["lo"], M["up"]
    assert n == {(3, 2, 2): 12, (9, 8, 7): 504, (13, 11, 9): 1287}[dims]
    lam, sf, visc, g, V = _inputs(M, dims, dev)
    addr = eng.Addressing(ctx, n, lo, up)
    for with_vol in (True, False):
        rface, rdiv = expected(dims, kind, with_vol)
        face, div = _run(eng, addr, kind, lam, sf, visc, g, V if with_vol else None, E, host)
        for j in range(3):
            assert np.array_equal(face[j], rface[j]), (with_vol, j)
            assert np.array_equal(div[j], rdiv[j]), (with_vol, j)
        # today's composition: element-wise glue for X, then mi_flux_div(cell_scale = visc) per component
        tr = (g[0] + g[4]) + g[8]
        ii = COEFF[kind] * tr
        x = [g[i] - ii if i % 4 == 0 else g[i] for i in range(9)]
        A = eng.Assembly(addr)
        for j in range(3):
            phi, d = E(nI), E(n)
            A.flux_div(lam, sf, [x[j], x[3 + j], x[6 + j]], phi, d, cell_scale=visc, vol=V if with_vol else None)
            assert np.array_equal(host(phi), face[j]) and np.array_equal(host(d), div[j]), (with_vol, j)
    assert torch.cuda.is_available()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(9, 8, 7), (13, 11, 9)])
@pytest.mark.parametrize("mode", ROW_MODES)
def test_engine_every_row_plan_gives_the_bits_of_the_default(pkg, monkeypatch, dims, mode):
    """gradient-plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, and the unstaged fall-back (MI_ROW_CAP=64): the
    bits of the default plan, which are the restatement's"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    M = mesh(dims)
    n, lo, up = M["n"], M["lo"], M["up"]
    lam, sf, visc, g, V = _inputs(M, dims, dev)
    default = {(k, v): _run(eng, eng.Addressing(ctx, n, lo, up), k, lam, sf, visc, g, V if v else None, E, host) for k in ("dev", "dev2") for v in (True, False)}
    set_row_blocks(monkeypatch, mode, grad=True)                              # after the default plan's runs above
    if mode.startswith("fixed"):                                              # the 504 cells of (9, 8, 7) are ONE default tile, a numbering that is tile-contiguous
        monkeypatch.setenv("MI_TILE_CELLS", "256")                            # as it stands; tiles of 256 cells permute it, so the fixed blocks are taken
    addr = eng.Addressing(ctx, n, lo, up, ordered=mode.startswith("tiles"))
    assert bool(addr.is_ordered) == mode.startswith("tiles")
    for (kind, with_vol), (dface, ddiv) in default.items():
        face, div = _run(eng, addr, kind, lam, sf, visc, g, V if with_vol else None, E, host)
        rface, rdiv = expected(dims, kind, with_vol)
        for j in range(3):
            assert np.array_equal(face[j], dface[j]) and np.array_equal(div[j], ddiv[j]), (kind, with_vol, j)
            assert np.array_equal(face[j], rface[j]) and np.array_equal(div[j], rdiv[j]), (kind, with_vol, j)


@pytest.mark.gpu
@pytest.mark.parametrize("n_comp", [1, 3])
def test_engine_patch_gauss_grad_correct_bit_exact(pkg, n_comp):
    """the box's wall patch (and its inlet): a fixedValue snGrad, deltaCoeffs*(U_b - U_internal), and the zero one of zeroGradient"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    dims = (9, 8, 7)
    M = mesh(dims)
    n = M["n"]
    g, _ = fields(dims)
    g = g[:3 * n_comp]
    gd = [dev(a) for a in g]
    for name in ("walls", "inlet"):
        fc, s, mag, dc = patch_geometry(M, name)
        m = fc.shape[0]
        assert m == {"walls": 2 * (9 * 7 + 9 * 8), "inlet": 8 * 7}[name]
        P = eng.Patch(ctx, n, fc)
        u = [uniform(31 + j, n, -1.0, 1.0) for j in range(n_comp)]
        ub = [uniform(41 + j, m, -1.0, 1.0) for j in range(n_comp)]
        for sn in ([dc * (b - a[fc]) for a, b in zip(u, ub)], [np.zeros(m) for _ in range(n_comp)]):
            ref = gauss_grad_correct(fc, s, mag, sn, g)
            out = [E(m) for _ in range(3 * n_comp)]
            P.gauss_grad_correct([dev(a) for a in s], dev(mag), [dev(a) for a in sn], gd, out)
            for i in range(3 * n_comp):
                assert np.array_equal(host(out[i]), ref[i]), (name, i)
            if not np.any(sn[0]):                                             # zeroGradient: the normal part of the cell gradient is taken out
                nh = np.stack(s, 1) / mag[:, None]
                assert np.max(np.abs(np.sum(nh * np.stack(ref[:3], 1), 1))) < 1e-12
        P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dev", "dev2"])
def test_engine_patch_flux_wall_and_coupled_bit_exact(pkg, kind):
    """NULL weights: the wall patch from its own boundary values (the corrected boundary gradient, a boundary viscosity).  Weights given: the
    first min(64, nI) internal faces posed as a patch whose neighbour values are the upper cells' (weights off 0.5)"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    for dims in ((3, 2, 2), (9, 8, 7)):
        M = mesh(dims)
        n, nI, lo, up, G = M["n"], M["nI"], M["lo"], M["up"], M["G"]
        g, visc = fields(dims)
        gd, viscd = [dev(a) for a in g], dev(visc)
        # the wall
        fc, s, mag, dc = patch_geometry(M, "walls")
        m = fc.shape[0]
        sn = [dc * (uniform(51 + j, m, -1.0, 1.0) - uniform(61 + j, n, -1.0, 1.0)[fc]) for j in range(3)]
        gb = gauss_grad_correct(fc, s, mag, sn, g)
        vb = uniform(71, m, 0.5, 1.5)
        ref = patch_flux_boundary(kind, s, vb, gb)
        P = eng.Patch(ctx, n, fc)
        out = [E(m) for _ in range(3)]
        P.dev_tgrad_flux(kind, [dev(a) for a in s], dev(vb), [dev(a) for a in gb], out)
        for j in range(3):
            assert np.array_equal(host(out[j]), ref[j]), (dims, j)
        P.close()
        # the coupled patch
        m = min(64, nI)
        fc = lo[:m]
        s = [np.ascontiguousarray(G["Sf"][:m, k]) for k in range(3)]
        w = np.ascontiguousarray(G["weights"][:m])
        assert np.all(np.abs(w - 0.5) > 1e-6)
        nvisc, ng = visc[up[:m]], [a[up[:m]] for a in g]
        ref = patch_flux_coupled(kind, fc, s, w, visc, g, nvisc, ng)
        P = eng.Patch(ctx, n, fc)
        out = [E(m) for _ in range(3)]
        P.dev_tgrad_flux(kind, [dev(a) for a in s], viscd, gd, out, weights=dev(w), nbr_visc=dev(nvisc), nbr_grad=[dev(a) for a in ng])
        for j in range(3):
            assert np.array_equal(host(out[j]), ref[j]), (dims, j)
        # the same faces as internal faces: the contracted interpolate differs from the patch's by rounding only
        face, _ = expected(dims, kind, False)
        for j in range(3):
            assert np.max(np.abs(ref[j] - face[j][:m])) <= 64 * EPS * np.max(np.abs(face[j][:m]))
        P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dev", "dev2"])
def test_engine_whole_term_into_the_source(pkg, orc, kind):
    """(9, 8, 7): the internal sums, the patch fluxes added in patch order (corner cells carry two and three boundary faces, from two
    patches and twice from one), /V, then source += V*div (negated with mi_vec_axpby, mi_fvm_su) -- against the same walk in numpy"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    dims = (9, 8, 7)
    M = mesh(dims)
    n, nI, lo, up, G = M["n"], M["nI"], M["lo"], M["up"], M["G"]
    per_cell = np.bincount(M["owner"][nI:], minlength=n)
    assert per_cell.max() == 3 and np.sum(per_cell == 2) > 0 and np.sum(per_cell == 3) == 8
    g, visc = fields(dims)
    lam, sf, viscd, gd, V = _inputs(M, dims, dev)
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    face, div = [E(nI) for _ in range(3)], [E(n) for _ in range(3)]
    A.div_dev_tgrad(kind, lam, sf, viscd, gd, face, div, None)
    rface, rdiv = expected(dims, kind, False)
    rdiv = [a.copy() for a in rdiv]
    for ip, (name, _, cnt, start) in enumerate(M["patches"]):
        fc, s, mag, dc = patch_geometry(M, name)
        fixed = name != "outlet"                                              # inlet and walls fixedValue, the outlet zeroGradient
        sn = [dc * (uniform(100 + 10 * ip + j, cnt, -1.0, 1.0) - uniform(61 + j, n, -1.0, 1.0)[fc]) if fixed else np.zeros(cnt) for j in range(3)]
        vb = uniform(200 + ip, cnt, 0.5, 1.5)
        gb = gauss_grad_correct(fc, s, mag, sn, g)
        rpf = patch_flux_boundary(kind, s, vb, gb)
        P = eng.Patch(ctx, n, fc)
        sd = [dev(a) for a in s]
        gbd, pf = [E(cnt) for _ in range(9)], [E(cnt) for _ in range(3)]
        P.gauss_grad_correct(sd, dev(mag), [dev(a) for a in sn], gd, gbd)
        P.dev_tgrad_flux(kind, sd, dev(vb), gbd, pf)
        for j in range(3):
            assert np.array_equal(host(pf[j]), rpf[j]), (name, j)
            P.add(pf[j], div[j])
            rdiv[j] = orc.patch_add(fc, rpf[j], rdiv[j], 0)
        P.close()
    src0 = [uniform(300 + j, n, -1.0, 1.0) for j in range(3)]
    for j in range(3):
        eng._chk(eng.lib().mi_vec_div(ctx.h, C.c_int64(n), eng._ptr(div[j]), eng._ptr(V), eng._ptr(div[j])))
        rd = rdiv[j] / G["V"]
        assert np.array_equal(host(div[j]), rd), j
        src, neg = dev(src0[j]), E(n)
        A.axpby(-1.0, div[j], 0.0, div[j], neg)
        A.fvm_su(V, neg, src)
        assert np.array_equal(host(src), src0[j] + G["V"] * rd), j             # source += V*div, the product rounded, then the sum
        assert np.array_equal(host(src), orc.fvm_su(G["V"], -rd, src0[j])), j


@pytest.mark.gpu
def test_engine_refusals_launch_nothing_and_zero_faces_are_ok(pkg):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    dims = (3, 2, 2)
    M = mesh(dims)
    n, nI, lo, up, G = M["n"], M["nI"], M["lo"], M["up"], M["G"]
    g, visc = fields(dims)
    lam, sf, viscd, gd, V = _inputs(M, dims, dev)
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    face, div = [E(nI) for _ in range(3)], [E(n) for _ in range(3)]
    lam0 = host(lam).copy()

    def refused(*a):
        with pytest.raises(eng.MiError, match="mi_fvc_div_dev_tgrad"):
            A.div_dev_tgrad(*a)
        assert all(np.all(host(o) == -77.0) for o in face + div) and np.array_equal(host(lam), lam0)
    refused(2, lam, sf, viscd, gd, face, div, V)                              # a kind other than the two
    refused(-1, lam, sf, viscd, gd, face, div, V)
    refused("dev", None, sf, viscd, gd, face, div, V)                         # a missing array
    refused("dev", lam, [sf[0], None, sf[2]], viscd, gd, face, div, V)
    refused("dev", lam, sf, None, gd, face, div, V)
    refused("dev2", lam, sf, viscd, gd[:8] + [None], face, div, V)
    refused("dev", lam, sf, viscd, gd, [face[0], None, face[2]], div, V)
    refused("dev", lam, sf, viscd, gd, face, div[:2] + [None], V)
    refused("dev", lam, sf, viscd, gd, [lam] + face[1:], div, V)              # an output aliases an input
    refused("dev", lam, sf, viscd, gd, face, [viscd] + div[1:], V)
    refused("dev", lam, sf, viscd, gd, face, [gd[4]] + div[1:], V)
    refused("dev2", lam, sf, viscd, gd, face, div[:2] + [V], V)
    refused("dev", lam, sf, viscd, gd, [face[0], face[0], face[2]], div, V)   # ... or another output
    refused("dev", lam, sf, viscd, gd, face, [div[0], div[1], div[0]], None)
    # the patch entries
    fc, s, mag, dc = patch_geometry(M, "walls")
    m = fc.shape[0]
    P = eng.Patch(ctx, n, fc)
    sd, magd = [dev(a) for a in s], dev(mag)
    sn, gb, pf = [dev(np.zeros(m)) for _ in range(3)], [E(m) for _ in range(9)], [E(m) for _ in range(3)]
    vb, w = dev(uniform(71, m, 0.5, 1.5)), dev(uniform(72, m, 0.3, 0.7))
    nb = [dev(a[fc]) for a in g]
    for bad in ((sd, magd, sn[:2], gd[:6], gb[:6]), (sd, None, sn, gd, gb), (sd, magd, sn, gd[:8] + [None], gb), (sd, magd, sn, gd, gb[:8] + [gb[0]]),
                (sd, magd, sn, gd, [magd] + gb[1:]), (sd, magd, [sn[0], None, sn[2]], gd, gb)):
        with pytest.raises(eng.MiError, match="mi_patch_gauss_grad_correct"):
            P.gauss_grad_correct(*bad)
        assert all(np.all(host(o) == -77.0) for o in gb)
    for bad in ((2, sd, vb, nb, pf), ("dev", sd, None, nb, pf), ("dev", sd, vb, nb[:8] + [None], pf), ("dev", sd, vb, nb, [pf[0], pf[0], pf[2]]),
                ("dev", sd, vb, nb, [vb] + pf[1:]), ("dev2", sd, viscd, gd, pf, w, None, nb), ("dev2", sd, viscd, gd, pf, w, vb, None),
                ("dev2", sd, viscd, gd, [w] + pf[1:], w, vb, nb)):
        with pytest.raises(eng.MiError, match="mi_patch_dev_tgrad_flux"):
            P.dev_tgrad_flux(*bad)
        assert all(np.all(host(o) == -77.0) for o in pf)
    P.close()
    # an empty patch: MI_OK, nothing to write
    P0 = eng.Patch(ctx, n, np.zeros(0, np.int32))
    none3, none9 = [None] * 3, [None] * 9
    P0.gauss_grad_correct(none3, None, none3, gd, none9)
    P0.dev_tgrad_flux("dev", none3, None, none9, none3)
    P0.close()
    # zero faces with cells present: MI_OK without a launch, the div arrays are zero
    nc = 5
    A0 = eng.Assembly(eng.Addressing(ctx, nc, np.zeros(0, np.int32), np.zeros(0, np.int32)))
    div0 = [E(nc) for _ in range(3)]
    A0.div_dev_tgrad("dev2", None, none3, dev(visc[:nc]), [dev(a[:nc]) for a in g], none3, div0, dev(G["V"][:nc]))
    assert all(np.all(host(o) == 0.0) for o in div0)
