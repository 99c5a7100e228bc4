"""`Gauss cubic`: the explicit correction of the centred fourth-order scheme (schemes/cubic/cubic.H:111-184, the two-weight interpolate of
surfaceInterpolationScheme.C:159-166,250-265) that gaussConvectionScheme::fvmDiv integrates into the source (gaussConvectionScheme.C:109-112).
The restatements of tests/filtered_support.py on hand-computed faces (CPU), then mi_cubic_correction / mi_patch_cubic_correction and the
unfused route into the matrix against the numpy restatement, bit for bit on every face (gpu).  Restated from the header, not pinned by
compiled reference functors."""
import numpy as np
import pytest

import filtered_support as fs
import test_limited_schemes as tl
from assembly_support import gpu_env, same, set_face_grid, set_row_tables, signed_flux


def _fields(pkg, n, n_rhs, seed):
    """-> (vf, grads): n_rhs cell fields and one [gx, gy, gz] each"""
    u = pkg.synthetic.splitmix_uniform
    return [u(seed + r, n) * 1.6 - 0.5 for r in range(n_rhs)], [[4.0 * (u(seed + 10 + 3 * r + k, n) - 0.5) for k in range(3)] for r in range(n_rhs)]


def _mesh(pkg, name):
    from conftest import random_graph_case
    return tl._graded_box(pkg, (9, 8, 7))[0] if name == "box" else random_graph_case(pkg, 600, extra=3.0, seed=13)


def _geo_dev(eng, dev, geo):
    return eng.cubic_geometry(dev(geo["lam"]), [dev(x) for x in geo["sf"]], dev(geo["mag_sf"]), dev(geo["dc"]))


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------
def test_restatement_semantics():
    # lambda = 0.5: kSc = 0.5*(1 - 0.5*(3 - 1)) = 0, kVecP = 0.25*0.5, kVecN = 0.25*(-0.5)
    assert fs.cubic_coeffs(np.array([0.5])) == (0.0, 0.125, -0.125)
    # ... so the field itself drops out and the correction is (gP - gN)/8 & Sf / magSf / deltaCoeffs
    sf = [2.0, 0.0, 0.0]
    assert fs.cubic_face(0.5, 7.0, -3.0, [1.0, 5.0, 5.0], [0.5, -5.0, 9.0], sf, 2.0, 4.0) == (0.5 / 8) / 4.0
    assert fs.cubic_face(0.5, 7.0, -3.0, [1.0, 5.0, 5.0], [0.5, -5.0, 9.0], sf, 2.0, 4.0, flux=-3.0) == -3.0 * ((0.5 / 8) / 4.0)
    # lambda = 0.25: kSc = 0.25*(1 - 0.25*2.5) = 0.09375, kVecP = 0.5625*0.25, kVecN = 0.0625*(-0.75): all exact
    kSc, kP, kN = (float(x[0]) for x in fs.cubic_coeffs(np.array([0.25])))
    assert (kSc, kP, kN) == (0.09375, 0.140625, -0.046875)
    assert fs.cubic_face(0.25, 2.0, 1.0, [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], 1.0, 1.0) == 0.09375 + (0.140625 - 0.046875)
    # the numpy restatement and the scalar one, every face of a seeded set
    m = 64
    u = lambda s: np.random.default_rng(s).random(m)
    geo = dict(lam=0.3 + 0.4 * u(1), sf=[u(2) - 0.5, u(3) - 0.5, u(4) - 0.5], mag_sf=0.1 + u(5), dc=0.5 + u(6))
    lo, up = np.arange(m), (np.arange(m) + 1) % m
    vf, g, flux = [u(7) - 0.5], [[u(8) - 0.5, u(9) - 0.5, u(10) - 0.5]], u(11) - 0.5
    for fl in (None, flux):
        got = fs.cubic_internal(lo, up, geo, vf, g, fl)[0]
        for f in range(m):
            P, N = lo[f], up[f]
            want = fs.cubic_face(geo["lam"][f], vf[0][P], vf[0][N], [x[P] for x in g[0]], [x[N] for x in g[0]], [x[f] for x in geo["sf"]],
                                 geo["mag_sf"][f], geo["dc"][f], None if fl is None else fl[f])
            assert got[f] == want, f


def test_linear_plus_correction_reconstructs_a_cubic_on_a_uniform_chain():
    """vf = x^3 with its exact gradient on a uniform 1-D chain: linear interpolate + correction is the face value (the Hermite cubic through
    two values and two slopes is exact for a cubic).  The only check here that is not bit for bit: each of the dozen operations behind a
    face value of magnitude <= 1 rounds by at most half an ulp of a number <= 1 (3*x^2*h/8 < 1 too), so 16 ulp of 1 bounds the sum."""
    m = 40
    h = 1.0 / m
    x = (np.arange(m) + 0.5) * h
    lo, up = np.arange(m - 1), np.arange(1, m)
    xf = (np.arange(m - 1) + 1.0) * h
    area = 0.37
    geo = dict(lam=np.full(m - 1, 0.5), sf=[np.full(m - 1, area), np.zeros(m - 1), np.zeros(m - 1)], mag_sf=np.full(m - 1, area),
               dc=np.full(m - 1, 1.0 / h))
    vf, grad = x ** 3, [3 * x * x, np.zeros(m), np.zeros(m)]
    corr = fs.cubic_internal(lo, up, geo, [vf], [grad])[0]
    linear = 0.5 * vf[lo] + 0.5 * vf[up]
    assert np.max(np.abs(linear + corr - xf ** 3)) <= 16 * np.finfo(float).eps
    assert np.max(np.abs(linear - xf ** 3)) > 1e-4                   # and the correction is what closes the gap


def test_library_exports_the_entry_points(pkg):
    for name in ("mi_cubic_correction", "mi_patch_cubic_correction"):
        assert hasattr(pkg.engine.lib(), name) and name in pkg.engine.SYMBOLS, name


def test_mirror_exports_the_cubic_correction(pkg):
    import os
    import subprocess
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert syms.count("Foam::fvc::cubicCorrectionFlux(") == 2


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "graph", "box_noxcd"])
def test_face_pass_against_the_restatement(pkg, monkeypatch, name):
    if name.endswith("_noxcd"):
        set_row_tables(monkeypatch, "noxcd"); name = name[:-len("_noxcd")]
    eng, ctx, dev, host, E = gpu_env(pkg)
    case = _mesh(pkg, name)
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    geo = fs.cubic_geometry(pkg, nf, 40)
    gd = _geo_dev(eng, dev, geo)
    flux = signed_flux(pkg.synthetic.splitmix_uniform(7, nf))
    fd = dev(flux)
    for n_rhs in (1, 3, 4):
        vf, g = _fields(pkg, n, n_rhs, 60 + 20 * n_rhs)
        vd, gdv = [dev(x) for x in vf], [[dev(x) for x in gr] for gr in g]
        for fl, fl_dev in ((flux, fd), (None, None)):
            out = [E(nf) for _ in range(n_rhs)]
            A.cubic_correction(gd, vd, gdv, out, face_flux=fl_dev)
            ref = fs.cubic_internal(lo, up, geo, vf, g, fl)
            for r in range(n_rhs):
                assert same(host(out[r]), ref[r]), (n_rhs, fl is None, r)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 3])
def test_the_loop_walk_under_a_forced_grid(pkg, monkeypatch, grid):
    set_face_grid(monkeypatch, grid)
    eng, ctx, dev, host, E = gpu_env(pkg)
    case = _mesh(pkg, "box")
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    assert nf > grid * 256
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    geo = fs.cubic_geometry(pkg, nf, 40)
    flux = signed_flux(pkg.synthetic.splitmix_uniform(7, nf))
    vf, g = _fields(pkg, n, 3, 120)
    out = [E(nf) for _ in range(3)]
    A.cubic_correction(_geo_dev(eng, dev, geo), [dev(x) for x in vf], [[dev(x) for x in gr] for gr in g], out, face_flux=dev(flux))
    ref = fs.cubic_internal(lo, up, geo, vf, g, flux)
    for r in range(3):
        assert same(host(out[r]), ref[r]), r


@pytest.mark.gpu
def test_zero_faces_one_face_and_refusals(pkg):
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg, fill=7.0)
    i32 = lambda *a: np.array(a, dtype=np.int32)
    # no face: nothing to do, nothing read
    A0 = eng.Assembly(eng.Addressing(ctx, 3, i32(), i32()))
    A0.cubic_correction(eng.CubicGeometry(), [dev(np.ones(3))], [[dev(np.ones(3))] * 3], [E(0)])
    # one face
    A1 = eng.Assembly(eng.Addressing(ctx, 2, i32(0), i32(1)))
    geo = fs.cubic_geometry(pkg, 1, 5)
    vf, g = _fields(pkg, 2, 1, 9)
    out = [E(1)]
    A1.cubic_correction(_geo_dev(eng, dev, geo), [dev(vf[0])], [[dev(x) for x in g[0]]], out, face_flux=dev(np.array([-0.75])))
    assert same(host(out[0]), fs.cubic_internal(i32(0), i32(1), geo, vf, g, np.array([-0.75]))[0])
    # refusals
    case = pkg.synthetic.box_case(6, 5, 4)
    n, nf = case.n_cells, case.n_faces
    A = eng.Assembly(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr))
    geo = fs.cubic_geometry(pkg, nf, 11)
    lam, sf, msf, dc = dev(geo["lam"]), [dev(x) for x in geo["sf"]], dev(geo["mag_sf"]), dev(geo["dc"])
    G = eng.cubic_geometry(lam, sf, msf, dc)
    vf, g = _fields(pkg, n, 4, 13)
    vd, gdv = [dev(x) for x in vf], [[dev(x) for x in gr] for gr in g]
    fd = dev(signed_flux(pkg.synthetic.splitmix_uniform(7, nf)))
    outs = [E(nf) for _ in range(5)]
    call = lambda **kw: A.cubic_correction(kw.get("geo", G), kw.get("vf", vd[:3]), kw.get("grad", gdv[:3]), kw.get("out", outs[:3]), face_flux=kw.get("flux", fd))
    with pytest.raises(eng.MiError, match="1 to 4"):
        call(vf=vd + [vd[0]], grad=gdv + [gdv[0]], out=outs)               # n_rhs = 5
    with pytest.raises(eng.MiError, match="1 to 4"):
        call(out=[])
    with pytest.raises(eng.MiError, match="alias"):
        call(out=[outs[0], fd, outs[2]])
    with pytest.raises(eng.MiError, match="alias"):
        call(out=[lam, outs[1], outs[2]])
    with pytest.raises(eng.MiError, match="alias"):
        call(out=[outs[0], outs[1], vd[1]])
    with pytest.raises(eng.MiError, match="alias"):
        call(out=[outs[0], gdv[2][1], outs[2]])
    with pytest.raises(eng.MiError, match="differ"):
        call(out=[outs[0], outs[1], outs[0]])
    with pytest.raises(eng.MiError, match="null output"):
        call(out=[outs[0], None, outs[2]])
    with pytest.raises(eng.MiError, match="missing"):
        call(geo=eng.cubic_geometry(lam, sf, None, dc))
    with pytest.raises(eng.MiError, match="missing"):
        call(grad=[gdv[0], [gdv[1][0], None, gdv[1][2]], gdv[2]])
    with pytest.raises(eng.MiError, match="missing"):
        call(vf=[vd[0], vd[1], None])
    with pytest.raises(eng.MiError, match="aligned"):
        call(flux=E(nf + 1)[1:])
    with pytest.raises(eng.MiError, match="aligned"):
        call(geo=eng.cubic_geometry(E(nf + 1)[1:], sf, msf, dc))
    P = eng.Patch(ctx, n, np.arange(5, dtype=np.int32))
    p5 = lambda: dev(np.ones(5))
    PG = eng.cubic_geometry(p5(), [p5(), p5(), p5()], p5(), p5())
    po = [E(5), E(5)]
    nv, ng = [p5(), p5()], [[p5(), p5(), p5()] for _ in range(2)]
    with pytest.raises(eng.MiError, match="alias"):
        P.cubic_correction(PG, vd[:2], nv, gdv[:2], ng, [po[0], nv[1]])
    with pytest.raises(eng.MiError, match="alias"):
        P.cubic_correction(PG, vd[:2], nv, gdv[:2], ng, [ng[1][2], po[1]])
    with pytest.raises(eng.MiError, match="1 to 4"):
        P.cubic_correction(PG, vd + vd[:1], nv, gdv, ng, [E(5) for _ in range(5)])
    with pytest.raises(eng.MiError, match="missing"):
        P.cubic_correction(PG, vd[:2], [nv[0], None], gdv[:2], ng, po)
    P.close()
    torch.cuda.synchronize()
    for t in outs + po:
        assert torch.all(t == 7.0)                                      # nothing was launched
    assert torch.all(nv[1] == 1.0) and torch.all(ng[1][2] == 1.0)


@pytest.mark.gpu
def test_cyclic_patch_against_the_restatement(pkg):
    """the 12x7x6 cyclic channel (x-min <-> x-max): the neighbour fields from mi_matrix_patch_neighbour_field"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    case = syn.box_case(12, 7, 6)
    n = case.n_cells
    cyc = syn.add_cyclic_x(case)
    fcs = [i.face_cells for i in cyc.interfaces]
    nbrs = [cyc.interfaces[i.nbr_patch].face_cells for i in cyc.interfaces]
    mat = eng.Matrix(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr, fcs, nbrs))
    npf = [len(f) for f in fcs]
    off = [0, npf[0]]
    vf, g = _fields(pkg, n, 4, 200)
    vd, gdv = [dev(x) for x in vf], [[dev(x) for x in gr] for gr in g]
    nvd, ngd = [E(sum(npf)) for _ in range(4)], [[E(sum(npf)) for _ in range(3)] for _ in range(4)]
    for r in range(4):
        mat.patch_neighbour_field(vd[r], nvd[r])
        for k in range(3):
            mat.patch_neighbour_field(gdv[r][k], ngd[r][k])
    assert same(host(nvd[0]), np.concatenate([vf[0][q] for q in nbrs]))
    for p in range(2):
        P = eng.Patch(ctx, n, fcs[p])
        m = npf[p]
        sl = lambda a: a[off[p]:off[p] + m]
        geo = fs.cubic_geometry(pkg, m, 300 + 10 * p)
        pflux = signed_flux(syn.splitmix_uniform(80 + p, m))
        for n_rhs in (1, 3, 4):
            for fl in (pflux, None):
                out = [E(m) for _ in range(n_rhs)]
                P.cubic_correction(_geo_dev(eng, dev, geo), vd[:n_rhs], [sl(x).contiguous() for x in nvd[:n_rhs]], gdv[:n_rhs],
                                   [[sl(x).contiguous() for x in row] for row in ngd[:n_rhs]], out, patch_flux=None if fl is None else dev(fl))
                ref = fs.cubic_patch(fcs[p], geo, vf[:n_rhs], [host(sl(x)) for x in nvd[:n_rhs]], g[:n_rhs],
                                     [[host(sl(x)) for x in row] for row in ngd[:n_rhs]], fl)
                for r in range(n_rhs):
                    assert same(host(out[r]), ref[r]), (p, n_rhs, fl is None, r)
        P.close()


@pytest.mark.gpu
def test_fvm_div_under_gauss_cubic_end_to_end(pkg, orc):
    """fvm::div(phi, T) under `Gauss cubic` on the graded box by the unfused route: mi_gauss_grad of T (Gauss linear), mi_fvm_div with the
    linear weights, the correction face field, mi_surface_integrate, source -= V*ivf.  lower / upper / diag are those of the linear
    scheme; the source is the restatement's (on the gradient the device formed)"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    u = pkg.synthetic.splitmix_uniform
    case = _mesh(pkg, "box")
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    geo = fs.cubic_geometry(pkg, nf, 500)
    V, T, src0 = 0.5 + u(510, n), u(511, n) * 1.6 - 0.5, u(512, n) - 0.5
    flux = signed_flux(u(513, nf))
    lam, sf, Vd, Td, fd = dev(geo["lam"]), [dev(x) for x in geo["sf"]], dev(V), dev(T), dev(flux)
    # grad(T), Gauss linear
    Tf, grad = E(nf), [E(n) for _ in range(3)]
    A.face_interpolate(lam, Td, Tf)
    A.gauss_grad(sf, Tf, Vd, grad)
    gh = [host(x) for x in grad]
    assert all(np.all(np.isfinite(x)) and np.any(x != 0) for x in gh)
    # the matrix of the linear scheme
    lower, upper, diag = E(nf), E(nf), E(n)
    A.fvm_div(lam, fd, lower, upper, diag)
    rl, ru, rd = orc.fvm_div(n, lo, up, geo["lam"], flux)
    assert same(host(lower), rl) and same(host(upper), ru) and same(host(diag), rd)
    # the correction into the source
    t, ivf, s = [E(nf)], E(n), dev(src0)
    A.cubic_correction(eng.cubic_geometry(lam, sf, dev(geo["mag_sf"]), dev(geo["dc"])), [Td], [grad], t, face_flux=fd)
    rt = fs.cubic_internal(lo, up, geo, [T], [gh], flux)[0]
    assert same(host(t[0]), rt)
    A.surface_integrate(t[0], Vd, ivf)
    rivf = orc.surface_integrate(n, lo, up, rt, V)
    assert same(host(ivf), rivf)
    A.submul(Vd, ivf, s)
    assert same(host(s), src0 - V * rivf)
    assert np.max(np.abs(host(s) - src0)) > 1e-3                        # the correction is not a no-op
