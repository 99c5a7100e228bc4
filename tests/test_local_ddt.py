"""`ddtSchemes { default steadyState | localEuler <rDeltaT> | CoEuler <phi> <rho> <maxCo>; }`: the parser, fvm::ddt, fvc::ddt, fvc::ddtCorr with a
per-cell rDeltaT, CoEuler's rDeltaT field in one row pass, and the fused assembly with the local time derivative
(steadyStateDdtScheme.C; localEulerDdtScheme.C:149-264, 339-445, 531-560; CoEulerDdtScheme.C:61-167; static mesh).

The expected values are a numpy restatement of the reference's field expressions written here: numpy evaluates one operator per pass and
rounds each, exactly as the reference's gpuField operators do (tests/test_backward_ddt.py), so every comparison with the engine is bit for
bit.  CPU: the parser through the C ABI, the exports, what the restated CoEuler field promises.  GPU: the streaming and face entries,
mi_co_r_delta_t in every block shape of the row pass, mi_fvm_assemble_local against the engine's own unfused sequence and against the
restatement.  The bounded convection scheme and the steady assembly: tests/test_bounded_steady.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from assembly_support import (OTHER_TABLES, ROW_MODES, SHAPES, VARIANTS, FusedCase, co_face, gpu_env, set_row_blocks, set_row_tables, shape_case,
                              shaped_addressing, signed_flux)

NEW_ENTRIES = ("mi_ddt_local_parse", "mi_fvm_ddt_local", "mi_fvc_ddt_local", "mi_ddt_phi_corr_local", "mi_co_face_r_delta_t", "mi_co_r_delta_t",
               "mi_patch_max", "mi_fvm_assemble_local")
SENTINEL = -7.25


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def fvm_ddt(r, V, p0, rho_value=None, rho=None, rho0=None):
    """-> (diag, source) of fvmDdt (localEulerDdtScheme.C:339-445): no density, constant density, density field"""
    if rho is not None:
        return (r * rho) * V, ((r * rho0) * p0) * V
    if rho_value is not None:
        return (r * rho_value) * V, ((r * rho_value) * p0) * V
    return r * V, (r * p0) * V


def fvc_ddt(r, f, f0, rho_value=None, rho=None, rho0=None):
    """fvcDdt (:149-157 no density, :200-209 constant, :255-264 field)"""
    if rho is not None:
        return r * ((rho * f) - (rho0 * f0))
    if rho_value is not None:
        return (r * rho_value) * (f - f0)
    return r * (f - f0)


def ddt_corr(orc, n, lo, up, r, lam, Sf, U0, phi0):
    """fvcDdtPhiCorr(U, phi) (:531-560): Euler's expression with rDeltaT := fvc::interpolate(r), one fma per face -> (out, coefficient)"""
    fU = orc.flux_div(n, lo, up, lam, Sf, U0, want_div=False)
    phi_corr = phi0 - fU
    k = 1 - np.minimum(np.abs(phi_corr) / (np.abs(phi0) + 1e-15), 1.0)
    rf = orc.face_interpolate(lo, up, lam, r)
    return (k * rf) * phi_corr, k


def co_cells(n, lo, up, x, patches=()):
    """CorDeltaT (:61-121): the maximum, from 0.0, over own faces, neighbour-side faces, then every patch's faces (all positive: any order)"""
    r = np.zeros(n)
    np.maximum.at(r, lo, x)
    np.maximum.at(r, up, x)
    for fc, xp in patches:
        np.maximum.at(r, fc, xp)
    return r


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported(pkg):
    eng = pkg.engine
    for name in NEW_ENTRIES:
        assert name in eng.SYMBOLS and hasattr(eng.lib(), name), name


def test_parser_accepts_and_refuses(pkg):
    eng = pkg.engine
    P = eng.ddt_local_parse
    assert P("steadyState") == dict(kind="steadyState") and P(" \t steadyState\n") == dict(kind="steadyState")
    assert P("localEuler rDeltaT") == dict(kind="localEuler", r_delta_t="rDeltaT")
    assert P("  localEuler\t\n rSubDeltaT  ") == dict(kind="localEuler", r_delta_t="rSubDeltaT")
    assert P("CoEuler phi rho 0.5") == dict(kind="CoEuler", phi="phi", rho="rho", max_co=0.5)
    assert P("\tCoEuler   phiv\nrho0 \t 1e-1 ") == dict(kind="CoEuler", phi="phiv", rho="rho0", max_co=0.1)
    refused = [("localEuler", "localEuler"), ("CoEuler", "CoEuler"), ("CoEuler phi", "phi"), ("CoEuler phi rho", "rho"),     # a missing word
               ("steadyState now", "now"), ("localEuler rDeltaT more", "more"), ("CoEuler phi rho 0.5 again", "again"),      # an extra word
               ("CoEuler phi rho fast", "fast"), ("CoEuler phi rho 0.5x", "0.5x"), ("CoEuler phi rho nan", "nan"),           # not a number
               ("CoEuler phi rho inf", "inf"), ("CoEuler phi rho 0", "0"), ("CoEuler phi rho -0.5", "-0.5"),                 # not finite, not > 0
               ("Euler", "not a local scheme"), ("backward", "not a local scheme"), ("CrankNicolson 0.9", "not a local scheme"),
               ("Euler", "Euler"), ("backward", "backward"), ("CrankNicolson 0.9", "CrankNicolson"),
               ("SLTS phi rho 1", "SLTS"), ("localEuler " + "x" * 64, "x" * 64), ("", "empty"), ("  \n\t", "empty"), (None, "NULL")]
    for text, token in refused:
        with pytest.raises(eng.MiError) as e:
            P(text)
        assert token in str(e.value), (text, str(e.value))
    lib, out = eng.lib(), eng.DdtLocalScheme()
    assert lib.mi_ddt_local_parse(b"steadyState", None) != 0 and lib.mi_ddt_local_parse(None, C.byref(out)) != 0
    out.kind = 77
    assert lib.mi_ddt_local_parse(b"CoEuler phi rho", C.byref(out)) != 0 and out.kind == 77          # a refused call writes nothing
    assert lib.mi_ddt_local_parse(b"localEuler " + b"y" * 63, C.byref(out)) == 0 and out.kind == 1 and out.name == b"y" * 63


def small_box_co(pkg, nx=7, ny=6, nz=5):
    """a uniform box under a swirling velocity: deltaCoeffs 1/h, magSf h*h, phi = U_f & Sf with |U| between 0 and ~2.5"""
    case = pkg.synthetic.box_case(nx, ny, nz)
    lo, up, n = case.lower_addr, case.upper_addr, case.n_cells
    h = 1.0 / nx
    d = up - lo                                                    # 1: an x face, nx: a y face, nx*ny: a z face
    cx, cy, cz = (lo % nx + 0.5) * h, ((lo // nx) % ny + 0.5) * h, (lo // (nx * ny) + 0.5) * h
    vel = np.where(d == 1, 2.5 * np.sin(5 * cy) * cz, np.where(d == nx, 2.5 * cx * cx, 0.3 * np.cos(7 * cx + cy)))
    return n, lo, up, np.full(lo.shape[0], 1.0 / h), np.full(lo.shape[0], h * h), vel * (h * h)


def test_restated_co_euler_field_keeps_its_promises(pkg):
    """rDeltaT >= 1/deltaT everywhere; == 1/deltaT exactly where every face of the cell has Co <= maxCo; and the face Courant number formed
    with the resulting local step is <= maxCo up to the five roundings of the expression (|phi|/magSf, *deltaCoeffs, *deltaT, /maxCo,
    /deltaT: each within a factor (1 - 2^-53) of exact) -- an exact rational bound, no tolerance"""
    n, lo, up, dc, mag_sf, phi = small_box_co(pkg)
    dt, max_co = 0.05, 0.5
    x = co_face(dc, phi, mag_sf, dt, max_co)
    r = co_cells(n, lo, up, x)
    co = (dc * (np.abs(phi) / mag_sf)) * dt
    over = co > max_co
    hot = np.zeros(n, bool); hot[lo[over]] = True; hot[up[over]] = True
    assert np.all(r >= 1.0 / dt) and np.all(r[~hot] == 1.0 / dt) and np.all(r[hot] > 1.0 / dt)
    assert 0.25 * n <= hot.sum() <= 0.75 * n
    slack = (1 - Fraction(1, 2 ** 53)) ** 5
    for f in range(lo.shape[0]):
        exact = Fraction(float(dc[f])) * Fraction(float(abs(phi[f]))) / Fraction(float(mag_sf[f]))
        for c in (lo[f], up[f]):
            assert exact / Fraction(float(r[c])) * slack <= Fraction(max_co), (f, c)
    # a mass flux: the interpolated old density divides the flux
    rho_f = 0.5 + 0.1 * np.arange(lo.shape[0]) / lo.shape[0]
    xm = co_face(dc, phi, mag_sf, dt, max_co, rho_f=rho_f)
    assert np.all(xm >= x) and np.any(xm > x)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streaming_entries_against_the_restatement(pkg):
    """mi_fvm_ddt_local / mi_fvc_ddt_local on the 31x23x19 box (an odd count: the unpaired element of the double2 loop), the three density forms;
    the refusals, with sentinel-filled outputs (nothing launched); zero cells"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=SENTINEL)
    u = pkg.synthetic.splitmix_uniform
    case = pkg.synthetic.box_case(31, 23, 19)
    n = case.n_cells
    assert n % 2 == 1
    asm = eng.Assembly(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr))
    V, p, p0, r = 0.5 + u(1, n), u(2, n) - 0.5, u(3, n) - 0.5, 50.0 + 400.0 * u(4, n)
    rho, rho0 = 0.9 + u(5, n), 0.8 + u(6, n)
    d, s, o = E(n), E(n), E(n)
    for form in ("none", "constant", "field"):
        kw = dict(constant=dict(rho_value=1.3), field=dict(rho=rho, rho0=rho0)).get(form, {})
        ekw = dict(constant=dict(rho_value=1.3), field=dict(rho=dev(rho), rho_old=dev(rho0))).get(form, {})
        asm.fvm_ddt_local(dev(r), dev(V), dev(p0), d, s, **ekw)
        rd, rs = fvm_ddt(r, V, p0, **kw)
        assert np.array_equal(host(d), rd) and np.array_equal(host(s), rs), form
        asm.fvc_ddt_local(dev(r), dev(p), dev(p0), o, **ekw)
        assert np.array_equal(host(o), fvc_ddt(r, p, p0, **kw)), form
    # a constant rDeltaT field is the Euler scheme, bit for bit
    asm.fvm_ddt_local(dev(np.full(n, 250.0)), dev(V), dev(p0), d, s, rho_value=1.3)
    d2, s2 = E(n), E(n)
    asm.fvm_ddt_euler(250.0, 1.3, dev(V), dev(p0), d2, s2)
    assert np.array_equal(host(d), host(d2)) and np.array_equal(host(s), host(s2))
    # refusals: an output among the inputs, the two outputs the same array, a missing array, one density array of two
    rD, Vd, pd, p0d, rhod = dev(r), dev(V), dev(p), dev(p0), dev(rho)
    d, s, o = E(n), E(n), E(n)
    for bad in (lambda: asm.fvm_ddt_local(rD, Vd, p0d, rD, s), lambda: asm.fvm_ddt_local(rD, Vd, p0d, d, Vd), lambda: asm.fvm_ddt_local(rD, Vd, p0d, d, d),
                lambda: asm.fvm_ddt_local(None, Vd, p0d, d, s), lambda: asm.fvm_ddt_local(rD, Vd, p0d, d, s, rho=rhod),
                lambda: asm.fvm_ddt_local(rD, Vd, p0d, d, s, rho=rhod, rho_old=d), lambda: asm.fvc_ddt_local(rD, pd, p0d, rD),
                lambda: asm.fvc_ddt_local(rD, pd, p0d, pd), lambda: asm.fvc_ddt_local(None, pd, p0d, o), lambda: asm.fvc_ddt_local(rD, pd, p0d, o, rho_old=rhod)):
        with pytest.raises(eng.MiError):
            bad()
    for t in (d, s, o):
        assert np.all(host(t) == SENTINEL)
    # zero cells: accepted, nothing written
    lib = eng.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.mi_fvm_ddt_local(ctx.h, C.c_int64(0), ptr(rD), C.c_double(1.0), None, None, ptr(Vd), ptr(p0d), ptr(d), ptr(s)) == 0
    assert lib.mi_fvc_ddt_local(ctx.h, C.c_int64(0), ptr(rD), C.c_double(1.0), None, None, ptr(pd), ptr(p0d), ptr(o)) == 0
    assert lib.mi_co_face_r_delta_t(ctx.h, C.c_int64(0), ptr(rD), ptr(Vd), ptr(pd), None, C.c_double(0.01), C.c_double(0.5), ptr(o)) == 0
    for t in (d, s, o):
        assert np.all(host(t) == SENTINEL)


@pytest.mark.gpu
def test_face_entries_against_the_restatement(pkg, orc):
    """mi_ddt_phi_corr_local on the 31x23x19 box: faces with phi0 == 0.0 (coefficient 0) and faces whose phi0 equals flux(U0) bit for bit
    (coefficient 1); a constant rDeltaT field gives mi_ddt_phi_corr's bits.  mi_co_face_r_delta_t, both flux forms.  Their refusals"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=SENTINEL)
    u = pkg.synthetic.splitmix_uniform
    case = pkg.synthetic.box_case(31, 23, 19)
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    asm = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    lam = 0.001 + 0.998 * u(9, nf)
    Sf, U0 = [u(10 + k, nf) - 0.5 for k in range(3)], [u(13 + k, n) - 0.5 for k in range(3)]
    r = 50.0 + 400.0 * u(4, n)
    fU = orc.flux_div(n, lo, up, lam, Sf, U0, want_div=False)
    phi0 = fU + 0.05 * (u(22, nf) - 0.5)
    phi0[::5] = 0.0
    phi0[2::7] = fU[2::7]
    ref, k = ddt_corr(orc, n, lo, up, r, lam, Sf, U0, phi0)
    assert np.any(k == 0.0) and np.any(k == 1.0) and np.any((k > 0.05) & (k < 0.95))
    lamd, Sfd, U0d, phid, out = dev(lam), [dev(x) for x in Sf], [dev(x) for x in U0], dev(phi0), E(nf)
    asm.ddt_phi_corr_local(dev(r), lamd, Sfd, U0d, phid, out)
    assert np.array_equal(host(out), ref)
    out2 = E(nf)
    asm.ddt_phi_corr_local(dev(np.full(n, 250.0)), lamd, Sfd, U0d, phid, out)
    asm.ddt_phi_corr(250.0, lamd, Sfd, U0d, None, phid, out2)
    assert np.array_equal(host(out), host(out2))
    # the face rDeltaT of CoEuler as a streaming pass: an odd count, both flux forms
    m = 1027
    dc, mag_sf, phi, rho_f = 1.0 + u(30, m), 0.5 + u(31, m), 60.0 * signed_flux(u(32, m)), 0.7 + u(33, m)
    x = E(m)
    for rf in (None, rho_f):
        asm.co_face_r_delta_t(dev(dc), dev(mag_sf), dev(phi), 0.02, 0.5, x, rho_face=None if rf is None else dev(rf))
        want = co_face(dc, phi, mag_sf, 0.02, 0.5, rho_f=rf)
        assert np.array_equal(host(x), want) and 0.2 * m < np.sum(want > 50.0) < 0.8 * m
    # refusals, nothing launched
    rD, dcd, md, pd = dev(r), dev(dc), dev(mag_sf), dev(phi)
    out, x = E(nf), E(m)
    for bad in (lambda: asm.ddt_phi_corr_local(None, lamd, Sfd, U0d, phid, out), lambda: asm.ddt_phi_corr_local(rD, lamd, Sfd, U0d, None, out),
                lambda: asm.ddt_phi_corr_local(rD, lamd, Sfd, U0d, phid, lamd), lambda: asm.ddt_phi_corr_local(rD, lamd, [Sfd[0], out, Sfd[2]], U0d, phid, out),
                lambda: asm.co_face_r_delta_t(dcd, md, pd, 0.0, 0.5, x), lambda: asm.co_face_r_delta_t(dcd, md, pd, 0.02, -1.0, x),
                lambda: asm.co_face_r_delta_t(dcd, md, pd, 0.02, float("inf"), x), lambda: asm.co_face_r_delta_t(dcd, md, pd, 0.02, float("nan"), x),
                lambda: asm.co_face_r_delta_t(dcd, md, None, 0.02, 0.5, x), lambda: asm.co_face_r_delta_t(x, md, pd, 0.02, 0.5, x)):
        with pytest.raises(eng.MiError):
            bad()
    assert np.all(host(out) == SENTINEL) and np.all(host(x) == SENTINEL)


CO_SHAPES = [(name, mode, tables) for name in ("box", "graph") for (mode, tables) in [(m, "default") for m in ROW_MODES] + [(m, t) for t, m in OTHER_TABLES]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,tables", CO_SHAPES)
def test_co_r_delta_t_in_every_row_shape(pkg, monkeypatch, name, mode, tables):
    """mi_co_r_delta_t against the restatement and against mi_co_face_r_delta_t followed by a numpy row max; a flux of both signs with exact
    zeros; volumetric and mass flux; then two patches (cells with several patch faces) through mi_patch_max.  Between a quarter and three
    quarters of the cells end above 1/deltaT, so both branches of the max are taken"""
    set_row_tables(monkeypatch, tables)
    set_row_blocks(monkeypatch, mode)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=SENTINEL)
    u = pkg.synthetic.splitmix_uniform
    case, addr = shaped_addressing(eng, ctx, pkg.synthetic, shape_case(pkg, name), mode)
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    asm = eng.Assembly(addr)
    dc, mag_sf, phi = 1.0 + u(40, nf), 0.5 + u(41, nf), signed_flux(u(42, nf))
    lam, rho0 = 0.001 + 0.998 * u(43, nf), 0.7 + u(44, n)
    dt, max_co = 0.02, 0.5
    scale = dict(box=34.0, graph=31.0)[name]
    fcs = [(u(50 + p, 300) * n).astype(np.int32) // 3 * 3 for p in range(2)]           # a third of the cells can be hit: repeated cells
    pfields = [dict(dc=1.0 + u(60 + p, 300), mag_sf=0.5 + u(62 + p, 300), phi=scale * signed_flux(u(64 + p, 300)), rho=0.7 + u(66 + p, 300)) for p in range(2)]
    patches = [eng.Patch(ctx, n, fc) for fc in fcs]
    out, xf, xp = E(n), E(nf), E(300)
    for mass in (False, True):
        rho_f = pkg_face_interpolate(lo, up, lam, rho0) if mass else None
        phis = scale * phi * (1.2 if mass else 1.0)
        x = co_face(dc, phis, mag_sf, dt, max_co, rho_f=rho_f)
        want = co_cells(n, lo, up, x)
        above = np.sum(want > 1.0 / dt)
        assert np.all(want >= 1.0 / dt) and 0.25 * n <= above <= 0.75 * n, (above, n)
        kw = dict(lam=dev(lam), rho_old=dev(rho0)) if mass else {}
        asm.co_r_delta_t(dev(dc), dev(mag_sf), dev(phis), dt, max_co, out, **kw)
        got = host(out).copy()
        assert np.array_equal(got, want), (name, mode, tables, mass)
        asm.co_face_r_delta_t(dev(dc), dev(mag_sf), dev(phis), dt, max_co, xf, rho_face=None if rho_f is None else dev(rho_f))
        assert np.array_equal(host(xf), x) and np.array_equal(co_cells(n, lo, up, host(xf)), got)
        pref = []
        for p, fc, q in zip(patches, fcs, pfields):
            asm.co_face_r_delta_t(dev(q["dc"]), dev(q["mag_sf"]), dev(q["phi"]), dt, max_co, xp, rho_face=dev(q["rho"]) if mass else None)
            p.max(xp, out)
            pref.append((fc, co_face(q["dc"], q["phi"], q["mag_sf"], dt, max_co, rho_f=q["rho"] if mass else None)))
        wantp = co_cells(n, lo, up, x, pref)
        assert np.array_equal(host(out), wantp) and np.any(wantp != want)
    if (mode, tables) != ("fixed256", "default"):
        return
    # refusals, nothing launched
    dcd, md, pd, ld, rd = dev(dc), dev(mag_sf), dev(phi), dev(lam), dev(rho0)
    out = E(n)
    for bad in (lambda: asm.co_r_delta_t(dcd, md, pd, 0.0, max_co, out), lambda: asm.co_r_delta_t(dcd, md, pd, dt, 0.0, out),
                lambda: asm.co_r_delta_t(dcd, md, pd, dt, float("nan"), out), lambda: asm.co_r_delta_t(dcd, md, pd, dt, max_co, out, lam=ld),
                lambda: asm.co_r_delta_t(dcd, md, pd, dt, max_co, out, rho_old=rd), lambda: asm.co_r_delta_t(dcd, md, None, dt, max_co, out),
                lambda: asm.co_r_delta_t(dcd, md, pd, dt, max_co, out, lam=ld, rho_old=out), lambda: patches[0].max(None, out),
                lambda: patches[0].max(out, out)):
        with pytest.raises(eng.MiError):
            bad()
    assert np.all(host(out) == SENTINEL)


def pkg_face_interpolate(lo, up, lam, vf):
    """fvc::interpolate: fma(lambda, vf[P] - vf[N], vf[N]) (surfaceInterpolationScheme.C:275-280), one rounding"""
    from assembly_support import fma_each
    return fma_each(lam, vf[lo] - vf[up], vf[up])


# ---- the fused assembly ----------------------------------------------------------------------------------------------------------
def local_ddt_call(V, r):
    """the ddt_call of assembly_support.unfused_sequence for the local schemes on the fields of the variant V"""
    return lambda k, dd, ds: V.case.A.fvm_ddt_local(r, V.case.vol, V.psi_old[k], dd, ds, **V.rho)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,tables", SHAPES)
def test_fused_local_assembly_bit_for_bit(pkg, orc, monkeypatch, name, mode, tables):
    """mi_fvm_assemble_local with r_delta_t_dev against (a) the engine's own unfused sequence -- mi_fvm_ddt_local, mi_fvm_div, mi_fvm_laplacian,
    mi_fvm_su / Sp, the mi_vec_axpby combinations -- and (b) the restatement; with a constant rDeltaT field it gives mi_fvm_assemble's bits; the
    Euler call on the same inputs is untouched.  Then the refusals of the entry, with sentinel-filled outputs"""
    F = FusedCase(pkg, orc, monkeypatch, name, mode, tables)
    eng, dev, host, A, addr, q = F.eng, F.dev, F.host, F.A, F.addr, F.q
    n, nf, vol, flux, lap = F.n, F.nf, F.vol, F.flux, F.lap
    u = pkg.synthetic.splitmix_uniform
    rh = 50.0 + 400.0 * u(181, n)
    r, rconst, rdt = dev(rh), dev(np.full(n, 250.0)), 250.0
    for v in VARIANTS:
        if v["corr"] and name != "box":
            continue
        V = F.variant(v)
        rkw = dict(rho=q["rho"], rho0=q["rho0"]) if v["field"] else dict(rho_value=1.2)
        got = V.fused(dict(V.ddt, local=dict(r_delta_t=r)))
        seq = V.unfused(local_ddt_call(V, r))
        V.assert_same(got, seq, "local")
        V.assert_restated(got, seq, lambda k: fvm_ddt(rh, q["vol"], q["psi0"][k], **rkw))
        # Euler: a constant rDeltaT array gives mi_fvm_assemble's bits, and the call without the key is today's
        eul = V.fused(dict(V.ddt, r_delta_t=rdt))
        V.assert_same(eul, V.unfused(V.euler(rdt)), "euler")
        same = V.fused(dict(V.ddt, r_delta_t=-1.0, local=dict(r_delta_t=rconst)))        # the scalar is ignored
        V.assert_same(same, eul, "constant rDeltaT")
        assert np.array_equal(host(same["mag"]), host(eul["mag"]))
        for k in range(V.R):
            assert not np.array_equal(host(eul["src"][k]), host(got["src"][k]))
    # refusals: nothing launched
    _, _, _, _, S = gpu_env(pkg, fill=SENTINEL)
    p0 = dev(q["psi0"][0])
    o = dict(lower=S(nf), upper=S(nf), diag=S(n), src=[S(n)], mag=S(n))
    call = lambda d, **kw: A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=d, div=dict(flux=flux), laplacian=lap, sum_mag_out=o["mag"], **kw)
    ddt = dict(vol=vol, psi_old=[p0])
    for bad in (dict(ddt, local=dict(r_delta_t=o["diag"])), dict(ddt, local=dict(r_delta_t=o["src"][0])), dict(ddt, local=dict(r_delta_t=o["mag"])),      # an output
                dict(ddt, local=dict(r_delta_t=r), backward=dict(coeffs=(1.5, 2.0, 0.5), psi_old_old=[p0])),                                             # two time schemes
                dict(ddt, local=dict(r_delta_t=r), crank_nicolson=dict(oc=0.9, ddt0=[p0])),
                dict(vol=vol, psi_old=[None], local=dict(r_delta_t=r))):                                                                                   # a missing old field
        with pytest.raises(eng.MiError):
            call(bad)
    lib, t, loc = eng.lib(), eng.FvmTerms(), eng.FvmLocalTerms()
    ptr = lambda x: x.data_ptr()
    t.div_flux_dev, t.vol_dev, t.lap_delta_coeffs_dev, t.lap_gamma_magsf_dev = ptr(flux), ptr(vol), ptr(lap["delta_coeffs"]), ptr(lap["gamma_magsf"])
    so = (C.c_void_p * 1)(ptr(o["src"][0]))
    run = lambda loc_ref: lib.mi_fvm_assemble_local(addr.h, C.byref(t), loc_ref, None, C.c_void_p(ptr(o["lower"])), C.c_void_p(ptr(o["upper"])),
                                                    C.c_void_p(ptr(o["diag"])), so, C.c_void_p(ptr(o["mag"])))
    assert run(None) != 0                                                                  # loc NULL
    assert run(C.byref(loc)) != 0 and b"use mi_fvm_assemble" in lib.mi_last_error()        # both pointers NULL
    loc.r_delta_t_dev = ptr(r)
    assert run(C.byref(loc)) != 0 and b"ddt == 0" in lib.mi_last_error()                   # r_delta_t_dev with terms->ddt == 0
    for x in (o["lower"], o["upper"], o["diag"], o["mag"], o["src"][0]):
        assert np.all(host(x) == SENTINEL)


# ---- the mirror: fv::steadyStateDdtScheme, fv::localEulerDdtScheme, fv::CoEulerDdtScheme ---------------------------------------------------
MIRROR_PROGRAM = r'''
#include "miFoam.H"
#include <cstdio>
using namespace Foam;
// the three scheme objects on a 7-cell chain with one patch: New() accepts and refuses; CorDeltaT, fvc::ddt, fvc::ddtCorr and fvm::assemble (with
// the bounded convection scheme's divPhi) of each, every double printed as %a
static std::vector<double> field(int s, int n, int salt) { std::vector<double> v(n); for (int i = 0; i < n; ++i) v[i] = ((i * 7 + s * 13 + salt) % 11) / 8.0 - 0.5 + s * 0.125; return v; }
static std::vector<double> pos(int s, int n, int salt) { std::vector<double> v = field(s, n, salt); for (double& x : v) x = x + 1.0; return v; }
static void print(const char* tag, const char* k, const scalargpuField& f) { std::printf("%s_%s", tag, k); for (double x : f.asHost()) std::printf(" %a", x); std::printf("\n"); }
template <class F> static void refused(const char* what, F f) { try { f(); std::printf("accepted %s\n", what); } catch (const error&) { std::printf("refused %s\n", what); } }
template <class Scheme> static void run(const char* k, Scheme& s, const lduAddressing& addr, const std::vector<labelList>& pfc, int n)
{
    const int nf = n - 1;
    const scalargpuField w(pos(0, nf, 3)), phiOld(field(1, nf, 5)), vf(field(4, n, 0)), vf0(field(5, n, 0)), V(pos(6, n, 1)), flux(field(7, nf, 2));
    const scalargpuField dcs(pos(8, nf, 4)), gm(pos(9, nf, 6)), divPhi(field(10, n, 3));
    vectorgpuField Sf(nf), Uold(n);
    for (int d = 0; d < 3; ++d) { Sf.component(d) = field(2, nf, d); Uold.component(d) = field(3, n, d); }
    scalargpuField out(n), corr(nf);
    fvc::ddt(out, s, vf, vf0); print("ddt", k, out);
    fvc::ddtCorr(corr, addr, s, w, Sf, Uold, phiOld); print("corr", k, corr);
    fvScalarMatrix M("T", addr, pfc, std::vector<bool>(pfc.size(), false));
    fvm::assemble(M, s, 1.0, V, vf0, &flux, &w, &dcs, &gm, &divPhi);
    print("diag", k, M.diag()); print("source", k, M.source()); print("upper", k, M.upper()); print("lower", k, M.lower());
    fvScalarMatrix D("T", addr, pfc, std::vector<bool>(pfc.size(), false));
    fvm::ddt(D, s, 1.0, V, vf0); print("ddtdiag", k, D.diag()); print("ddtsource", k, D.source());
}
int main()
{
    try {
        const int n = 7, nf = n - 1;
        labelList lo(nf), up(nf); for (int i = 0; i < nf; ++i) { lo[i] = i; up[i] = i + 1; }
        lduAddressing addr(n, lo, up);
        const labelList fc{0, 6, 6};
        const std::vector<labelList> pfc{fc};
        fvPatchCells patch(n, fc);
        fv::steadyStateDdtScheme st = fv::steadyStateDdtScheme::New(" steadyState ");
        fv::localEulerDdtScheme le = fv::localEulerDdtScheme::New("localEuler rDeltaT");
        fv::CoEulerDdtScheme co = fv::CoEulerDdtScheme::New("CoEuler phi rho 0.5");
        std::printf("names %s %s %s %a\n", le.rDeltaTName().c_str(), co.phiName().c_str(), co.rhoName().c_str(), co.maxCo());
        const scalargpuField r(pos(11, n, 2)), dc(pos(12, nf, 1)), magSf(pos(13, nf, 5)), lam(pos(0, nf, 3)), phi(field(14, nf, 4)), rho0(pos(15, n, 6));
        const scalargpuField pdc(pos(16, 3, 1)), pms(pos(17, 3, 2)), pphi(field(18, 3, 3)), prho(pos(19, 3, 4));
        refused("unbound", [&] { le.localRDeltaT(); });
        refused("bind_other_name", [&] { le.bind("rSubDeltaT", r); });
        le.bind("rDeltaT", r);
        refused("cor_before_bind", [&] { scalargpuField x(n); co.CorDeltaT(x); });
        refused("bind_other_flux", [&] { co.bind("phiv", phi); });
        co.setMesh(addr, dc, magSf, lam); co.bind("phi", phi); co.addPatch(patch, pdc, pms, pphi, &prho); co.setTime(0.25);
        scalargpuField cor(n); co.CorDeltaT(cor); print("cor", "vol", cor);
        run("steady", st, addr, pfc, n); run("local", le, addr, pfc, n); run("co", co, addr, pfc, n);
        co.bind("phi", phi, "rho", &rho0); co.CorDeltaT(cor); print("cor", "mass", cor);
        refused("bind_other_rho", [&] { co.bind("phi", phi, "thermo:rho", &rho0); });
        refused("localEuler", [] { fv::localEulerDdtScheme::New("localEuler"); });
        refused("CoEuler_no_maxCo", [] { fv::CoEulerDdtScheme::New("CoEuler phi rho"); });
        refused("CoEuler_bad_maxCo", [] { fv::CoEulerDdtScheme::New("CoEuler phi rho -1"); });
        refused("steady_extra", [] { fv::steadyStateDdtScheme::New("steadyState 1"); });
        refused("steady_Euler", [] { fv::steadyStateDdtScheme::New("Euler"); });
        refused("local_given_steady", [] { fv::localEulerDdtScheme::New("steadyState"); });
        refused("co_given_local", [] { fv::CoEulerDdtScheme::New("localEuler rDeltaT"); });
        std::vector<std::string> e{"bounded", "Gauss", "upwind"}, e2{"Gauss", "linear"};
        const bool b1 = fv::boundedConvection(e), b2 = fv::boundedConvection(e2);
        std::printf("bounded %d %d %d %d %s\n", (int)b1, (int)e.size(), (int)b2, (int)e2.size(), e[0].c_str());
        const scalargpuField vf(field(4, n, 0)), V(pos(6, n, 1)), flux(field(7, nf, 2)), divPhi(field(10, n, 3));
        scalargpuField db(n), dp(n), face(nf);
        fvc::divBounded(db, addr, flux, &lam, vf, V, divPhi); print("div", "bounded", db);
    } catch (const std::exception& e) { std::printf("FAILED %s\n", e.what()); return 1; }
    return 0;
}
'''


@pytest.mark.gpu
def test_mirror_scheme_objects_against_the_restatement(pkg, orc, tmp_path):
    """the mirror's three scheme objects from a small program of its own: New() accepts and refuses; CoEuler's CorDeltaT (internal faces, then the
    patch; volumetric and mass flux), fvc::ddt, fvc::ddtCorr, fvm::ddt and fvm::assemble with the bounded scheme's divPhi, each against the
    restatement on the values the program formed, bit for bit"""
    import os
    import subprocess
    from test_polymesh import PKG
    from test_bounded_steady import bounded_diag
    src, exe = tmp_path / "local.C", tmp_path / "local"
    src.write_text(MIRROR_PROGRAM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "foam"), "-I", os.path.join(os.path.dirname(PKG), "include"), str(src), "-o", str(exe),
                    "-L" + PKG, "-lmiFoam", "-lrapidcfd_amd", "-Wl,-rpath," + PKG], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAILED" not in out.stdout and "accepted" not in out.stdout, out.stdout + out.stderr
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if "_" in w[0] and w[0] not in ("refused",) and len(w) > 1 and w[1].startswith(("0x", "-0x")):
            got[w[0]] = np.array([float.fromhex(x) for x in w[1:]])
    for what in ("unbound", "bind_other_name", "cor_before_bind", "bind_other_flux", "bind_other_rho", "localEuler", "CoEuler_no_maxCo", "CoEuler_bad_maxCo",
                 "steady_extra", "steady_Euler", "local_given_steady", "co_given_local"):
        assert "refused " + what in out.stdout, what
    assert "names rDeltaT phi rho 0x1p-1" in out.stdout and "bounded 1 2 0 2 Gauss" in out.stdout
    n, nf = 7, 6
    field = lambda s, m, salt: np.array([((i * 7 + s * 13 + salt) % 11) / 8.0 - 0.5 + s * 0.125 for i in range(m)])
    pos = lambda s, m, salt: field(s, m, salt) + 1.0
    lo, up, fc = np.arange(nf, dtype=np.int32), np.arange(1, n, dtype=np.int32), np.array([0, 6, 6], dtype=np.int32)
    r, dc, mag_sf, lam, phi, rho0 = pos(11, n, 2), pos(12, nf, 1), pos(13, nf, 5), pos(0, nf, 3), field(14, nf, 4), pos(15, n, 6)
    pdc, pms, pphi, prho = pos(16, 3, 1), pos(17, 3, 2), field(18, 3, 3), pos(19, 3, 4)
    dt, max_co = 0.25, 0.5
    cor = co_cells(n, lo, up, co_face(dc, phi, mag_sf, dt, max_co), [(fc, co_face(pdc, pphi, pms, dt, max_co))])
    assert np.array_equal(got["cor_vol"], cor) and np.any(cor > 1.0 / dt) and np.any(cor == 1.0 / dt)
    cor_mass = co_cells(n, lo, up, co_face(dc, phi, mag_sf, dt, max_co, rho_f=pkg_face_interpolate(lo, up, lam, rho0)),
                        [(fc, co_face(pdc, pphi, pms, dt, max_co, rho_f=prho))])
    assert np.array_equal(got["cor_mass"], cor_mass) and not np.array_equal(cor_mass, cor)
    w, phi_old, vf, vf0, V, flux = pos(0, nf, 3), field(1, nf, 5), field(4, n, 0), field(5, n, 0), pos(6, n, 1), field(7, nf, 2)
    dcs, gm, div_phi = pos(8, nf, 4), pos(9, nf, 6), field(10, n, 3)
    Sf, U0 = [field(2, nf, d) for d in range(3)], [field(3, n, d) for d in range(3)]
    lB, uB, dB = orc.fvm_div(n, lo, up, w, flux)
    uL, dL = orc.fvm_laplacian(n, lo, up, dcs, gm)
    dB = bounded_diag(dB, V, div_phi)
    for k, rk in (("steady", None), ("local", r), ("co", cor)):
        if rk is None:
            want_ddt, want_corr, (dD, sD) = np.zeros(n), np.zeros(nf), (np.zeros(n), np.zeros(n))
        else:
            want_ddt, want_corr, (dD, sD) = fvc_ddt(rk, vf, vf0), ddt_corr(orc, n, lo, up, rk, w, Sf, U0, phi_old)[0], fvm_ddt(rk, V, vf0)
        assert np.array_equal(got["ddt_" + k], want_ddt) and np.array_equal(got["corr_" + k], want_corr), k
        assert np.array_equal(got["ddtdiag_" + k], dD) and np.array_equal(got["ddtsource_" + k], sD), k
        assert np.array_equal(got["diag_" + k], (dD + dB) - dL) and np.array_equal(got["source_" + k], sD), k
        assert np.array_equal(got["upper_" + k], uB - uL) and np.array_equal(got["lower_" + k], lB - uL), k
    face = flux * pkg_face_interpolate(lo, up, lam, vf)
    assert np.array_equal(got["div_bounded"], orc.surface_integrate(n, lo, up, face, V) - (div_phi * vf))
