"""`snGradSchemes { default limited 0.5; }`, `laplacianSchemes { default Gauss linear limited corrected 0.33; }`: the limited
non-orthogonal correction (snGradSchemes/limitedSnGrad/limitedSnGrad.{H,C}) -- parser, the face pass on the internal faces and on a
coupled patch for a scalar and a vector field, the non-orthogonal corrector loop, scalarTransportFoam and icoFoam.

The expected values are a numpy restatement of limitedSnGrad.C:58-84 written here, one numpy operator per field operator of the
reference and each rounded, so every comparison with the engine is bit for bit:
    corr    = correctedScheme_().correction(vf)            the oracle's pinned sngrad_correction_flux without gammaMagSf, per component
    sn      = deltaCoeffs*(vf[N] - vf[P])                  snGradScheme.C:103-108 with nonOrthDeltaCoeffs
    limiter = min(k*mag(sn)/((1 - k)*mag(corr) + SMALL), 1)
    result  = limiter*corr                                  then gammaMagSf*result (gaussLaplacianSchemes.C:64-90)
mag of a vector is sqrt(magSqr) with magSqr contracted as every dot product of the engine's face passes is:
fma(z, z, fma(x, x, y*y)), written out exactly with Fraction (assembly_support.fma_each)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from assembly_support import fma_each, gpu_env

SMALL = 1e-15


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def mag(v):
    """mag(scalar) = fabs; mag(Vector) = sqrt(magSqr), magSqr = fma(z, z, fma(x, x, y*y))"""
    if len(v) == 1:
        return np.abs(v[0])
    return np.sqrt(fma_each(v[2], v[2], fma_each(v[0], v[0], v[1] * v[1])))


def limit(k, sn, corr, gamma_magsf=None):
    """limitedSnGrad.C:63-84 from the snGrad and the correction of every component -> ([gammaMagSf *] limiter*corr per component, limiter)"""
    with np.errstate(invalid="ignore", over="ignore"):
        num = k * mag(sn)
        den = ((1 - k) * mag(corr)) + SMALL
        q = num / den
        limiter = np.where(q < 1.0, q, 1.0)                  # Foam::min(a, b) = (a < b) ? a : b -- a NaN quotient gives 1
        out = [limiter * c for c in corr]
        if gamma_magsf is not None:
            out = [gamma_magsf * o for o in out]
    return out, limiter


def limited_flux(orc, lo, up, k, cv, lam, delta, vf, grad, gamma_magsf=None):
    """internal faces; vf 1 or 3 cell arrays, grad[3*j + d] = d(vf_j)/dx_d"""
    corr = [orc.sngrad_correction_flux(lo, up, cv, lam, grad[3 * j:3 * j + 3], None) for j in range(len(vf))]
    sn = [delta * (f[up] - f[lo]) for f in vf]
    return limit(k, sn, corr, gamma_magsf)


def patch_limited_flux(orc, fc, k, cv, w, delta, vf, nbr_vf, grad, nbr_grad, gamma_magsf=None):
    """a coupled patch: corr from the oracle's patch form, snGrad = deltaCoeffs*(patchNeighbourField - patchInternalField) (snGradScheme.C:165-169)"""
    corr = [orc.patch_sngrad_correction_flux(fc, cv, w, grad[3 * j:3 * j + 3], nbr_grad[3 * j:3 * j + 3], None) for j in range(len(vf))]
    sn = [delta * (nb - f[fc]) for f, nb in zip(vf, nbr_vf)]
    return limit(k, sn, corr, gamma_magsf)


@functools.lru_cache(maxsize=None)
def mesh(dims):
    from test_assembly import skewed_mesh
    return skewed_mesh(dims)


@functools.lru_cache(maxsize=None)
def synthetic(dims, n_comp):
    """inputs that take both branches of the min: vf in [-0.5, 0.5), `gradients` in [-64, 64) (not a Gauss gradient), a varying gammaMagSf"""
    import __graft_entry__ as graft
    syn = graft.load_package().synthetic
    M = mesh(dims)
    n, nI = M["n"], M["nI"]
    vf = syn.splitmix_uniform(11, n_comp * n) - 0.5
    g = (syn.splitmix_uniform(12, 3 * n_comp * n) - 0.5) * 128
    gms = M["G"]["magSf"][:nI] * (1.0 + 0.3 * syn.splitmix_uniform(4, nI))
    return ([np.ascontiguousarray(vf[j * n:(j + 1) * n]) for j in range(n_comp)], [np.ascontiguousarray(g[i * n:(i + 1) * n]) for i in range(3 * n_comp)], gms)


@functools.lru_cache(maxsize=None)
def expected(dims, n_comp, k, with_gamma):
    from oracle import oracle as orc
    M = mesh(dims)
    vf, g, gms = synthetic(dims, n_comp)
    return limited_flux(orc, M["lo"], M["up"], k, M["corr"], M["G"]["weights"], M["G"]["delta"], vf, g, gms if with_gamma else None)


KS = (0.0, 0.33, 0.5, 1.0)
MESHES = [(3, 2, 2), (9, 8, 7)]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_sngrad_parse_through_the_c_abi(pkg):
    """every accepted and every refused form: kind, coefficient and the token in the message"""
    eng = pkg.engine
    lib = eng.lib()
    for name in ("mi_sngrad_parse", "mi_sngrad_limited_correction_flux", "mi_patch_sngrad_limited_correction_flux"):
        assert name in eng.SYMBOLS and hasattr(lib, name)
    assert eng.SNGRAD_KINDS == ("uncorrected", "orthogonal", "corrected", "limited")
    for text, kind, k in (("uncorrected", 0, 1.0), ("orthogonal", 1, 1.0), ("corrected", 2, 1.0), ("limited 0.5", 3, 0.5), ("limited corrected 0.33", 3, 0.33),
                          ("limited 1", 3, 1.0), ("limited 0", 3, 0.0), ("limited corrected 1.0", 3, 1.0), ("limited corrected 0", 3, 0.0),
                          ("  limited\tcorrected\n3.3e-1 ", 3, 0.33), (" corrected ", 2, 1.0)):
        s = eng.sngrad_parse(text)
        assert (s.kind, s.limit_coeff) == (kind, k), text
    out = eng.SnGradScheme(-7, -7.0)
    for text, token in (("limited 1.5", "1.5"), ("limited -0.1", "-0.1"), ("limited corrected 2", "2"), ("limited nan", "nan"),
                        ("limited", "limited"), ("limited corrected", "corrected"), ("", "empty"),
                        ("corrected 0.5", "0.5"), ("uncorrected corrected", "corrected"), ("limited 0.5 0.5", "0.5"), ("limited corrected 0.5 x", "x"),
                        ("limited 0.5 corrected", "corrected"), ("limited corrected abc", "abc"),
                        ("limited uncorrected 0.5", "uncorrected"), ("limited orthogonal 0.5", "orthogonal"),
                        ("limited limited 0.5", "limited limited"), ("limited limited corrected 0.5", "limited limited"),
                        ("faceCorrected", "faceCorrected"), ("linearFit 1", "linearFit"), ("quadraticFit 1", "quadraticFit"), ("Corrected", "Corrected"),
                        ("limited faceCorrected 0.5", "faceCorrected"), ("Gauss linear corrected", "Gauss")):
        rc = lib.mi_sngrad_parse(text.encode(), C.byref(out))
        assert rc != 0 and token in lib.mi_last_error().decode(), (text, lib.mi_last_error().decode())
        assert (out.kind, out.limit_coeff) == (-7, -7.0)                      # a refusal writes nothing
        with pytest.raises(eng.MiError):
            eng.sngrad_parse(text)
    assert lib.mi_sngrad_parse(None, C.byref(out)) != 0 and lib.mi_sngrad_parse(b"corrected", None) != 0


@pytest.mark.parametrize("dims", MESHES)
@pytest.mark.parametrize("n_comp", [1, 3])
def test_restatement_k1_is_corrected_k0_is_zero_and_both_branches_are_taken(orc, dims, n_comp):
    M = mesh(dims)
    lo, up, G = M["lo"], M["up"], M["G"]
    vf, g, gms = synthetic(dims, n_comp)
    sn_mag = mag([G["delta"] * (f[up] - f[lo]) for f in vf])
    assert np.all(sn_mag > 1e-15)
    one, lim1 = expected(dims, n_comp, 1.0, True)
    for j in range(n_comp):                                                  # k = 1: the `corrected` flux, bit for bit
        assert np.array_equal(one[j], orc.sngrad_correction_flux(lo, up, M["corr"], G["weights"], g[3 * j:3 * j + 3], gms))
    assert np.all(lim1 == 1.0)
    zero, lim0 = expected(dims, n_comp, 0.0, True)
    assert np.all(lim0 == 0.0) and all(np.all(z == 0.0) for z in zero)       # k = 0: +-0 everywhere
    for k in (0.33, 0.5):
        flux, lim = expected(dims, n_comp, k, False)
        assert np.all(lim >= 0.0) and np.all(lim <= 1.0)
        share = float(np.mean(lim < 1.0))
        print(f"dims {dims} n_comp {n_comp} k {k}: share of faces with limiter < 1 = {share:.3f}")
        assert 0.10 <= share <= 0.90, share                                  # at least 10 % of the faces take each branch of the min
        for j in range(n_comp):                                              # the limited correction is never larger than the full one
            full = orc.sngrad_correction_flux(lo, up, M["corr"], G["weights"], g[3 * j:3 * j + 3], None)
            assert np.all(np.abs(flux[j]) <= np.abs(full)) and np.array_equal(flux[j][lim == 1.0], full[lim == 1.0])


def test_restatement_keeps_the_exact_face_gradient_of_a_linear_field(orc):
    """skewed_mesh((7, 6, 5)), phi = a.x with its exact gradient: |snGrad| >= |correction| on every face of this mesh, so limited 0.5 takes limiter 1
    and the identity of test_nonorth_correction_recovers_the_exact_face_gradient_of_a_linear_field holds unchanged"""
    M = mesh((7, 6, 5))
    G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
    a = np.array([0.7, -1.3, 0.45])
    phi = G["C"] @ a
    gex = [np.full(n, a[k]) for k in range(3)]
    (flux,), lim = limited_flux(orc, lo, up, 0.5, M["corr"], G["weights"], G["delta"], [phi], gex, G["magSf"][:nI])
    assert np.all(lim == 1.0)
    unc = G["delta"] * G["magSf"][:nI] * (phi[up] - phi[lo])
    assert np.max(np.abs(unc + flux - G["Sf"][:nI] @ a)) < 1e-13
    assert np.max(np.abs(flux)) > 1e-3 * np.max(np.abs(unc))
    # the vector form: three linear fields, one limiter from the vector magnitudes
    b = np.array([[0.7, -1.3, 0.45], [0.2, 0.9, -0.4], [-1.1, 0.3, 0.8]])
    vf = [G["C"] @ b[j] for j in range(3)]
    gv = [np.full(n, b[j][d]) for j in range(3) for d in range(3)]
    fl, lim = limited_flux(orc, lo, up, 0.5, M["corr"], G["weights"], G["delta"], vf, gv, G["magSf"][:nI])
    assert np.all(lim == 1.0)
    for j in range(3):
        unc = G["delta"] * G["magSf"][:nI] * (vf[j][up] - vf[j][lo])
        assert np.max(np.abs(unc + fl[j] - G["Sf"][:nI] @ b[j])) < 1e-13
    # the patch form with the upper cells as neighbours is the internal form up to the uncontracted interpolate
    m = 50
    pf, plim = patch_limited_flux(orc, lo[:m], 0.5, [c[:m] for c in M["corr"]], G["weights"][:m], G["delta"][:m], [phi], [phi[up[:m]]], gex,
                                  [x[up[:m]] for x in gex], G["magSf"][:m])
    assert np.all(plim == 1.0) and np.max(np.abs(pf[0] - flux[:m])) < 1e-14


def test_restatement_nan_quotient_gives_limiter_one():
    sn, corr = [np.array([np.nan, 0.3, 0.0, 0.0])], [np.array([0.2, np.nan, 0.0, 0.5])]
    (out,), lim = limit(0.5, sn, corr)
    assert np.array_equal(lim, [1.0, 1.0, 0.0, 0.0]) and out[0] == 0.2 and np.isnan(out[1]) and out[2] == 0.0 and out[3] == 0.0
    (out,), lim = limit(1.0, [np.array([0.0, 1e-16, 1e-15])], [np.array([0.4, 0.4, 0.4])])
    assert np.array_equal(lim, [0.0, 1e-16 / 1e-15, 1.0])                    # k = 1 is `corrected` only where |snGrad| >= SMALL


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dims", MESHES)
@pytest.mark.parametrize("n_comp", [1, 3])
def test_engine_limited_flux_internal_faces_bit_exact(pkg, orc, dims, n_comp):
    """(3, 2, 2): 20 faces, one partial block; (9, 8, 7): 1 321 faces, several blocks and a tail.  Every k, with and without gammaMagSf,
    with and without the limiter output: flux of every component and the limiter bit for bit"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    M = mesh(dims)
    G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
    assert nI == {(3, 2, 2): 20, (9, 8, 7): 1321}[dims]
    vf, g, gms = synthetic(dims, n_comp)
    addrs = [eng.Addressing(ctx, n, lo, up)]
    if dims == (9, 8, 7):
        addrs.append(eng.Addressing(ctx, n, lo, up, ordered=True))           # the caller's numbering kept (mi_addr_create_ordered)
        assert addrs[1].is_ordered
    cv, lam, dc, vfd, gd, gmsd = [dev(c) for c in M["corr"]], dev(G["weights"]), dev(G["delta"]), [dev(x) for x in vf], [dev(x) for x in g], dev(gms)
    for addr in addrs:
        A = eng.Assembly(addr)
        for k in (KS if addr is addrs[0] else (0.33,)):
            for with_gamma in (True, False):
                ref, rlim = expected(dims, n_comp, k, with_gamma)
                for want_lim in (True, False):
                    out, lim = [E(nI) for _ in range(n_comp)], E(nI)
                    A.sngrad_limited_correction_flux(k, cv, lam, dc, vfd, gd, gmsd if with_gamma else None, out, lim if want_lim else None)
                    for j in range(n_comp):
                        assert np.array_equal(host(out[j]), ref[j]), (k, with_gamma, want_lim, j)
                    assert np.array_equal(host(lim), rlim if want_lim else np.full(nI, -77.0)), (k, with_gamma, want_lim)
    # the yardstick pass still gives what it gave (its interpolate-and-dot is the shared device function now)
    A = eng.Assembly(addrs[0])
    y = E(nI); A.sngrad_correction_flux(cv, lam, gd[:3], gmsd, y)
    assert np.array_equal(host(y), orc.sngrad_correction_flux(lo, up, M["corr"], G["weights"], g[:3], gms))


@pytest.mark.gpu
@pytest.mark.parametrize("n_comp", [1, 3])
def test_engine_limited_flux_nan_in_one_cell(pkg, orc, n_comp):
    """a NaN in vf at one cell: the quotient of that cell's faces is NaN, Foam::min gives limiter 1, the flux there is the full correction
    (finite: the gradient arrays are separate inputs here); a NaN in one gradient array at another cell: limiter 1 and a NaN flux in that
    component.  Every other face keeps its bits."""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    dims, k = (9, 8, 7), 0.5
    M = mesh(dims)
    G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
    vf, g, gms = synthetic(dims, n_comp)
    vf, g = [x.copy() for x in vf], [x.copy() for x in g]
    c1, c2 = 200, 37
    vf[0][c1] = np.nan; g[1][c2] = np.nan
    ref, rlim = limited_flux(orc, lo, up, k, M["corr"], G["weights"], G["delta"], vf, g, gms)
    clean, clim = expected(dims, n_comp, k, True)
    f1, f2 = (lo == c1) | (up == c1), (lo == c2) | (up == c2)
    assert f1.sum() >= 3 and f2.sum() >= 3 and not np.any(f1 & f2)
    assert np.all(rlim[f1] == 1.0) and np.all(rlim[f2] == 1.0) and np.all(np.isfinite(ref[0][f1])) and np.all(np.isnan(ref[0][f2]))
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    out, lim = [E(nI) for _ in range(n_comp)], E(nI)
    A.sngrad_limited_correction_flux(k, [dev(c) for c in M["corr"]], dev(G["weights"]), dev(G["delta"]), [dev(x) for x in vf], [dev(x) for x in g], dev(gms), out, lim)
    got, glim = [host(o) for o in out], host(lim)
    assert np.array_equal(glim, rlim)
    other = ~(f1 | f2)
    assert np.array_equal(glim[other], clim[other])
    for j in range(n_comp):
        assert np.array_equal(got[j], ref[j], equal_nan=True), j
        assert np.array_equal(got[j][other], clean[j][other]), j
    assert np.all(np.isnan(got[0][f2])) and np.all(np.isfinite(got[0][f1]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_comp", [1, 3])
def test_engine_limited_flux_coupled_patch_bit_exact(pkg, orc, n_comp):
    """the first min(64, nI) internal faces posed as a patch whose neighbour values are the upper cells'"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    for dims in MESHES:
        M = mesh(dims)
        G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
        vf, g, gms = synthetic(dims, n_comp)
        m = min(64, nI)
        fc = lo[:m]
        P = eng.Patch(ctx, n, fc)
        nvf, ng = [x[up[:m]] for x in vf], [x[up[:m]] for x in g]
        cv, w, dc = [c[:m] for c in M["corr"]], G["weights"][:m], G["delta"][:m]
        for k in KS:
            for gamma in (gms[:m], None):
                ref, rlim = patch_limited_flux(orc, fc, k, cv, w, dc, vf, nvf, g, ng, gamma)
                if k in (0.33, 0.5):
                    assert 0 < np.sum(rlim < 1.0) < m
                out, lim = [E(m) for _ in range(n_comp)], E(m)
                P.sngrad_limited_correction_flux(k, [dev(c) for c in cv], dev(w), dev(dc), [dev(x) for x in vf], [dev(x) for x in nvf], [dev(x) for x in g],
                                                 [dev(x) for x in ng], None if gamma is None else dev(gamma), out, lim)
                for j in range(n_comp):
                    assert np.array_equal(host(out[j]), ref[j]), (dims, k, j)
                assert np.array_equal(host(lim), rlim), (dims, k)
        # k = 1: the `corrected` patch pass
        y = E(m); P.sngrad_correction_flux([dev(c) for c in cv], dev(w), [dev(x) for x in g[:3]], [dev(x) for x in ng[:3]], dev(gms[:m]), y)
        out = [E(m) for _ in range(n_comp)]
        P.sngrad_limited_correction_flux(1.0, [dev(c) for c in cv], dev(w), dev(dc), [dev(x) for x in vf], [dev(x) for x in nvf], [dev(x) for x in g],
                                         [dev(x) for x in ng], dev(gms[:m]), out)
        assert np.array_equal(host(out[0]), host(y))


@pytest.mark.gpu
def test_engine_limited_flux_refusals_launch_nothing(pkg):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    dims = (3, 2, 2)
    M = mesh(dims)
    G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    P = eng.Patch(ctx, n, lo[:8])
    for n_comp in (1, 3):
        vf, g, gms = synthetic(dims, n_comp)
        cv, lam, dc, vfd, gd, gmsd = [dev(c) for c in M["corr"]], dev(G["weights"]), dev(G["delta"]), [dev(x) for x in vf], [dev(x) for x in g], dev(gms)
        out, lim = [E(nI) for _ in range(n_comp)], E(nI)
        gms0 = gms.copy()

        def refused(*a, **kw):
            with pytest.raises(eng.MiError):
                A.sngrad_limited_correction_flux(*a, **kw)
            assert all(np.all(host(o) == -77.0) for o in out) and np.all(host(lim) == -77.0) and np.array_equal(host(gmsd), gms0)
        refused(1.5, cv, lam, dc, vfd, gd, gmsd, out, lim)                                       # k outside [0, 1]
        refused(-0.1, cv, lam, dc, vfd, gd, gmsd, out, lim)
        refused(float("nan"), cv, lam, dc, vfd, gd, gmsd, out, lim)
        refused(0.5, cv, lam, dc, vfd, gd, gmsd, [gmsd] + out[1:], lim)                          # an output aliases an input
        refused(0.5, cv, lam, dc, vfd, gd, gmsd, out, lam)
        refused(0.5, cv, lam, dc, vfd, gd, gmsd, out, out[0])                                    # ... or another output
        refused(0.5, cv, lam, dc, vfd, gd, gmsd, [out[0]] + [None] * (n_comp - 1) if n_comp > 1 else [None], lim)   # a missing output
        refused(0.5, cv, None, dc, vfd, gd, gmsd, out, lim)                                      # a missing input
        refused(0.5, cv, lam, dc, vfd, gd[:-1] + [None], gmsd, out, lim)
        refused(0.5, cv, lam, dc, vfd, gd, gmsd, out, gmsd)
        if n_comp == 3:
            refused(0.5, cv, lam, dc, vfd, gd, gmsd, [out[0], out[1], out[0]], lim)
        # n_comp = 2
        with pytest.raises(eng.MiError):
            A.sngrad_limited_correction_flux(0.5, cv, lam, dc, [vfd[0], vfd[0]], (gd + gd)[:6], gmsd, [out[0], lim], None)
        assert np.all(host(out[0]) == -77.0) and np.all(host(lim) == -77.0)
        # an array not aligned for a double
        lib = eng.lib()
        pv = lambda xs: (C.c_void_p * len(xs))(*[eng._ptr(x) for x in xs])
        odd = C.c_void_p(gmsd.data_ptr() + 4)
        rc = lib.mi_sngrad_limited_correction_flux(A.addr.h, C.c_int32(n_comp), C.c_double(0.5), eng._ptr(cv[0]), eng._ptr(cv[1]), eng._ptr(cv[2]), eng._ptr(lam),
                                                   eng._ptr(dc), pv(vfd), pv(gd), odd, pv(out), eng._ptr(lim))
        assert rc != 0 and "aligned" in lib.mi_last_error().decode()
        assert all(np.all(host(o) == -77.0) for o in out)
        # the patch form
        m = 8
        pout, plim = [E(m) for _ in range(n_comp)], E(m)
        pa = ([dev(c[:m]) for c in M["corr"]], dev(G["weights"][:m]), dev(G["delta"][:m]), vfd, [dev(x[up[:m]]) for x in vf], gd, [dev(x[up[:m]]) for x in g], dev(gms[:m]))
        for bad in ((1.5,) + pa + (pout, plim), (0.5,) + pa + (pout, pa[1]), (0.5,) + pa + (pout, pout[0]), (0.5,) + pa[:3] + (vfd + vfd[:1],) + pa[4:] + (pout, plim)):
            with pytest.raises(eng.MiError):
                P.sngrad_limited_correction_flux(*bad)
            assert all(np.all(host(o) == -77.0) for o in pout) and np.all(host(plim) == -77.0)


@pytest.mark.gpu
def test_engine_limited_laplacian_three_nonorth_correctors(pkg, orc):
    """nNonOrthogonalCorrectors = 3 of laplacian(gamma, p) == S with `limited 0.5` on skewed_mesh((9, 8, 7)): the engine's sweeps against the same
    loop over the restatement and the oracle's sweeps -- sources bit for bit, solutions to the bar of
    test_engine_nonorth_correction_bit_exact_and_corrected_solve"""
    import torch
    from test_assembly import nonorth_source_correction
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    syn = pkg.synthetic
    k = 0.5
    M = mesh((9, 8, 7))
    G, n, nI, lo, up = M["G"], M["n"], M["nI"], M["lo"], M["up"]
    addr = eng.Addressing(ctx, n, lo, up)
    A = eng.Assembly(addr)
    patches = {name: (eng.Patch(ctx, n, M["owner"][start:start + cnt]), start, cnt, ptype) for name, ptype, cnt, start in M["patches"]}
    Sf = [np.ascontiguousarray(G["Sf"][:nI, d]) for d in range(3)]
    gms = G["magSf"][:nI] * (1.0 + 0.3 * syn.splitmix_uniform(4, nI))
    bv_host = lambda name, ptype, fc, start, cnt, phi: (np.zeros(cnt) if ptype == "patch" else phi[fc])
    V = dev(G["V"])

    def engine_correction(phi_d):
        ssf = E(nI); A.face_interpolate(dev(G["weights"]), phi_d, ssf)
        g = [E(n) for _ in range(3)]
        A.gauss_grad([dev(x) for x in Sf], ssf, None, g)
        for name, (P, start, cnt, ptype) in patches.items():
            bv = E(cnt)
            if ptype == "patch": bv.zero_()
            else: P.internal_field(phi_d, bv)
            for d in range(3):
                P.add_product(dev(G["Sf"][start:start + cnt, d]), bv, g[d], 0)
        gd = [E(n) for _ in range(3)]
        for d in range(3):
            eng._chk(eng.lib().mi_vec_div(ctx.h, n, eng._ptr(g[d]), eng._ptr(V), eng._ptr(gd[d])))
        flux, lim = E(nI), E(nI)
        A.sngrad_limited_correction_flux(k, [dev(c) for c in M["corr"]], dev(G["weights"]), dev(G["delta"]), [phi_d], gd, dev(gms), [flux], lim)
        div = E(n); A.surface_integrate(flux, V, div)
        return flux, lim, div

    def restated_correction(phi):
        g, _, _ = nonorth_source_correction(orc, M, phi, lambda nm, pt, fc, s, c: bv_host(nm, pt, fc, s, c, phi), gms)
        (flux,), lim = limited_flux(orc, lo, up, k, M["corr"], G["weights"], G["delta"], [phi], g, gms)
        return flux, lim, G["V"] * orc.surface_integrate(n, lo, up, flux, G["V"])

    up_c, diag_c = E(nI), E(n)
    A.fvm_laplacian(dev(G["delta"]), dev(gms), up_c, diag_c)
    ru, rd = orc.fvm_laplacian(n, lo, up, G["delta"], gms)
    for name, (P, start, cnt, ptype) in patches.items():
        if ptype != "patch":
            continue
        ic = -(G["magSf"][start:start + cnt] * G["delta_b"][start - nI:start - nI + cnt])
        P.add(dev(ic), diag_c, 0)
        rd = orc.patch_add(M["owner"][start:start + cnt], ic, rd, 0)
    assert np.array_equal(host(diag_c), rd) and np.array_equal(host(up_c), ru)
    mat = eng.Matrix(addr); mat.set_coeffs(diag_c, up_c, None)
    S = orc.System([syn.LduCase(n, lo, up, rd, ru, None, np.zeros(n))])
    S0 = -(G["V"] * (1.0 + np.sin(5 * G["C"][:, 0])))
    p_d = torch.zeros(n, dtype=torch.float64, device="cuda:0"); p_h = np.zeros(n)
    limited_faces = 0
    for corr in range(3):
        flux, lim, div = engine_correction(p_d)
        src_d = dev(S0.copy()); A.submul(V, div, src_d)
        rflux, rlim, rvdiv = restated_correction(p_h)
        src_h = orc.submul(G["V"], rvdiv / G["V"], S0)
        if corr == 0:                                                        # the same p on both sides: every sweep bit for bit
            assert np.array_equal(host(flux), rflux) and np.array_equal(host(lim), rlim) and np.array_equal(host(src_d), src_h)
        limited_faces += int(np.sum(rlim < 1.0))
        perf = mat.pcg(p_d, src_d, "DIC", tolerance=1e-10, maxIter=500)
        p_h, ref = S.pcg(p_h, src_h, "DIC", tolerance=1e-10, maxIter=500)
        assert perf["nIterations"] == ref["nIterations"] and np.max(np.abs(perf["history"] - ref["history"])) < 1e-10 * ref["history"][0]
        assert np.max(np.abs(host(p_d) - p_h)) < 1e-9 * np.max(np.abs(p_h))
        # the restated sweeps on the ENGINE's p give the engine's source bit for bit
        if corr < 2:
            ph = host(p_d).copy()
            _, _, d2 = engine_correction(p_d)
            s2 = dev(S0.copy()); A.submul(V, d2, s2)
            _, _, rv2 = restated_correction(ph)
            assert np.array_equal(host(s2), orc.submul(G["V"], rv2 / G["V"], S0))
    assert corr == 2 and np.max(np.abs(p_h)) > 0


# ---- the applications ------------------------------------------------------------------------------------------------------------
def walk_scalar_transport(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, delta_t, n_steps, k, n_non_orth):
    """tests/transport_walk.py::walk (div Gauss linear) with the correction flux of the Laplacian by the restatement; k None: `corrected`.
    -> solver lines, T, share of faces with limiter < 1 over the run"""
    import transport_walk
    w = transport_walk.walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, [delta_t] * n_steps, "linear", "corrected" if k is None else ("limited", k),
                            n_non_orth)
    return w.lines, w.T, w.limited_share


def walk_icofoam(pkg, orc, pts, faces, owner, neighbour, patches, nu, delta_t, n_steps, k):
    """the walk of tests/test_icofoam.py (div Gauss linear, nCorrectors 2, one non-orthogonal corrector), both Laplacians' correction fluxes swapped
    for the restatement: the U correction ONE vector call (one limiter from the vector snGrad and the vector correction), the p correction the
    scalar form, also in pEqn.flux().  k None: `corrected`.  -> solver lines, continuity errors, U, p, share of faces with limiter < 1 (U, p)"""
    from test_polymesh import geometry
    syn = pkg.synthetic
    G = geometry(pts, faces, owner, neighbour)
    n, nI = int(owner.max()) + 1, len(neighbour)
    lo, up = owner[:nI].astype(np.int32), neighbour.astype(np.int32)
    V, lam, delta, magSf = G["V"], G["weights"], G["delta"], G["magSf"][:nI]
    Sf = [np.ascontiguousarray(G["Sf"][:nI, d]) for d in range(3)]
    P = []
    for name, ptype, cnt, start in patches:
        fc = owner[start:start + cnt].astype(np.int32)
        ub = np.tile(np.array([0.0, 1.0, 0.0]) if name == "inlet" else np.zeros(3), (cnt, 1))
        sfb = G["Sf"][start:start + cnt]
        P.append(dict(fc=fc, ub=ub, sf=[np.ascontiguousarray(sfb[:, d]) for d in range(3)], phi=ub[:, 0] * sfb[:, 0] + ub[:, 1] * sfb[:, 1] + ub[:, 2] * sfb[:, 2],
                      diff=nu * G["magSf"][start:start + cnt] * G["delta_b"][start - nI:start - nI + cnt]))
    U = [np.zeros(n) for _ in range(3)]
    p = np.zeros(n)
    phi = orc.flux_div(n, lo, up, lam, Sf, U, want_div=False)
    r_dt = 1.0 / delta_t
    lines, cont, cumulative, totalV = [], [], 0.0, float(np.sum(V))
    cv = G["Sf"][:nI] / magSf[:, None] - (G["C"][up] - G["C"][lo]) * delta[:, None]
    cv = [np.ascontiguousarray(cv[:, d]) for d in range(3)]
    count = dict(U=[0, 0], p=[0, 0])

    def full_grad(vf, patch_values):
        g = orc.gauss_grad(n, lo, up, Sf, orc.face_interpolate(lo, up, lam, vf), None)
        for q, pv in zip(P, patch_values):
            for d in range(3):
                g[d] = orc.patch_add_product(q["fc"], q["sf"][d], vf[q["fc"]] if pv is None else pv, g[d], 0)
        return [x / V for x in g]
    grad_p = lambda: full_grad(p, [None] * len(P))

    def correction(name, vf, grads, gamma):
        if k is None:
            return [orc.sngrad_correction_flux(lo, up, cv, lam, grads[3 * j:3 * j + 3], gamma) for j in range(len(vf))]
        out, lim = limited_flux(orc, lo, up, k, cv, lam, delta, vf, grads, gamma)
        count[name][0] += int(np.sum(lim < 1.0)); count[name][1] += nI
        return out
    for step in range(n_steps):
        Uold, phiOld = [u.copy() for u in U], phi.copy()
        lB, uB, dB = orc.fvm_div(n, lo, up, lam, phi)
        uL, dL = orc.fvm_laplacian(n, lo, up, delta, nu * magSf)
        lower, upper = lB - uL, uB - uL
        gp = grad_p()
        gU = [x for j in range(3) for x in full_grad(Uold[j], [q["ub"][:, j].copy() for q in P])]
        cfU = correction("U", Uold, gU, -(nu * magSf))
        mats = []
        for j in range(3):
            dD, sD = orc.fvm_ddt_euler(r_dt, 1.0, V, Uold[j])
            diag = (dD + dB) - dL
            source = orc.submul(V, orc.surface_integrate(n, lo, up, cfU[j], V), sD)
            mats.append(dict(diag=diag, source=source, ic=[q["diff"] for q in P], bc=[q["diff"] * q["ub"][:, j] - q["phi"] * q["ub"][:, j] for q in P]))
        for j in range(3):
            Mj = mats[j]
            dtot, stot = Mj["diag"].copy(), Mj["source"] - V * gp[j]
            for q, ic, bc in zip(P, Mj["ic"], Mj["bc"]):
                dtot = orc.patch_add(q["fc"], ic, dtot, 0); stot = orc.patch_add(q["fc"], bc, stot, 0)
            U[j], perf = orc.System([syn.LduCase(n, lo, up, dtot, upper, lower, stot)]).pbicg(U[j], stot, "AINV", tolerance=1e-9, relTol=0.0)
            lines.append(("AINVPBiCG", "Ux Uy Uz".split()[j], perf["initialResidual"], perf["finalResidual"], perf["nIterations"]))
        for corr in range(2):
            A = mats[0]["diag"].copy()
            for q in P:
                A = orc.patch_add(q["fc"], ((q["diff"] + q["diff"]) + q["diff"]) / 3.0, A, 0)
            rAU = 1.0 / (A / V)
            HbyA = []
            for j in range(3):
                Mj = mats[j]
                H = orc.System([syn.LduCase(n, lo, up, Mj["diag"], upper, lower, Mj["source"])]).H(U[j]) + Mj["source"]
                for q, bc in zip(P, Mj["bc"]):
                    H = orc.patch_add(q["fc"], bc, H, 0)
                HbyA.append(rAU * (H / V))
            rAUf = orc.face_interpolate(lo, up, lam, rAU)
            ddtc = orc.ddt_phi_corr(lo, up, r_dt, lam, Sf, Uold, None, phiOld)
            phiHbyA, div = orc.flux_div(n, lo, up, lam, Sf, HbyA, None, rAUf, ddtc, None, True)
            for q in P:
                div = orc.patch_add(q["fc"], q["phi"], div, 0)
            for non_orth in range(2):
                upP, dP = orc.fvm_laplacian(n, lo, up, delta, rAUf * magSf)
                (cfp,) = correction("p", [p], grad_p(), rAUf * magSf)
                sP = orc.submul(V, orc.surface_integrate(n, lo, up, cfp, V), div.copy())
                sP[0] += dP[0] * 0.0; dP = dP.copy(); dP[0] += dP[0]                    # setReference(0, 0)
                final = corr == 1 and non_orth == 1
                p, perf = orc.System([syn.LduCase(n, lo, up, dP, upP, None, sP)]).pcg(p, sP, "AINV", tolerance=1e-8, relTol=0.0 if final else 0.05)
                lines.append(("AINVPCG", "p", perf["initialResidual"], perf["finalResidual"], perf["nIterations"]))
            flux = orc.System([syn.LduCase(n, lo, up, dP, upP, None, sP)]).faceH(p)
            phi = phiHbyA - (flux + cfp)
            ce = orc.surface_integrate(n, lo, up, phi, None)
            for q in P:
                ce = orc.patch_add(q["fc"], q["phi"], ce, 0)
            loc, glob = float(np.sum(np.abs(ce))) * delta_t / totalV, float(np.sum(ce)) * delta_t / totalV
            cumulative += glob
            cont.append((loc, glob, cumulative))
            gp = grad_p()
            U = [HbyA[j] - rAU * gp[j] for j in range(3)]
    share = {key: c[0] / max(c[1], 1) for key, c in count.items()}
    return lines, cont, U, p, share


def set_laplacian_scheme(case_dir, scheme):
    from transport_walk import rewrite_schemes
    rewrite_schemes(case_dir, ("Gauss linear corrected", "Gauss linear " + scheme), ("default corrected", "default " + scheme))


def test_the_walks_reproduce_the_existing_corrected_walks(pkg, orc, tmp_path):
    """CPU: with k None the two walks above ARE the walks of test_scalartransportfoam.py / test_icofoam.py (`corrected`), bit for bit -- so what the
    application tests compare against differs from those only in the swapped correction flux"""
    from test_icofoam import oracle_icofoam, write_cavity
    from test_scalartransportfoam import oracle_scalar_transport, write_channel
    dims = (6, 5, 4)
    pts, faces, owner, neighbour, patches, tin, T0 = write_channel(str(tmp_path / "channel"), dims, 0.01, 0.01, 2, "linear", True, 1)
    ref, Tref = oracle_scalar_transport(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, 0.01, 0.01, 2, "linear", True, 1)
    got, T, _ = walk_scalar_transport(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, 0.01, 0.01, 2, None, 1)
    assert got == ref and np.array_equal(T, Tref)
    pts, faces, owner, neighbour, patches = write_cavity(str(tmp_path / "cavity"), dims, 0.01, 0.005, 1, "linear", "binary", True)
    rl, rc, rU, rp = oracle_icofoam(pkg, orc, pts, faces, owner, neighbour, patches, 0.01, 0.005, 1, "linear", True)
    gl, gc, gU, gp, _ = walk_icofoam(pkg, orc, pts, faces, owner, neighbour, patches, 0.01, 0.005, 1, None)
    assert gl == rl and gc == rc and np.array_equal(gp, rp) and all(np.array_equal(a, b) for a, b in zip(gU, rU))


@pytest.mark.gpu
def test_scalarTransportFoam_limited_laplacian_matches_the_walk(pkg, orc, tmp_path):
    """the distorted (12, 9, 7) channel, `Gauss linear limited 0.5`, 2 non-orthogonal correctors, 3 steps: every solver line and the written T to
    the bars of test_scalartransportfoam.py.  k = 0.5: 32.3 % of the faces take limiter < 1 over the run on this mesh (the walk reports the share)."""
    from test_polymesh import PKG, read_vol_field
    from transport_walk import assert_solver_lines, solver_lines
    from test_scalartransportfoam import write_channel
    DT, delta_t, n_steps, n_non_orth, k = 0.01, 0.01, 3, 2, 0.5
    case_dir = str(tmp_path / "channel")
    pts, faces, owner, neighbour, patches, tin, T0 = write_channel(case_dir, (12, 9, 7), DT, delta_t, n_steps, "linear", True, n_non_orth)
    set_laplacian_scheme(case_dir, "limited 0.5")
    out = subprocess.run([os.path.join(PKG, "scalarTransportFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout[-1500:]
    got = solver_lines(out.stdout)
    ref, Tref, share = walk_scalar_transport(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, delta_t, n_steps, k, n_non_orth)
    print(f"scalarTransportFoam limited {k}: share of faces with limiter < 1 over the run = {share:.4f}")
    assert share > 0
    assert len(got) == len(ref) == n_steps * (n_non_orth + 1)
    assert_solver_lines(got, ref)
    f = read_vol_field(os.path.join(case_dir, f"{n_steps * delta_t:.10g}", "T"))
    assert f["header"]["class"] == "volScalarField" and np.max(np.abs(f["internalField"] - Tref)) <= 1e-8 * np.max(np.abs(Tref))
    # ... and the limiter limits: not the `corrected` result
    _, Tc, _ = walk_scalar_transport(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, delta_t, n_steps, None, n_non_orth)
    assert np.max(np.abs(Tc - Tref)) > 1e-9 * np.max(np.abs(Tref))


@pytest.mark.gpu
def test_icoFoam_limited_laplacians_match_the_walk(pkg, orc, tmp_path):
    """the distorted (12, 9, 7) cavity, `Gauss linear limited corrected 0.33`, 3 steps: every solver line, the continuity errors and the written
    U and p to the bars of test_icofoam.py.  k = 0.33: 52.1 % of the faces take limiter < 1 in the U correction and 34.6 % in the p
    correction over the run on this mesh (the walk reports the shares)."""
    from test_polymesh import PKG, read_vol_field
    from transport_walk import assert_solver_lines, solver_lines
    from test_icofoam import CONT, write_cavity
    nu, delta_t, n_steps, k = 0.01, 0.005, 3, 0.33
    case_dir = str(tmp_path / "cavity")
    pts, faces, owner, neighbour, patches = write_cavity(case_dir, (12, 9, 7), nu, delta_t, n_steps, "linear", "binary", True)
    set_laplacian_scheme(case_dir, "limited corrected 0.33")
    out = subprocess.run([os.path.join(PKG, "icoFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout[-2000:]
    got = solver_lines(out.stdout)
    cont = [tuple(map(float, m.groups())) for m in map(CONT.match, out.stdout.splitlines()) if m]
    ref_lines, ref_cont, refU, refp, share = walk_icofoam(pkg, orc, pts, faces, owner, neighbour, patches, nu, delta_t, n_steps, k)
    print(f"icoFoam limited corrected {k}: share of faces with limiter < 1 over the run: U {share['U']:.4f}, p {share['p']:.4f}")
    assert share["U"] > 0 and share["p"] > 0
    assert len(got) == len(ref_lines) == n_steps * 7 and len(cont) == len(ref_cont) == n_steps * 2
    assert_solver_lines(got, ref_lines)
    for g, r in zip(cont, ref_cont):
        assert abs(g[0] - r[0]) <= 1e-6 * r[0] + 1e-16 and abs(g[1] - r[1]) < 1e-15 and abs(g[2] - r[2]) < 1e-15, (g, r)
    tn = f"{n_steps * delta_t:.10g}"
    fU, fp = read_vol_field(os.path.join(case_dir, tn, "U")), read_vol_field(os.path.join(case_dir, tn, "p"))
    Uref = np.stack(refU, axis=1)
    assert fU["internalField"].shape == Uref.shape and np.max(np.abs(fU["internalField"] - Uref)) <= 1e-7 * np.max(np.abs(Uref))
    assert np.max(np.abs(fp["internalField"] - refp)) <= 1e-7 * np.max(np.abs(refp))
    _, _, Uc, _, _ = walk_icofoam(pkg, orc, pts, faces, owner, neighbour, patches, nu, delta_t, n_steps, None)
    assert np.max(np.abs(np.stack(Uc, axis=1) - Uref)) > 1e-9 * np.max(np.abs(Uref))   # not the `corrected` result


@pytest.mark.gpu
def test_applications_refuse_limited_over_uncorrected(pkg, tmp_path):
    from test_polymesh import PKG
    from test_icofoam import write_cavity
    from test_scalartransportfoam import write_channel
    write_channel(str(tmp_path / "channel"), (4, 3, 2), 0.01, 0.01, 1, "linear", True, 0)
    write_cavity(str(tmp_path / "cavity"), (4, 3, 2), 0.01, 0.005, 1, "linear", "ascii", True)
    for app, case in (("scalarTransportFoam", "channel"), ("icoFoam", "cavity")):
        for bad, token in (("limited uncorrected 0.5", "uncorrected"), ("limited 1.5", "1.5"), ("faceCorrected", "faceCorrected")):
            case_dir = str(tmp_path / case)
            sch = os.path.join(case_dir, "system", "fvSchemes")
            good = open(sch).read()
            set_laplacian_scheme(case_dir, bad)
            out = subprocess.run([os.path.join(PKG, app), case_dir], capture_output=True, text=True, timeout=120)
            open(sch, "w").write(good)
            assert out.returncode != 0 and "limited [corrected] <k>" in out.stderr and token in out.stderr, (app, bad, out.stderr)
        # a limited Laplacian beside another snGradSchemes entry (what test_icoFoam_refuses_what_it_does_not_assemble poses) or another coefficient
        for entry in ("corrected", "limited 0.33"):
            case_dir = str(tmp_path / case)
            sch = os.path.join(case_dir, "system", "fvSchemes")
            good = open(sch).read()
            open(sch, "w").write(good.replace("Gauss linear corrected", "Gauss linear limited 0.5").replace("default corrected", "default " + entry))
            out = subprocess.run([os.path.join(PKG, app), case_dir], capture_output=True, text=True, timeout=120)
            open(sch, "w").write(good)
            assert out.returncode != 0 and "needs the same snGradSchemes entry" in out.stderr and "'" + entry + "'" in out.stderr, (app, entry, out.stderr)
