"""interFoam's interfaceProperties on the device (transportModels/interfaceProperties/interfaceProperties.C:58-159, :220-231): the face unit
interface normal flux nHatf with its patch and contact-angle forms, the curvature K = -fvc::div(nHatf), the surface tension force and
nearInterface (mi_interface_nhatf, mi_patch_interface_nhatf, mi_interface_curvature, mi_surface_tension_force and its coupled-patch form,
mi_near_interface), bit for bit against the restatement of tests/interface_support.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from assembly_support import bits, gpu_env, same, set_face_grid
from interface_support import (B12_BOUND, MESHES, angle_case, boundary_cells, circle_curvature, coupled_gradient, fma_v, inputs,
                               literal_curvature, literal_force, literal_near_interface, literal_nhatf, literal_patch_nhatf, mesh, patch_case,
                               quiet_cell, restate_curvature, restate_force, restate_near_interface, restate_nhatf, restate_patch_nhatf)

EXPORTS = ("mi_interface_nhatf", "mi_patch_interface_nhatf", "mi_interface_create", "mi_interface_destroy", "mi_interface_curvature",
           "mi_surface_tension_force", "mi_patch_surface_tension_force", "mi_near_interface")
NAN = float("nan")
SEED = {"box": 1000, "edge_257": 1020, "isolated": 1040}
_CACHE = {}


def _case(pkg, name):
    """the mesh, its inputs and the restated results, computed once and left unchanged"""
    if name not in _CACHE:
        L = mesh(pkg, name)
        I = inputs(pkg.synthetic, L, SEED[name])
        lo, up = L["lo"], L["up"]
        nhatf, nv, m = restate_nhatf(lo, up, I["lam"], L["Sf"], I["grad"], I["delta_n"])
        K = restate_curvature(L, nhatf, I["bn"], I["vol"])
        _CACHE[name] = dict(L=L, I=I, nhatf=nhatf, nv=nv, m=m, K=K)
    return _CACHE[name]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS


def test_mirror_has_interface_properties(pkg):
    """foam/miFoam: the class interfaceProperties with the reference's members is in the library, each once"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    for name in ("Foam::interfaceProperties::interfaceProperties(", "Foam::interfaceProperties::correct(", "Foam::interfaceProperties::calculateK(",
                 "Foam::interfaceProperties::surfaceTensionForce(", "Foam::interfaceProperties::nearInterface(", "Foam::interfaceProperties::sigmaK("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name
    for name in ("Foam::interfaceProperties::correct(", "Foam::interfaceProperties::calculateK(", "Foam::interfaceProperties::surfaceTensionForce(",
                 "Foam::interfaceProperties::nearInterface(", "Foam::interfaceProperties::sigmaK("):
        assert syms.count(" T " + name) == 1, name


@pytest.mark.parametrize("name", MESHES)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg, name):
    c = _case(pkg, name)
    L, I = c["L"], c["I"]
    lo, up, dn = L["lo"], L["up"], I["delta_n"]
    lit, lnv = literal_nhatf(lo, up, I["lam"], L["Sf"], I["grad"], dn)
    assert same(lit, c["nhatf"]) and all(same(a, b) for a, b in zip(lnv, c["nv"]))
    gz = [g == 0.0 for g in I["grad"]]
    zero = (gz[0] & gz[1] & gz[2])
    both = zero[lo] & zero[up]
    assert np.any(both) and np.all(c["nhatf"][both] == 0.0) and np.all(c["m"][both] == 0.0)   # 0/(0 + delta_n): exactly 0, no special case
    near = (c["m"] > 0.1 * dn) & (c["m"] < 10 * dn)
    assert np.any(near) and np.any(c["m"] > 1e6 * dn)
    without = restate_nhatf(lo, up, I["lam"], L["Sf"], I["grad"], 1e-300)[0]                  # adding delta_n changes many bits there
    moved = np.abs(bits(without[near]).astype(np.int64) - bits(c["nhatf"][near]).astype(np.int64))
    assert np.any(moved > 2 ** 40)
    # the curvature: its own literal loops, both signs, an exact -0.0 on the quiet cell and on every cell without faces
    assert same(literal_curvature(L, c["nhatf"], I["bn"], I["vol"]), c["K"])
    assert np.any(c["K"] > 0) and np.any(c["K"] < 0)
    c0, _ = quiet_cell(L)
    cnt = np.bincount(lo, minlength=L["n"]) + np.bincount(up, minlength=L["n"])
    assert cnt[c0] > 0 and c["K"][c0] == 0.0 and np.signbit(c["K"][c0])
    faceless = cnt + np.bincount(boundary_cells(L), minlength=L["n"]) == 0
    assert np.any(faceless) == (name == "isolated") and np.all(np.signbit(c["K"][faceless])) and np.all(c["K"][faceless] == 0.0)
    assert all(len(p) > 0 for p in L["fcs"]) and len(L["fcs"]) == 2
    # the force and nearInterface
    for corr in (None, I["corr"]):
        args = (I["sigma"], I["lam"], I["dc"], c["K"][lo], c["K"][up], I["alpha"][lo], I["alpha"][up], corr)
        assert same(literal_force(*args), restate_force(*args))
    a = I["alpha"]
    ni = restate_near_interface(a)
    assert same(ni, literal_near_interface(a))
    assert np.any(a == 0.01) and np.all(ni[a == 0.01] == 1.0) and np.any(a == 0.99) and np.all(ni[a == 0.99] == 1.0)
    assert np.all(ni[(a < 0.01) | (a > 0.99)] == 0.0) and np.any(a < 0.01) and np.any(a > 0.99) and set(np.unique(ni)) == {0.0, 1.0}


@pytest.mark.parametrize("name", MESHES)
def test_each_stated_rounding_changes_a_compared_bit(pkg, name):
    """magSqr contracted or not, division or reciprocal-multiply, sigma*K before or after the interpolate: the GPU comparison can tell"""
    c = _case(pkg, name)
    L, I = c["L"], c["I"]
    lo, up = L["lo"], L["up"]
    for alt in (dict(contracted=False), dict(reciprocal=True)):
        other = restate_nhatf(lo, up, I["lam"], L["Sf"], I["grad"], I["delta_n"], **alt)
        assert not same(other[0], c["nhatf"]) and not all(same(a, b) for a, b in zip(other[1], c["nv"])), alt
    args = (I["sigma"], I["lam"], I["dc"], c["K"][lo], c["K"][up], I["alpha"][lo], I["alpha"][up])
    assert not same(restate_force(*args), restate_force(*args, sigma_after=True))


def test_patch_restatements_agree_and_tell_the_rules_apart(pkg):
    P = patch_case(pkg.synthetic)
    fc, dn = P["fc"], P["delta_n"]
    g = coupled_gradient(P["w"], [x[fc] for x in P["grad"]], P["nbr"])
    r = restate_patch_nhatf(g, P["Sf"], dn)
    l = literal_patch_nhatf(g, P["Sf"], dn)
    assert same(r[0], l[0]) and all(same(a, b) for a, b in zip(r[1], l[1]))
    assert P["m"] % 256 and P["m"] > 256
    zero = (g[0] == 0) & (g[1] == 0) & (g[2] == 0)
    assert np.any(zero) and np.all(r[0][zero] == 0.0) and np.any(~zero)
    as_internal = [fma_v(P["w"], x[fc] - q, q) for x, q in zip(P["grad"], P["nbr"])]          # the internal faces' interpolate: other bits
    assert not all(same(a, b) for a, b in zip(g, as_internal))
    for corr in (None, P["corr"]):
        args = (P["sigma"], P["w"], P["dc"], P["K"][fc], P["nbrK"], P["alpha"][fc], P["nbr_alpha"], corr)
        assert same(literal_force(*args, patch=True), restate_force(*args, patch=True))
        assert not same(restate_force(*args, patch=True), restate_force(*args, patch=False))


def test_contact_angle_restatements_agree(pkg):
    A = angle_case(pkg.synthetic)
    r = restate_patch_nhatf(A["g"], A["Sf"], A["delta_n"], A["magSf"], A["theta"])
    a12 = r[3]
    assert a12[0] == 1.0 and np.all(np.abs(a12[1:]) <= 0.999) and np.any(np.abs(a12) > 0.99) and np.any(a12 < -0.9) and np.any(a12 > 0.9)
    assert A["theta"].min() == 10.0 and A["theta"].max() == 170.0
    assert np.isnan(r[0][0]) and np.isnan(r[2][0]) and np.all(np.isfinite(r[0][1:])) and np.all(np.isfinite(r[2][1:]))
    # from the same b1 and b2 the two forms agree bit for bit (the libm of numpy and of math may differ: that is what b12 is for)
    l = literal_patch_nhatf(A["g"], A["Sf"], A["delta_n"], A["magSf"], A["theta"], b12=r[4])
    ok = np.arange(A["m"]) > 0
    assert same(r[0][ok], l[0][ok]) and same(r[2][ok], l[2][ok]) and same(r[3], l[3]) and all(same(a[ok], b[ok]) for a, b in zip(r[1], l[1]))
    assert np.isnan(l[0][0]) and np.isnan(l[2][0])
    # the corrected normal makes the angle theta with the wall: nf & n = cos(theta).  Not exactly: both normalisations leave n short of
    # unit length by delta_n/|g| <= 3.7e-8/0.5, and the 2 x 2 solve amplifies that by at most 1/det <= 1/(1 - 0.999^2) = 500: 1e-4 bounds it
    nf = [s / A["magSf"] for s in A["Sf"]]
    cosw = sum(a * b for a, b in zip(nf, r[1]))
    assert np.max(np.abs(cosw[ok] - np.cos(np.pi / 180.0 * A["theta"][ok]))) < 1e-4


def test_curvature_of_a_circle(pkg):
    """the restatement alone: over the cells with 0.1 < alpha < 0.9 the mean of K lies within 10 % of 1/R = 4 and every value between 0.5/R
    and 1.5/R (numpy over 180 cells: mean 3.86, range 2.82 to 4.98)"""
    alpha, K = circle_curvature(pkg.synthetic)
    band = (alpha > 0.1) & (alpha < 0.9)
    k = K[band]
    print("cells", int(band.sum()), "mean", float(k.mean()), "range", float(k.min()), float(k.max()))
    assert band.sum() > 100
    assert abs(k.mean() - 4.0) <= 0.4
    assert k.min() >= 2.0 and k.max() <= 6.0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_nhatf_on_the_three_meshes(pkg, monkeypatch, name, blocks):
    """with and without the nHatfv output; MI_FACE_GRID at its default and forced to 1 and 3 workgroups"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I = c["L"], c["I"]
    nf = L["lo"].shape[0]
    A = eng.Assembly(eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    lam, sf, grad = dev(I["lam"]), [dev(s) for s in L["Sf"]], [dev(g) for g in I["grad"]]
    out, out2, nv = E(nf), E(nf), [E(nf) for _ in range(3)]
    A.interface_nhatf(I["delta_n"], lam, sf, grad, out, nv)
    A.interface_nhatf(I["delta_n"], lam, sf, grad, out2)
    _eq(host(out), c["nhatf"], (name, blocks, "nHatf"))
    _eq(host(out2), c["nhatf"], (name, blocks, "nHatf alone"))
    for k in range(3):
        _eq(host(nv[k]), c["nv"][k], (name, blocks, "nHatfv", k))


@pytest.mark.gpu
def test_the_patch_forms_on_429_faces(pkg):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    P = patch_case(pkg.synthetic)
    fc, m, dn = P["fc"], P["m"], P["delta_n"]
    patch = eng.Patch(ctx, P["n"], fc)
    sf = [dev(s) for s in P["Sf"]]
    g = coupled_gradient(P["w"], [x[fc] for x in P["grad"]], P["nbr"])
    want = restate_patch_nhatf(g, P["Sf"], dn)
    out, nv, out2 = E(m), [E(m) for _ in range(3)], E(m)
    patch.interface_nhatf(dn, [dev(x) for x in P["grad"]], sf, out, patch_weights=dev(P["w"]), nbr_grad=[dev(x) for x in P["nbr"]], nhatfv_out=nv)
    patch.interface_nhatf(dn, [dev(x) for x in P["grad"]], sf, out2, patch_weights=dev(P["w"]), nbr_grad=[dev(x) for x in P["nbr"]])
    _eq(host(out), want[0], "coupled nHatf"); _eq(host(out2), want[0], "coupled nHatf alone")
    for k in range(3):
        _eq(host(nv[k]), want[1][k], ("coupled nHatfv", k))
    # the plain form: the boundary value of gradAlpha as given, no cell read
    plain = restate_patch_nhatf(P["nbr"], P["Sf"], dn)
    out, nv = E(m), [E(m) for _ in range(3)]
    patch.interface_nhatf(dn, [dev(x) for x in P["nbr"]], sf, out, nhatfv_out=nv)
    _eq(host(out), plain[0], "plain nHatf")
    for k in range(3):
        _eq(host(nv[k]), plain[1][k], ("plain nHatfv", k))


@pytest.mark.gpu
def test_the_contact_angle_form(pkg):
    """The device's cos / acos are not the host's, so: given the device's own b1 and b2, everything after them bit for bit; b1 and b2 against
    numpy within 16*2^-52 absolute.  The bound is derived: the host expression is within 2*2^-52 of the exact value (checked against 200-bit
    arithmetic over 24 000 inputs including |a12| up to 1 - 1e-12), a device library at <= 2 ulp per function adds at most 4 + 1 + 1 units
    of 2^-52 through acos, the subtraction and cos.  On the face with a12 = 1 exactly both sides are NaN."""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    A = angle_case(pkg.synthetic)
    m, dn = A["m"], A["delta_n"]
    patch = eng.Patch(ctx, 3 * m, np.arange(0, 3 * m, 3, dtype=np.int32))
    out, nv, grd, b1, b2 = E(m), [E(m) for _ in range(3)], E(m), E(m), E(m)
    patch.interface_nhatf(dn, [dev(x) for x in A["g"]], [dev(x) for x in A["Sf"]], out, nhatfv_out=nv, patch_magsf=dev(A["magSf"]),
                          theta_deg=dev(A["theta"]), gradient_out=grd, b12_out=(b1, b2))
    b1, b2 = host(b1), host(b2)
    host_form = restate_patch_nhatf(A["g"], A["Sf"], dn, A["magSf"], A["theta"])
    d1, d2 = np.max(np.abs(b1 - host_form[4][0])), np.max(np.abs(b2 - host_form[4][1]))
    print("largest deviation of b1, b2 from numpy in units of 2^-52:", d1 * 2.0 ** 52, d2 * 2.0 ** 52)
    want = restate_patch_nhatf(A["g"], A["Sf"], dn, A["magSf"], A["theta"], b12=(b1, b2))
    ok = np.arange(m) > 0
    got = host(out)
    assert np.isnan(got[0]) and np.isnan(want[0][0]) and np.isnan(host(grd)[0]) and np.isnan(want[2][0])
    _eq(got[ok], want[0][ok], "nHatf")
    _eq(host(grd)[ok], want[2][ok], "gradient")
    for k in range(3):
        _eq(host(nv[k])[ok], want[1][k][ok], ("nHatp", k))
    # without the optional outputs: the same flux
    out2 = E(m)
    patch.interface_nhatf(dn, [dev(x) for x in A["g"]], [dev(x) for x in A["Sf"]], out2, patch_magsf=dev(A["magSf"]), theta_deg=dev(A["theta"]))
    _eq(host(out2)[ok], want[0][ok], "nHatf alone")
    assert d1 <= B12_BOUND and d2 <= B12_BOUND, (d1 * 2.0 ** 52, d2 * 2.0 ** 52)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_curvature_on_the_three_meshes(pkg, name):
    """against the restatement, and against the engine's own unfused sequence with the sign flipped on the host"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I = c["L"], c["I"]
    n = L["n"]
    for tag, addr in _addressings(eng, ctx, L):
        B = eng.GradBoundary(addr, L["fcs"], ["other", "other"])
        H = eng.Interface(addr, B)
        A = eng.Assembly(addr)
        nhatf, bn, vol, K = dev(c["nhatf"]), dev(I["bn"]), dev(I["vol"]), E(n)
        A.interface_curvature(H, nhatf, vol, K, bn)
        got = host(K)
        _eq(got, c["K"], (name, tag, "restatement"))
        s, off = E(n), 0
        A.surface_integrate(nhatf, None, s)
        for fc in L["fcs"]:
            eng.Patch(ctx, n, fc).add(dev(I["bn"][off:off + fc.shape[0]]), s)
            off += fc.shape[0]
        eng._chk(eng.lib().mi_vec_div(ctx.h, C.c_int64(n), eng._ptr(s), eng._ptr(vol), eng._ptr(s)))
        _eq(got, -host(s), (name, tag, "unfused sequence"))
        H.close(); B.close()


@pytest.mark.gpu
def test_surface_tension_force_and_near_interface(pkg):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    for name in MESHES:
        c = _case(pkg, name)
        L, I = c["L"], c["I"]
        lo, up, n = L["lo"], L["up"], L["n"]
        nf = lo.shape[0]
        A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
        for corr in (None, I["corr"]):
            out = E(nf)
            A.surface_tension_force(I["sigma"], dev(I["lam"]), dev(I["dc"]), dev(c["K"]), dev(I["alpha"]), out, None if corr is None else dev(corr))
            _eq(host(out), restate_force(I["sigma"], I["lam"], I["dc"], c["K"][lo], c["K"][up], I["alpha"][lo], I["alpha"][up], corr), (name, corr is None))
        ni = E(n)
        A.near_interface(dev(I["alpha"]), ni)
        _eq(host(ni), restate_near_interface(I["alpha"]), (name, "nearInterface"))
    P = patch_case(pkg.synthetic)
    fc, m = P["fc"], P["m"]
    patch = eng.Patch(ctx, P["n"], fc)
    for corr in (None, P["corr"]):
        out = E(m)
        patch.surface_tension_force(P["sigma"], dev(P["w"]), dev(P["dc"]), dev(P["K"]), dev(P["nbrK"]), dev(P["alpha"]), dev(P["nbr_alpha"]), out,
                                    None if corr is None else dev(corr))
        _eq(host(out), restate_force(P["sigma"], P["w"], P["dc"], P["K"][fc], P["nbrK"], P["alpha"][fc], P["nbr_alpha"], corr, patch=True), ("patch", corr is None))


class Misaligned:
    """a device address four bytes into a float64 tensor, as engine._ptr takes one: not aligned for a double"""

    def __init__(self, t):
        self.t, self.dtype = t, t.dtype

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def data_ptr(self):
        return self.t.data_ptr() + 4


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, "box")
    L, I = c["L"], c["I"]
    lo, up, n = L["lo"], L["up"], L["n"]
    nf, dn = lo.shape[0], I["delta_n"]
    addr = eng.Addressing(ctx, n, lo, up)
    A = eng.Assembly(addr)
    lam, sf, grad = dev(I["lam"]), [dev(s) for s in L["Sf"]], [dev(g) for g in I["grad"]]
    out, nv, spare = E(nf), [E(nf) for _ in range(3)], E(nf + 1)
    bad = Misaligned(spare)
    for args, why in (((NAN, lam, sf, grad, out, nv), "delta_n"), ((float("inf"), lam, sf, grad, out, nv), "delta_n"), ((0.0, lam, sf, grad, out, nv), "delta_n"),
                      ((-dn, lam, sf, grad, out, nv), "delta_n"),
                      ((dn, None, sf, grad, out, nv), "missing"), ((dn, lam, [sf[0], None, sf[2]], grad, out, nv), "missing"),
                      ((dn, lam, sf, [grad[0], grad[1], None], out, nv), "missing"), ((dn, lam, sf, grad, None, nv), "missing"),
                      ((dn, lam, sf, grad, out, [nv[0], None, nv[2]]), "missing"),
                      ((dn, lam, sf, grad, lam, nv), "alias"), ((dn, lam, sf, grad, out, [nv[0], sf[1], nv[2]]), "alias"),
                      ((dn, lam, sf, grad, out, [nv[0], out, nv[2]]), "differ"), ((dn, lam, sf, grad, out, [nv[0], nv[0], nv[2]]), "differ"),
                      ((dn, bad, sf, grad, out, nv), "aligned"), ((dn, lam, [sf[0], sf[1], bad], grad, out, nv), "aligned"),
                      ((dn, lam, sf, [bad, grad[1], grad[2]], out, nv), "aligned"), ((dn, lam, sf, grad, bad, nv), "aligned"),
                      ((dn, lam, sf, grad, out, [nv[0], nv[1], bad]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.interface_nhatf(*args)
    # the patch forms
    fc = L["fcs"][0]
    m = fc.shape[0]
    P = eng.Patch(ctx, n, fc)
    w, psf, nbr = dev(I["lam"][:m]), [dev(s[:m]) for s in L["Sf"]], [dev(g[fc]) for g in I["grad"]]
    ms, th = dev(0.5 + I["lam"][:m]), dev(90.0 * I["lam"][:m])
    po, pv, pg, p1, p2 = E(m), [E(m) for _ in range(3)], E(m), E(m), E(m)
    for kw, why in ((dict(delta_n=0.0), "delta_n"), (dict(delta_n=NAN), "delta_n"),
                    (dict(patch_weights=w), "missing"), (dict(patch_sf=[psf[0], psf[1], None]), "missing"), (dict(nhatf_out=None), "missing"),
                    (dict(nhatfv_out=[pv[0], pv[1], None]), "missing"), (dict(grad=[nbr[0], None, nbr[2]]), "missing"),
                    (dict(patch_weights=w, nbr_grad=nbr, theta_deg=th, patch_magsf=ms), "not coupled"),
                    (dict(theta_deg=th), "patch_magsf"), (dict(gradient_out=pg), "theta_deg missing"), (dict(b12_out=(p1, p2)), "theta_deg missing"),
                    (dict(theta_deg=th, patch_magsf=ms, b12_out=(p1, None)), "together"),
                    (dict(nhatf_out=psf[0]), "alias"), (dict(nhatfv_out=[pv[0], po, pv[2]]), "differ"),
                    (dict(theta_deg=th, patch_magsf=ms, gradient_out=th), "alias"), (dict(theta_deg=th, patch_magsf=ms, gradient_out=pg, b12_out=(pg, p2)), "differ"),
                    (dict(nhatf_out=bad), "aligned"), (dict(grad=[nbr[0], bad, nbr[2]]), "aligned")):
        args = dict(delta_n=dn, grad=nbr, patch_sf=psf, nhatf_out=po, nhatfv_out=pv)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            P.interface_nhatf(**args)
    # the curvature
    B = eng.GradBoundary(addr, L["fcs"], ["other", "other"])
    H = eng.Interface(addr, B)
    nh, bn, vol, K = dev(c["nhatf"]), dev(I["bn"]), dev(I["vol"]), E(n)
    for args, why in (((None, vol, K, bn), "missing"), ((nh, None, K, bn), "missing"), ((nh, vol, K, None), "boundary has faces"), ((nh, vol, None, bn), "missing"),
                      ((nh, vol, vol, bn), "alias"), ((nh, vol, bad, bn), "aligned"), ((nh, bad, K, bn), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            H.curvature(*args)
    other = eng.Addressing(ctx, n, lo, up)
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.Interface(other, B)
    # the force and nearInterface
    dc, Kd, al, corr, fo = dev(I["dc"]), dev(c["K"]), dev(I["alpha"]), dev(I["corr"]), E(nf)
    for args, why in (((None, dc, Kd, al, fo), "missing"), ((lam, None, Kd, al, fo), "missing"), ((lam, dc, None, al, fo), "missing"), ((lam, dc, Kd, None, fo), "missing"),
                      ((lam, dc, Kd, al, None), "missing"), ((lam, dc, Kd, al, dc), "alias"), ((lam, dc, Kd, al, corr, corr), "alias"),
                      ((lam, dc, Kd, al, bad), "aligned"), ((lam, dc, Kd, al, fo, bad), "aligned"), ((lam, dc, bad, al, fo), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.surface_tension_force(I["sigma"], *args)
    pK, pa, pdc = dev(c["K"][fc]), dev(I["alpha"][fc]), dev(I["dc"][:m])
    for args, why in (((None, pdc, Kd, pK, al, pa, po), "missing"), ((w, pdc, Kd, None, al, pa, po), "missing"), ((w, pdc, Kd, pK, al, pa, None), "missing"),
                      ((w, pdc, Kd, pK, al, pa, pa), "alias"), ((w, pdc, Kd, pK, al, pa, bad), "aligned"), ((w, pdc, Kd, pK, al, pa, po, bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            P.surface_tension_force(I["sigma"], *args)
    ni = E(n)
    for args in ((None, ni), (al, None), (al, bad)):
        with pytest.raises(eng.MiError):
            A.near_interface(*args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(y == fill)) for y in [out, spare, po, pg, p1, p2, K, fo, ni] + nv + pv)
    assert same(host(lam), I["lam"]) and same(host(vol), I["vol"]) and same(host(th), 90.0 * I["lam"][:m]) and same(host(dc), I["dc"])
    A.interface_nhatf(dn, lam, sf, grad, out, nv)             # the valid calls after them write every value
    H.curvature(nh, vol, K, bn)
    P.interface_nhatf(dn, nbr, psf, po, nhatfv_out=pv, theta_deg=th, patch_magsf=ms, gradient_out=pg, b12_out=(p1, p2))
    A.surface_tension_force(I["sigma"], lam, dc, Kd, al, fo)
    A.near_interface(al, ni)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == fill)) for y in [out, po, pg, p1, p2, K, fo, ni] + nv + pv)
    H.close(); B.close()
