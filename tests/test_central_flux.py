"""rhoCentralFoam's Kurganov and Tadmor face fluxes on the device (rhoCentralFoam.C:60-185, compressibleCourantNo.H:35-47):
mi_central_scheme_parse, mi_central_flux, mi_patch_central_flux, mi_central_sound_speed and mi_central_courant, bit for bit against the
restatement of tests/central_support.py.  Nothing in the path calls a transcendental function and sqrt and / are correctly rounded: there
is no tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from assembly_support import bits, gpu_env, same, set_face_grid
from central_support import (FLUX_SCHEMES, GRAD_OF, LIMITER_SETS, MESHES, OPT, OUT, SCALARS, TUBE, TUBE_AIR, Hits, boundary_values, courant_products,
                             gather, inputs, lit_flux, literal_faces, literal_sound_speed, mesh, patch_case, restate_flux, restate_internal,
                             restate_patch, restate_reconstruct, restate_sound_speed, restate_walk, slots, tube_mesh, tube_start)
from thermo_support import host_model

EXPORTS = ("mi_central_scheme_parse", "mi_central_flux", "mi_patch_central_flux", "mi_central_sound_speed", "mi_central_courant")
SEED = {"box": 5000, "edge_257": 5100, "isolated": 5200}
FILL = -77.0
_CACHE = {}


def _case(pkg, name, lset):
    """the mesh, its inputs, the interpolated face fields and the fluxes of both schemes, computed once and left unchanged"""
    key = (name, lset)
    if key not in _CACHE:
        if ("mesh", name) not in _CACHE:
            L = mesh(pkg, name)
            _CACHE[("mesh", name)] = (L, inputs(pkg.synthetic, L["n"], SEED[name]))
        L, F = _CACHE[("mesh", name)]
        S = slots(LIMITER_SETS[lset])
        R, V = restate_internal(L, S, F, False)
        _CACHE[key] = dict(L=L, F=F, S=S, V=V, R={"Kurganov": R, "Tadmor": restate_flux(V, L["Sf"], L["magSf"], True)})
    return _CACHE[key]


def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    for word in ("rhoCentralFoam", "Kurganov", "Tadmor", "mi_central_scheme", "mi_central_cells", "mi_central_out", "compressibleCourantNo"):
        assert word in header, word


def test_mirror_has_the_central_fluxes(pkg):
    """foam/miFoam: centralFluxes with the reference's field names is declared and in the library, and the driver is built"""
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    for word in ("class centralFluxes", "phiUp", "phiEp", "amaxSf", "void update(", "CourantNo("):
        assert word in text, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    for name in ("Foam::centralFluxes::centralFluxes(", "Foam::centralFluxes::update(", "Foam::centralFluxes::CourantNo("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name
    assert os.path.exists(os.path.join(PKG, "shockTube"))


def test_parse_accepts_what_the_issue_says(pkg):
    eng = pkg.engine
    for fi, flux in enumerate(FLUX_SCHEMES):
        for names in LIMITER_SETS.values():
            s = eng.central_scheme(flux, *names)
            assert s.flux_scheme == fi
            for got, text in zip((s.rho, s.U, s.T), names):
                want = eng.limiter(text)
                assert (got.kind, got.vector_form, got.bounded, got.k, got.lower, got.upper) == (want.kind, want.vector_form, want.bounded, want.k,
                                                                                                  want.lower, want.upper), text
    # every TVD/NVD name of mi_limiter_parse: scalar and bounded forms in every slot, V forms for U
    for kind in eng.LIMITER_KINDS:
        k = " 0.5" if kind in ("limitedLinear", "limitedCubic", "Gamma") else ""
        s = eng.central_scheme("Kurganov", kind + k, kind + "V" + k, kind + k)
        assert (s.rho.vector_form, s.U.vector_form, s.T.vector_form) == (0, 1, 0)
        assert eng.central_scheme("Tadmor", kind + k, kind + k, kind + k).U.vector_form == 0
    s = eng.central_scheme(" Tadmor ", "vanLeer01", "Minmod", "limitedLimitedLinear 1 0 5")
    assert (s.rho.bounded, s.T.bounded, s.T.upper) == (1, 1, 5.0)


@pytest.mark.parametrize("args,why", [
    (("kurganov", "vanLeer", "vanLeerV", "vanLeer"), "not a valid choice"), (("KT", "vanLeer", "vanLeerV", "vanLeer"), "not a valid choice"),
    (("", "vanLeer", "vanLeerV", "vanLeer"), "not a valid choice"), (("Kurganov Tadmor", "vanLeer", "vanLeerV", "vanLeer"), "not a valid choice"),
    (("Kurganov", "vanLeerV", "vanLeerV", "vanLeer"), r"reconstruct\(rho\).*scalar"), (("Kurganov", "vanLeer", "vanLeerV", "MinmodV"), r"reconstruct\(T\).*scalar"),
    (("Kurganov", "filteredLinear", "vanLeerV", "vanLeer"), r"reconstruct\(rho\).*unknown"), (("Kurganov", "vanLeer", "filteredLinear2V 1 0", "vanLeer"), r"reconstruct\(U\).*unknown"),
    (("Kurganov", "vanLeer", "vanLeerV", "filteredLinear3 1"), r"reconstruct\(T\).*unknown"), (("Kurganov", "linear", "vanLeerV", "vanLeer"), "unknown"),
    (("Kurganov", "vanLeer", "vanLeerV 1", "vanLeer"), "extra"), (("Kurganov", "limitedLinear", "vanLeerV", "vanLeer"), "coefficient"),
    (("Kurganov", "vanLeer", "vanLeer01V", "vanLeer"), "unknown"), (("Kurganov", "vanLeer", "vanLeerV", "limitedVanLeer 2 1"), "lower bound"),
    (("Kurganov", "vanLeer", "vanLeerV", "Gamma 2"), "k should be"), (("Kurganov", "vanLeer", "", "vanLeer"), "empty")])
def test_parse_refuses_and_leaves_out_untouched(pkg, args, why):
    eng = pkg.engine
    with pytest.raises(eng.MiError, match=why):
        eng.central_scheme(*args)
    out = eng.CentralScheme()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    assert eng.lib().mi_central_scheme_parse(*[a.encode() for a in args], C.byref(out)) != 0
    assert bytes(out) == before
    assert "mi_central_scheme_parse" in eng.lib().mi_last_error().decode()


@pytest.mark.parametrize("lset", sorted(LIMITER_SETS))
@pytest.mark.parametrize("name", MESHES)
def test_restatements_agree_and_the_inputs_reach_every_branch(pkg, name, lset):
    c = _case(pkg, name, lset)
    L, F, S = c["L"], c["F"], c["S"]
    lo, up = L["lo"], L["up"]
    d = [x[up] - x[lo] for x in L["C"]]
    for flux in FLUX_SCHEMES:
        hit = Hits()
        lit = literal_faces(S, L["cdw"], gather(F, lo), gather(F, up), d, L["Sf"], L["magSf"], flux == "Tadmor", hit=hit)
        for k in OUT + OPT:
            _eq(c["R"][flux][k], lit[k], (name, lset, flux, k))
            assert np.all(np.isfinite(lit[k])), k
        for key in ("subsonic", "supersonic_pos", "supersonic_neg", "at_rest", "r_guard", "gradf_zero"):
            assert hit.n.get(key, 0) > 0, (name, lset, flux, key, hit.n)
        if lset == "mixed":
            assert hit.n.get("bounded_pos", 0) > 0 and hit.n.get("bounded_neg", 0) > 0, hit.n
    if lset == "mixed":
        assert not S[1]["vec"] and S[2]["bounds"] is not None
    assert not same(c["R"]["Kurganov"]["phi"], c["R"]["Tadmor"]["phi"])


def test_max_of_minus_zero_and_zero_is_plus_zero():
    """the one face on which the inner min of am is -0.0: a gas at rest with c = 0 and Sf < 0 in every component.  The reference's ternary
    gives am = +0.0; ap - am is 0.0 either way and a_pos is the reference's NaN (0/0): the sign of the zero is not visible in an output,
    which is why the seeded meshes do not carry such a face"""
    hit = Hits()
    v = dict(rho=[1.0, 1.0], rhoU=[[0.0] * 3, [0.0] * 3], rPsi=[8e4, 8e4], e=[2.5e5, 2.5e5], c=[0.0, 0.0])
    out = lit_flux(v, [-1.0, -2.0, -0.5], 2.3, False, hit)
    assert hit.n.get("minus_zero") == 1 and hit.n.get("at_rest") == 1
    assert np.isnan(out["a_pos"]) and np.isnan(out["phi"])
    from assembly_support import rmax, rmin
    assert bits(np.array([rmax(-0.0, 0.0), rmin(-0.0, 0.0)])).tolist() == [0, 0]
    V = {k: (np.array([x[0]]), np.array([x[1]])) for k, x in v.items() if k != "rhoU"}
    V["rhoU"] = ([np.zeros(1)] * 3, [np.zeros(1)] * 3)
    assert np.isnan(restate_flux(V, [np.array([-1.0]), np.array([-2.0]), np.array([-0.5])], np.array([2.3]), False)["phi"][0])


@pytest.mark.parametrize("name", MESHES)
def test_each_stated_rounding_changes_a_compared_bit(pkg, name):
    """magSqr contracted or not, three divisions or a reciprocal, the fma interpolate or the coupled two-product form, aSf*p_pos - aSf*p_neg
    or aSf*(p_pos - p_neg), (Cp/Cv)*rPsi or Cp/(Cv*psi): the GPU comparison can tell each pair apart on these inputs"""
    c = _case(pkg, name, "vanLeer")
    L, F, S, V = c["L"], c["F"], c["S"], c["V"]
    base = c["R"]["Kurganov"]
    for alt, keys in (("magsqr_plain", ("phiEp",)), ("reciprocal", ("phi", "phiEp", "amaxSf")), ("asf_factored", ("phiEp",))):
        other = restate_flux(V, L["Sf"], L["magSf"], False, alt=(alt,))
        assert any(not same(other[k], base[k]) for k in keys), alt
        assert all(same(other[k], base[k]) for k in OUT if k not in keys + ("phiUp0", "phiUp1", "phiUp2")), alt
    other, _ = restate_internal(L, S, F, False, coupled_rule=True)
    assert all(not same(other[k], base[k]) for k in OUT)
    u = pkg.synthetic.splitmix_uniform
    Cp, Cv, psi = 1000.0 + 10.0 * u(31, 257), 700.0 + 30.0 * u(32, 257), 1.0e-5 * (1.0 + u(33, 257))
    a, b = restate_sound_speed(Cp, Cv, psi), restate_sound_speed(Cp, Cv, psi, regroup=True)
    assert same(a[0], b[0]) and not same(a[1], b[1])
    lit = literal_sound_speed(Cp, Cv, psi)
    assert same(a[0], lit[0]) and same(a[1], lit[1])


def test_patch_restatements_agree_and_tell_the_rules_apart(pkg):
    P = patch_case(pkg.synthetic)
    for lset in ("vanLeer", "mixed"):
        S = slots(LIMITER_SETS[lset])
        for flux in FLUX_SCHEMES:
            t = flux == "Tadmor"
            want = restate_patch(P, S, t)
            lit = literal_faces(S, P["w"], gather(P["cells"], P["fc"]), P["nbr"], P["pd"], P["Sf"], P["magSf"], t, coupled=True)
            for k in OUT + OPT:
                _eq(want[k], lit[k], ("coupled", lset, flux, k))
    S = slots(LIMITER_SETS["vanLeer"])
    plain = restate_patch(P, S, False, coupled=False)
    one = P["m"]
    lit = literal_faces(S, np.ones(one), P["nbr"], P["nbr"], P["pd"], P["Sf"], P["magSf"], False, coupled=False)   # w = 1: fma(1, v - v, v) = v
    for k in OUT + OPT:
        _eq(plain[k], lit[k], ("plain", k))
    # the coupled rule between equal sides is not the plain rule: w*v + (1 - w)*v rounds
    twin = dict(P, cells={k: ([np.resize(a, P["n"]) for a in v] if isinstance(v, list) else np.resize(v, P["n"])) for k, v in P["nbr"].items()})
    for k, v in P["nbr"].items():
        for a, full in zip(v if isinstance(v, list) else [v], twin["cells"][k] if isinstance(v, list) else [twin["cells"][k]]):
            full[P["fc"]] = a
    eq = restate_patch(twin, S, False)
    assert any(not same(eq[k], plain[k]) for k in OUT)


def test_equal_states_give_the_euler_fluxes(pkg):
    """With equal pos and neg states and a subsonic state the Kurganov fluxes are the physical Euler fluxes: with u = U & Sf, aphiv_pos +
    aphiv_neg = u*a_pos - aSf + u*a_neg + aSf = u, so phi = rho*u, phiUp = rhoU*u + p*Sf and phiEp = (rho*(e + |U|^2/2) + p)*u.  The bound,
    in units of eps = 2^-53 and relative to scale = |u| + c*magSf, which bounds |u|, |ap|, |am|, |aSf| and both aphiv: a_pos carries 4
    roundings (ap, am, their difference, the quotient), a_neg one more, u*a_pos and u*a_neg one more each, aSf = am*a_pos 6, each aphiv so at
    most 8 of scale; two aphiv, the products with the state and the sum add 3; the two dot products (the restatement's fma chain, numpy's
    plain sum here) differ by at most 6 of |U||Sf| < scale: 8 + 8 + 3 + 6 = 25 < 32.  phiUp adds (a_pos*p + a_neg*p)*Sf_k, at most 14 of
    p*|Sf_k|; phiEp adds and takes away aSf*p, two roundings of at most scale*H, and magSqr's contraction, under 3 of H.  So every output
    lies within 32*2^-53 of the Euler flux, relative to scale times the state (plus p*|Sf_k| for phiUp)"""
    u = pkg.synthetic.splitmix_uniform
    m = 300
    rho, rPsi, e, c = 0.6 + 0.8 * u(1, m), 7.0e4 + 2.0e4 * u(2, m), 2.0e5 + 1.0e5 * u(3, m), 300.0 + 80.0 * u(4, m)
    U = [200.0 * (u(5 + d, m) - 0.5) for d in range(3)]
    Sf = [u(8 + d, m) - 0.5 for d in range(3)]
    magSf = np.sqrt(Sf[0] ** 2 + Sf[1] ** 2 + Sf[2] ** 2)
    F = dict(rho=rho, rhoU=[rho * x for x in U], rPsi=rPsi, e=e, c=c)
    R = restate_flux(boundary_values(F), Sf, magSf, False)
    Ur = [x / rho for x in F["rhoU"]]
    un = Ur[0] * Sf[0] + Ur[1] * Sf[1] + Ur[2] * Sf[2]
    p = rho * rPsi
    scale = np.abs(un) + c * magSf                                          # bounds |aphiv_pos| and |aphiv_neg|
    bound = 32 * 2.0 ** -53
    assert np.all(np.abs(un) < c * magSf)
    assert np.max(np.abs(R["phi"] - rho * un) / (scale * rho)) <= bound
    for k in range(3):
        assert np.max(np.abs(R["phiUp%d" % k] - (F["rhoU"][k] * un + p * Sf[k])) / (scale * np.abs(F["rhoU"][k]) + p * np.abs(Sf[k]))) <= bound
    H = rho * (e + 0.5 * (Ur[0] ** 2 + Ur[1] ** 2 + Ur[2] ** 2)) + p
    assert np.max(np.abs(R["phiEp"] - H * un) / (scale * H)) <= bound


def test_the_tube_conserves_mass(pkg):
    """between two steps sum(rho*V) changes by -deltaT*(the boundary fluxes) only, to rounding: 120 cells, each update within a few units
    of 2^-53 of rho*V, so 120*8*2^-53 of the total is a safe bound; the boundary fluxes are zero while the waves are inside"""
    M = host_model("e", "eConst", "const", TUBE_AIR)
    L = tube_mesh()
    W = restate_walk(M, L, slots(LIMITER_SETS["vanLeer"]), False)
    p0, T0 = tube_start(L)
    total = float(np.sum((p0 / (M["R"] * T0)) * L["vol"]))
    for st in W:
        assert abs(st["sum_rhoV"] - (total - TUBE["dt"] * st["bflux"])) <= 120 * 8 * 2.0 ** -53 * total
        total = st["sum_rhoV"]
        assert st["bflux"] == 0.0 and st["co_max"] > 0
    assert not same(W[0]["rho"], W[2]["rho"]) and np.max(np.abs(W[2]["rhoU0"])) > 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _shift(dev, a, shift):
    """the values at an address 16 bytes further on"""
    return dev(np.concatenate([np.zeros(2), a]))[2:] if shift else dev(a)


def _cells(eng, dev, F, S, shift=False, grads=True):
    put = lambda a: _shift(dev, a, shift)
    kw = dict(rho=put(F["rho"]), rhoU=[put(x) for x in F["rhoU"]], rPsi=put(F["rPsi"]), e=put(F["e"]), c=put(F["c"]))
    if grads:
        kw.update(grad_rho=[put(x) for x in F["gRho"]], grad_rPsi=[put(x) for x in F["gRPsi"]], grad_e=[put(x) for x in F["gE"]],
                  grad_c=[put(x) for x in F["gC"]])
        if S[1]["vec"]:
            kw.update(grad_rhoU=[put(x) for x in F["gRhoU"]])
        else:
            kw.update(lim_U=put(F["limU"]), grad_lim_U=[put(x) for x in F["gLimU"]])
    return eng.central_cells(**kw), kw


def _outs(eng, E, m, opt, shift=False):
    mk = (lambda: E(m + 2)[2:]) if shift else (lambda: E(m))
    t = dict(phi=mk(), phiUp=[mk() for _ in range(3)], phiEp=mk(), amaxSf=mk())
    if opt:
        t.update(a_pos=mk(), aU=[mk() for _ in range(3)])
    return eng.central_out(**t), t


def _check(host, t, want, opt, tag):
    got = dict(phi=t["phi"], phiEp=t["phiEp"], amaxSf=t["amaxSf"], **{"phiUp%d" % k: t["phiUp"][k] for k in range(3)})
    if opt:
        got.update(a_pos=t["a_pos"], **{"aU%d" % k: t["aU"][k] for k in range(3)})
    for k, v in got.items():
        _eq(host(v), want[k], tag + (k,))


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_central_flux_on_the_three_meshes(pkg, monkeypatch, name, blocks):
    """every limiter set, Kurganov and Tadmor, with and without a_pos and aU, caller-order and ordered addressing, aligned arrays and arrays
    16 bytes further on; MI_FACE_GRID at its default and forced to 1 and 3 workgroups"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=float("nan"))
    for lset in sorted(LIMITER_SETS):
        c = _case(pkg, name, lset)
        L, F, S = c["L"], c["F"], c["S"]
        nf = L["lo"].shape[0]
        for aname, addr in _addressings(eng, ctx, L):
            A = eng.Assembly(addr)
            for shift in (False, True):
                cells, keep = _cells(eng, dev, F, S, shift)
                cdw, sf, ms, cc = _shift(dev, L["cdw"], shift), [_shift(dev, s, shift) for s in L["Sf"]], _shift(dev, L["magSf"], shift), [dev(x) for x in L["C"]]
                for flux in FLUX_SCHEMES:
                    scheme = eng.central_scheme(flux, *LIMITER_SETS[lset])
                    for opt in (False, True):
                        out, t = _outs(eng, E, nf, opt, shift)
                        A.central_flux(scheme, cdw, sf, ms, cells, cc, out)
                        _check(host, t, c["R"][flux], opt, (name, blocks, lset, aname, shift, flux, opt))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_the_unfused_start_gives_the_interpolated_fields(pkg, name):
    """mi_limited_weights with flux arrays of +1 and -1, then mi_face_interpolate: the engine's own entries, pinned by the compiled reference,
    reproduce the ten interpolated face fields the restatement continues from"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=float("nan"))
    for lset in ("vanLeer", "mixed"):
        c = _case(pkg, name, lset)
        L, F, S, V = c["L"], c["F"], c["S"], c["V"]
        nf = L["lo"].shape[0]
        A = eng.Assembly(eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
        cdw, cc = dev(L["cdw"]), [dev(x) for x in L["C"]]
        names = LIMITER_SETS[lset]
        for di, fl in enumerate((1.0, -1.0)):
            flux = dev(np.full(nf, fl))
            for fname in SCALARS:
                w, out = E(nf), E(nf)
                A.limited_weights(names[0 if fname == "rho" else 2], cdw, flux, [dev(F[fname])], [dev(g) for g in F[GRAD_OF[fname]]], cc, w)
                A.face_interpolate(w, dev(F[fname]), out)
                _eq(host(out), V[fname][di], (name, lset, fname, fl))
            w = E(nf)
            if S[1]["vec"]:
                A.limited_weights(names[1], cdw, flux, [dev(x) for x in F["rhoU"]], [dev(g) for g in F["gRhoU"]], cc, w)
            else:
                A.limited_weights(names[1], cdw, flux, [dev(F["limU"])], [dev(g) for g in F["gLimU"]], cc, w)
            for k in range(3):
                out = E(nf)
                A.face_interpolate(w, dev(F["rhoU"][k]), out)
                _eq(host(out), V["rhoU"][di][k], (name, lset, "rhoU", k, fl))


@pytest.mark.gpu
def test_the_patch_forms_on_429_faces(pkg):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=float("nan"))
    P = patch_case(pkg.synthetic)
    m = P["m"]
    patch = eng.Patch(ctx, P["n"], P["fc"])
    sf, ms, w, pd = [dev(s) for s in P["Sf"]], dev(P["magSf"]), dev(P["w"]), [dev(x) for x in P["pd"]]
    for lset in ("vanLeer", "mixed"):
        S = slots(LIMITER_SETS[lset])
        own, k1 = _cells(eng, dev, P["cells"], S)
        nbr, k2 = _cells(eng, dev, P["nbr"], S)
        vals, k3 = _cells(eng, dev, P["nbr"], S, grads=False)
        for flux in FLUX_SCHEMES:
            scheme = eng.central_scheme(flux, *LIMITER_SETS[lset])
            t = flux == "Tadmor"
            for opt in (False, True):
                out, o = _outs(eng, E, m, opt)
                patch.central_flux(scheme, sf, ms, own, out, patch_weights=w, nbr=nbr, patch_delta=pd)
                _check(host, o, restate_patch(P, S, t), opt, ("coupled", lset, flux, opt))
                out, o = _outs(eng, E, m, opt)
                patch.central_flux(scheme, sf, ms, vals, out)
                _check(host, o, restate_patch(P, S, t, coupled=False), opt, ("plain", lset, flux, opt))
    # the plain form takes the plain path's bits where the coupled path between equal sides would round
    S = slots(LIMITER_SETS["vanLeer"])
    V = restate_reconstruct(S, P["w"], P["nbr"], P["nbr"], P["pd"], True)
    coupled_equal = restate_flux(V, P["Sf"], P["magSf"], False)
    plain = restate_patch(P, S, False, coupled=False)
    assert any(not same(coupled_equal[k], plain[k]) for k in OUT)
    out, o = _outs(eng, E, m, False)
    vals, k3 = _cells(eng, dev, P["nbr"], S, grads=False)
    patch.central_flux(eng.central_scheme("Kurganov", *LIMITER_SETS["vanLeer"]), sf, ms, vals, out)
    _check(host, o, plain, False, ("plain, equal sides",))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_sound_speed(pkg, n):
    eng, ctx, dev, host, E = gpu_env(pkg, fill=float("nan"))
    u = pkg.synthetic.splitmix_uniform
    Cp, Cv, psi = 1000.0 + 10.0 * u(41, n), 700.0 + 30.0 * u(42, n), 1.0e-5 * (1.0 + u(43, n))
    want = restate_sound_speed(Cp, Cv, psi)
    A = eng.Assembly(eng.Addressing(ctx, 2, np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)))
    for odd in (False, True):                                               # 16-byte aligned: two cells a thread; 8 bytes on: one by one
        put = (lambda a: dev(np.concatenate([[0.0], a]))[1:]) if odd else dev
        rPsi, c = (E(n + 1)[1:], E(n + 1)[1:]) if odd else (E(n), E(n))
        A.central_sound_speed(put(Cp), put(Cv), put(psi), rPsi, c)
        _eq(host(rPsi), want[0], (n, odd, "rPsi")); _eq(host(c), want[1], (n, odd, "c"))


@pytest.mark.gpu
def test_courant_against_the_engines_own_reductions(pkg):
    """max and sum equal to mi_min_max and mi_sum over the host-formed products, bit for bit; the boundary takes part in the max only"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    u = pkg.synthetic.splitmix_uniform
    for name in MESHES:
        c = _case(pkg, name, "vanLeer")
        L = c["L"]
        nf, nb = L["lo"].shape[0], 37
        A = eng.Assembly(eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
        dc, ms, am = 0.5 + u(51, nf), L["magSf"], c["R"]["Kurganov"]["amaxSf"]
        prod, quot = courant_products(dc, ms, am)
        for case in ("inside", "boundary_max", "boundary_huge"):
            bdc, bms, bam = 0.5 + u(52, nb), 0.5 + u(53, nb), float(np.max(am)) * u(54, nb) * 0.01
            if case == "boundary_max":
                bam[11] = 3.0 * float(np.max(quot)) * bms[11] / bdc[11]
            if case == "boundary_huge":
                bam[:] = 1.0e6 * float(np.max(am))                           # a boundary sum that must be ignored, every face above the internal ones
            _, bquot = courant_products(bdc, bms, bam)
            both = np.concatenate([quot, bquot])
            want_max = A.min_max(dev(both))[1]
            want_sum = ctx.sum(dev(prod))
            got = A.central_courant(dev(dc), dev(ms), dev(am), dev(bdc), dev(bms), dev(bam))
            assert bits(np.array(got)).tolist() == bits(np.array([want_max, want_sum])).tolist(), (name, case, got, want_max, want_sum)
            assert want_max == float(np.max(both))
            assert (int(np.argmax(both)) >= nf) == (case != "inside"), (name, case)
        got = A.central_courant(dev(dc), dev(ms), dev(am))                  # no boundary faces
        assert bits(np.array(got)).tolist() == bits(np.array([A.min_max(dev(quot))[1], ctx.sum(dev(prod))])).tolist()
    none = np.zeros(0, dtype=np.int32)
    A = eng.Assembly(eng.Addressing(ctx, 3, none, none))
    assert A.central_courant(None, None, None, dev(np.ones(4)), dev(np.ones(4)), dev(np.ones(4))) == (0.0, 0.0)   # if (mesh.nInternalFaces())
    assert A.central_courant(None, None, None) == (0.0, 0.0)


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
    eng, ctx, dev, host, E = gpu_env(pkg, fill=FILL)
    c = _case(pkg, "box", "vanLeer")
    L, F, S = c["L"], c["F"], c["S"]
    nf, n = L["lo"].shape[0], L["n"]
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    A = eng.Assembly(addr)
    scheme = eng.central_scheme("Kurganov", *LIMITER_SETS["vanLeer"])
    scalarU = eng.central_scheme("Kurganov", "vanLeer", "vanLeer", "vanLeer")
    cdw, sf, ms, cc = dev(L["cdw"]), [dev(s) for s in L["Sf"]], dev(L["magSf"]), [dev(x) for x in L["C"]]
    _, kw = _cells(eng, dev, F, S)
    _, t = _outs(eng, E, nf, True)
    spare = E(nf + 1)
    off8, bad = spare[1:], Misaligned(spare)

    def call(scheme=scheme, cdw=cdw, sf=sf, ms=ms, cc=cc, cells=None, out=None, **change):
        k, o = dict(kw), dict(t)
        for key, v in change.items():
            (k if key in k or key in ("lim_U", "grad_lim_U", "grad_rhoU") else o)[key] = v
        A.central_flux(scheme, cdw, sf, ms, eng.central_cells(**k) if cells is None else cells, cc, eng.central_out(**o) if out is None else out)

    broken = eng.central_scheme("Kurganov", *LIMITER_SETS["vanLeer"]); broken.flux_scheme = 2
    vrho = eng.central_scheme("Kurganov", *LIMITER_SETS["vanLeer"]); vrho.rho.vector_form = 1
    kind12 = eng.central_scheme("Kurganov", *LIMITER_SETS["vanLeer"]); kind12.T.kind = 12
    three = lambda xs, i, v: [v if j == i else x for j, x in enumerate(xs)]
    for change, why in ((dict(scheme=broken), "invalid mi_central_scheme"), (dict(scheme=vrho), "invalid mi_central_scheme"), (dict(scheme=kind12), "invalid mi_central_scheme"),
                        (dict(scheme=None), "scheme is missing"),
                        (dict(cdw=None), "missing"), (dict(ms=None), "missing"), (dict(sf=three(sf, 1, None)), "missing"), (dict(cc=three(cc, 2, None)), "missing"),
                        (dict(rho=None), "missing"), (dict(rhoU=three(kw["rhoU"], 0, None)), "missing"), (dict(c=None), "missing"),
                        (dict(grad_e=three(kw["grad_e"], 1, None)), "missing"), (dict(grad_rhoU=kw["grad_rhoU"][:8]), "missing"),
                        (dict(phi=None), "missing"), (dict(phiUp=three(t["phiUp"], 2, None)), "missing"), (dict(amaxSf=None), "missing"),
                        (dict(cdw=off8), "aligned"), (dict(sf=three(sf, 0, off8)), "aligned"), (dict(ms=off8), "aligned"), (dict(phiEp=off8), "aligned"),
                        (dict(aU=three(t["aU"], 1, off8)), "aligned"), (dict(e=bad), "aligned"), (dict(cc=three(cc, 0, bad)), "aligned"),
                        (dict(phi=cdw), "alias"), (dict(phiEp=kw["e"]), "alias"), (dict(a_pos=ms), "alias"), (dict(phiUp=three(t["phiUp"], 0, t["phi"])), "differ"),
                        (dict(aU=three(t["aU"], 2, t["a_pos"])), "differ"),
                        (dict(a_pos=None), "together"), (dict(aU=three(t["aU"], 0, None)), "together"), (dict(aU=None), "together"),
                        (dict(scheme=scalarU), "lim_u"), (dict(scheme=scalarU, lim_U=dev(F["limU"])), "lim_u"),
                        (dict(cells=None, out=None, scheme=scheme, sf=None), "missing")):
        with pytest.raises(eng.MiError, match=why) as err:
            call(**change)
        assert "mi_central_flux" in str(err.value), str(err.value)
    with pytest.raises(eng.MiError, match="missing"):
        A.central_flux(scheme, cdw, sf, ms, None, cc, eng.central_out(**t))
    with pytest.raises(eng.MiError, match="missing"):
        A.central_flux(scheme, cdw, sf, ms, eng.central_cells(**kw), cc, None)
    # the patch forms
    P = patch_case(pkg.synthetic)
    m = P["m"]
    patch = eng.Patch(ctx, P["n"], P["fc"])
    psf, pms, w, pd = [dev(s) for s in P["Sf"]], dev(P["magSf"]), dev(P["w"]), [dev(x) for x in P["pd"]]
    own, k1 = _cells(eng, dev, P["cells"], S)
    nbr, k2 = _cells(eng, dev, P["nbr"], S)
    vals, k3 = _cells(eng, dev, P["nbr"], S, grads=False)
    _, po = _outs(eng, E, m, True)
    pout = eng.central_out(**po)
    for args, kwargs, why in (((broken, psf, pms, vals, pout), {}, "invalid mi_central_scheme"), ((scheme, three(psf, 0, None), pms, vals, pout), {}, "missing"),
                              ((scheme, psf, None, vals, pout), {}, "missing"), ((scheme, psf, pms, None, pout), {}, "missing"), ((scheme, psf, pms, vals, None), {}, "missing"),
                              ((scheme, psf, pms, eng.central_cells(**dict(k3, e=None)), pout), {}, "missing"),
                              ((scheme, psf, pms, vals, eng.central_out(**dict(po, phi=None))), {}, "missing"),
                              ((scheme, psf, pms, vals, eng.central_out(**dict(po, a_pos=None))), {}, "together"),
                              ((scheme, psf, pms, vals, eng.central_out(**dict(po, phi=pms))), {}, "alias"),
                              ((scheme, psf, pms, vals, eng.central_out(**dict(po, phiEp=po["phi"]))), {}, "differ"),
                              ((scheme, psf, pms, vals, eng.central_out(**dict(po, phi=bad))), {}, "aligned"),
                              ((scheme, psf, Misaligned(pms), vals, pout), {}, "aligned"),
                              ((scheme, psf, pms, own, pout), dict(patch_weights=w), "coupled patch needs"),
                              ((scheme, psf, pms, own, pout), dict(patch_weights=w, nbr=nbr), "coupled patch needs"),
                              ((scheme, psf, pms, vals, pout), dict(patch_weights=w, nbr=nbr, patch_delta=pd), "missing"),
                              ((scheme, psf, pms, own, pout), dict(patch_weights=w, nbr=vals, patch_delta=pd), "missing"),
                              ((scalarU, psf, pms, own, pout), dict(patch_weights=w, nbr=nbr, patch_delta=pd), "lim_u")):
        with pytest.raises(eng.MiError, match=why) as err:
            patch.central_flux(*args, **kwargs)
        assert "mi_patch_central_flux" in str(err.value), str(err.value)
    # the cell pass and the reduction
    Cp, Cv, psi, r1, r2 = dev(1000.0 + F["rho"]), dev(700.0 + F["rho"]), dev(1e-5 * F["rho"]), E(n), E(n)
    for args, why in (((None, Cv, psi, r1, r2), "missing"), ((Cp, Cv, None, r1, r2), "missing"), ((Cp, Cv, psi, None, r2), "missing"), ((Cp, Cv, psi, r1, None), "missing"),
                      ((Cp, Cv, psi, psi, r2), "alias"), ((Cp, Cv, psi, r1, Cp), "alias"), ((Cp, Cv, psi, r1, r1), "differ"), ((Cp, bad, psi, r1, r2), "aligned"),
                      ((Cp, Cv, psi, r1, bad), "aligned")):
        with pytest.raises(eng.MiError, match=why) as err:
            A.central_sound_speed(*args)
        assert "mi_central_sound_speed" in str(err.value)
    dc, am, b = dev(0.5 + L["cdw"]), dev(c["R"]["Kurganov"]["amaxSf"]), dev(np.ones(4))
    for args, why in (((None, ms, am), "missing"), ((dc, None, am), "missing"), ((dc, ms, None), "missing"), ((dc, ms, am, b, None, b), "missing"),
                      ((dc, ms, am, None, b, b), "missing"), ((off8, ms, am), "aligned"), ((dc, ms, off8), "aligned"), ((dc, ms, am, b, bad, b), "aligned")):
        with pytest.raises(eng.MiError, match=why) as err:
            A.central_courant(*args)
        assert "mi_central_courant" in str(err.value)
    torch.cuda.synchronize()
    outs = [t["phi"], t["phiEp"], t["amaxSf"], t["a_pos"], po["phi"], po["phiEp"], po["amaxSf"], po["a_pos"], spare, r1, r2] + t["phiUp"] + t["aU"] + po["phiUp"] + po["aU"]
    assert all(bool(torch.all(y == FILL)) for y in outs)
    assert same(host(cdw), L["cdw"]) and same(host(kw["e"]), F["e"]) and same(host(ms), L["magSf"]) and same(host(pms), P["magSf"])
    call()                                                                  # the valid calls after them write every value
    patch.central_flux(scheme, psf, pms, vals, pout)
    A.central_sound_speed(Cp, Cv, psi, r1, r2)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == FILL)) for y in outs if y is not spare)
    # a mesh without internal faces is legal and launches nothing
    none = np.zeros(0, dtype=np.int32)
    A0 = eng.Assembly(eng.Addressing(ctx, 3, none, none))
    A0.central_flux(scheme, None, None, None, None, None, eng.central_out())


def _tube_device(pkg, eng, ctx, dev, host, E, M, K, L, S, lset, flux):
    """three steps of the inviscid rhoCentralFoam.C on the device; host glue, where the engine has no entry: the products of the two-face
    boundary fields and e = rhoE/rho - 0.5*magSqr(U) (torch, every operator rounded; U_y = U_z = 0 on the tube)"""
    import torch
    n, nf = L["n"], L["lo"].shape[0]
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    A = eng.Assembly(addr)
    patches = [eng.Patch(ctx, n, fc) for fc in L["fcs"]]
    bnd = eng.GradBoundary(addr, L["fcs"], ["other", "other"])
    scheme = eng.central_scheme(flux, *LIMITER_SETS[lset])
    cdw, sf, ms, cc, vol, dcf = dev(L["cdw"]), [dev(s) for s in L["Sf"]], dev(L["magSf"]), [dev(x) for x in L["C"]], dev(L["vol"]), dev(L["dc"])
    bsf, bms, bdc = [dev(s) for s in L["bSf"]], dev(L["bMagSf"]), dev(L["bdc"])
    p0, T0 = tube_start(L)
    p, T = dev(p0), dev(T0)
    e, psi, mu, alpha = E(n), E(n), E(n), E(n)
    A.thermo_he(K, p, T, e)
    A.thermo_calculate(K, e, p, T, T, psi, mu, alpha)
    U = [torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    rho = psi * p
    rhoU = [rho * u for u in U]
    rhoE = rho * (e + 0.5 * (U[0] * U[0] + U[1] * U[1] + U[2] * U[2]))
    bcells = torch.from_numpy(L["bcells"]).to("cuda:0")
    take = lambda x: x[bcells].contiguous()                                 # zeroGradient: the cell's value
    b = dict(p=take(p), T=take(T), e=take(e), psi=take(psi), U=[take(u) for u in U])
    b["rho"] = b["psi"] * b["p"]
    b["rhoU"] = [b["rho"] * u for u in b["U"]]
    rdt = 1.0 / TUBE["dt"]
    states = []

    def grad(x, bx):
        ssf, g = E(nf), [E(n) for _ in range(3)]
        A.face_interpolate(cdw, x, ssf)
        A.gauss_grad(sf, ssf, None, g)
        for k in range(3):
            for i, pt in enumerate(patches):
                pt.add_product(bsf[k][i:i + 1].clone(), bx[i:i + 1].clone(), g[k])
            A.vec_div(g[k], vol, g[k])
        return g

    def solve(old, fl, bfl):
        diag, source, dv = E(n), E(n), E(n)
        A.fvm_ddt_euler(rdt, 1.0, vol, old, diag, source)
        A.surface_integrate(fl, None, dv)
        for i, pt in enumerate(patches):
            pt.add(bfl[i:i + 1].clone(), dv)
        A.vec_div(dv, vol, dv)
        A.submul(vol, dv, source)
        A.vec_div(source, diag, source)
        return source

    for _ in range(TUBE["steps"]):
        Cp, Cv, rPsi, c = E(n), E(n), E(n), E(n)
        A.thermo_property(K, "Cp", p, T, Cp); A.thermo_property(K, "Cv", p, T, Cv)
        A.central_sound_speed(Cp, Cv, psi, rPsi, c)
        bCp, bCv, brPsi, bc = E(2), E(2), E(2), E(2)
        A.thermo_property(K, "Cp", b["p"], b["T"], bCp); A.thermo_property(K, "Cv", b["p"], b["T"], bCv)
        A.central_sound_speed(bCp, bCv, b["psi"], brPsi, bc)
        G = dict(grad_rho=grad(rho, b["rho"]), grad_rPsi=grad(rPsi, brPsi), grad_e=grad(e, b["e"]), grad_c=grad(c, bc),
                 grad_rhoU=[g for k in range(3) for g in grad(rhoU[k], b["rhoU"][k])])   # kept: the struct holds addresses, not tensors
        cells = eng.central_cells(rho=rho, rhoU=rhoU, rPsi=rPsi, e=e, c=c, **G)
        out, t = _outs(eng, E, nf, False)
        A.central_flux(scheme, cdw, sf, ms, cells, cc, out)
        bout, bt = _outs(eng, E, 2, False)
        for i, pt in enumerate(patches):                                    # one face each: the outputs are slices of the boundary arrays
            one = lambda x: x[i:i + 1]
            pt.central_flux(scheme, [one(s) for s in bsf], one(bms), eng.central_cells(rho=one(b["rho"]), rhoU=[one(x) for x in b["rhoU"]], rPsi=one(brPsi),
                                                                                     e=one(b["e"]), c=one(bc)),
                            eng.central_out(phi=one(bt["phi"]), phiUp=[one(x) for x in bt["phiUp"]], phiEp=one(bt["phiEp"]), amaxSf=one(bt["amaxSf"])))
        co = A.central_courant(dcf, ms, t["amaxSf"], bdc, bms, bt["amaxSf"])
        rho = solve(rho, t["phi"], bt["phi"])
        rhoU = [solve(rhoU[k], t["phiUp"][k], bt["phiUp"][k]) for k in range(3)]
        for k in range(3):
            U[k] = E(n)
            A.vec_div(rhoU[k], rho, U[k])
        b["rho"] = take(rho)
        b["U"] = [take(u) for u in U]
        b["rhoU"] = [b["rho"] * u for u in b["U"]]
        rhoE = solve(rhoE, t["phiEp"], bt["phiEp"])
        q = E(n)
        A.vec_div(rhoE, rho, q)
        e = q - 0.5 * (U[0] * U[0] + U[1] * U[1] + U[2] * U[2])
        b["e"] = take(e)
        A.thermo_calculate(K, e, p, T, T, psi, mu, alpha)
        bmu, balpha = E(2), E(2)
        A.thermo_calculate_boundary(bnd, K, [2, 2], b["e"], b["p"], b["T"], b["psi"], bmu, balpha)
        pn = E(n)
        A.vec_div(rho, psi, pn)
        p = pn
        b["p"] = take(p)
        b["rho"] = b["psi"] * b["p"]
        states.append(dict(rho=host(rho), rhoU0=host(rhoU[0]), rhoE=host(rhoE), e=host(e), T=host(T).copy(), p=host(p), psi=host(psi).copy(),
                           phi=host(t["phi"]), phiEp=host(t["phiEp"]), amaxSf=host(t["amaxSf"]), bphi=host(bt["phi"]), co=co))
    bnd.close()
    return states


WALK_KEYS = ("phi", "phiEp", "amaxSf", "bphi", "rho", "rhoU0", "rhoE", "e", "T", "psi", "p")


@pytest.mark.gpu
def test_walk_through_the_c_abi(pkg):
    """the 120-cell shock tube (left p = 1e5, T = 348.4; right p = 1e4, T = 278.2; eConst, perfect gas, vanLeer / vanLeerV), three steps on
    the device with gradients from mi_gauss_grad, bit for bit the restated walk; the Courant reduction against numpy's max and the engine's
    sum of the stored products"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=float("nan"))
    M, K = host_model("e", "eConst", "const", TUBE_AIR), eng.thermo_model(energy="e", thermo="eConst", transport="const", **TUBE_AIR)
    L = tube_mesh()
    S = slots(LIMITER_SETS["vanLeer"])
    want = restate_walk(M, L, S, False)
    got = _tube_device(pkg, eng, ctx, dev, host, E, M, K, L, S, "vanLeer", "Kurganov")
    for step, (g, w) in enumerate(zip(got, want)):
        for k in WALK_KEYS:
            _eq(g[k], w[k], (step, k))
        assert g["co"][0] == w["co_max"], (step, g["co"], w["co_max"])
        assert g["co"][1] == ctx.sum(dev(w["co_sum_terms"]))


@pytest.mark.gpu
def test_mirror_driver_reproduces_the_walk(pkg, tmp_path):
    """foam/shockTube.C in a process of its own: the mirror's centralFluxes and hePsiThermo on the same tube, bit for bit the restated walk"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    M = host_model("e", "eConst", "const", TUBE_AIR)
    L = tube_mesh()
    want = restate_walk(M, L, slots(LIMITER_SETS["vanLeer"]), False)
    dst = tmp_path / "out.bin"
    r = subprocess.run([os.path.join(PKG, "shockTube"), str(TUBE["n"]), str(TUBE["steps"]), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, dtype=np.float64)
    n, nf = L["n"], L["lo"].shape[0]
    at = 0
    for step, W in enumerate(want):
        for k, m in (("phi", nf), ("phiEp", nf), ("amaxSf", nf), ("bphi", 2), ("rho", n), ("rhoU0", n), ("rhoE", n), ("e", n), ("T", n), ("psi", n), ("p", n)):
            _eq(got[at:at + m], W[k], ("driver", step, k))
            at += m
        assert got[at] == 0.5 * W["co_max"] * TUBE["dt"], (step, got[at], W["co_max"])
        assert got[at + 1] == 0.5 * (ctx.sum(dev(W["co_sum_terms"])) / float(np.sum(L["magSf"]))) * TUBE["dt"]
        at += 2
    assert at == got.shape[0]
