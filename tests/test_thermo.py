"""The thermo update of rhoPimpleFoam on the device (hePsiThermo.C:31-171, heRhoThermo.C:31-177, heThermo.C:131-145, thermoI.H:42-90):
mi_thermo_model_init, mi_thermo_calculate, mi_thermo_calculate_boundary, mi_thermo_he and mi_thermo_property, bit for bit against the
restatement of tests/thermo_support.py.  NaN is compared by position: its sign and payload are the arithmetic unit's own."""
import os
import re
import subprocess

import numpy as np
import pytest

from assembly_support import gpu_env, set_face_grid
from thermo_support import (AIR, FULL_GRID, MODELS, N_ALL, N_BASE, NAN, PROPERTIES, SETS, boundary_inputs, engine_model, host_model, inputs,
                            literal_boundary, literal_calculate, literal_property, patch_kinds, restate_boundary, restate_calculate,
                            restate_property, restate_walk, same_bits, v_cp, v_he, walk_rule)
from turbulence_support import ALL_MESHES, MESHES, mesh

EXPORTS = ("mi_thermo_model_init", "mi_thermo_calculate", "mi_thermo_calculate_boundary", "mi_thermo_he", "mi_thermo_property")
OUT = ("T", "psi", "mu", "alpha", "rho")
SEED = 3100
BSEED = {"box": 3200, "edge_257": 3240, "isolated": 3280, "big": 3320}
THREE = (("h", "hConst", "sutherland"), ("e", "janaf", "sutherland"), ("e", "eConst", "const"))   # he and property: FULL_GRID plus one
_CACHE = {}


def _id(m):
    return "-".join(m)


def _case(pkg, model, numbers="air", n=N_BASE, rho_form=2):
    """the model, its inputs and the restated results, computed once and left unchanged"""
    key = (model, numbers, n, rho_form)
    if key not in _CACHE:
        M = host_model(*model, SETS[numbers])
        I = inputs(pkg.synthetic, M, n, SEED)
        _CACHE[key] = dict(M=M, I=I, R=restate_calculate(M, I["he"], I["p"], I["t0"], rho_form))
    return _CACHE[key]


def _bcase(pkg, model, name, rho_form=2):
    key = (model, name, rho_form)
    if key not in _CACHE:
        M = host_model(*model, AIR)
        L = mesh(pkg, name)
        sizes, B = boundary_inputs(pkg.synthetic, M, L, BSEED[name])
        kinds = patch_kinds(L)
        _CACHE[key] = dict(M=M, L=L, sizes=sizes, B=B, kinds=kinds, R=restate_boundary(M, kinds, sizes, B, rho_form),
                           Rhe=restate_boundary(M, kinds, sizes, B, rho_form, t_into_he=True))
    return _CACHE[key]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    for word in ("hePsiThermo", "heRhoThermo", "janaf", "sutherland", "mi_thermo_model"):
        assert word in header, word


@pytest.mark.parametrize("numbers", sorted(SETS))
def test_model_against_the_host_formulas(pkg, numbers):
    for model in MODELS:
        M, K = host_model(*model, SETS[numbers]), engine_model(pkg.engine, *model, SETS[numbers])
        for name, want in M.items():
            got = getattr(K, name)
            got = tuple(got) if hasattr(got, "__len__") else got
            assert same_bits(np.atleast_1d(np.array(got, dtype=np.float64)), np.atleast_1d(np.array(want, dtype=np.float64))), (model, name)
    assert pkg.engine.THERMO_DEFAULTS == dict(AIR, energy="sensibleEnthalpy", thermo="hConst", transport="const")


def test_model_refusals(pkg):
    eng = pkg.engine
    inf = float("inf")
    bad = [dict(W=0.0), dict(W=-28.9), dict(W=NAN), dict(Cp=0.0), dict(Cp=inf), dict(Hf=NAN), dict(Hf=inf), dict(mu=0.0), dict(Pr=-0.7), dict(Pr=NAN),
           dict(thermo="eConst", Cv=0.0), dict(thermo="eConst", Cv=-1.0), dict(thermo="eConst", Hf=NAN),
           dict(transport="sutherland", As=0.0), dict(transport="sutherland", Ts=-116.0), dict(transport="sutherland", Ts=NAN),
           dict(thermo="janaf", Tlow=0.0), dict(thermo="janaf", Thigh=inf), dict(thermo="janaf", Tcommon=NAN),
           dict(thermo="janaf", highCpCoeffs=(1.0, 2.0, NAN, 0.0, 0.0, 0.0, 0.0)), dict(thermo="janaf", lowCpCoeffs=(inf, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0))]
    for given in bad:
        with pytest.raises(eng.MiError, match="finite"):
            eng.thermo_model(**given)
    for given, what in ((dict(Tlow=6000.0), "Tlow >= Thigh"), (dict(Tlow=7000.0), "Tlow >= Thigh"), (dict(Tcommon=200.0), "Tcommon <= Tlow"),
                        (dict(Tcommon=100.0), "Tcommon <= Tlow"), (dict(Tcommon=6001.0), "Tcommon > Thigh")):
        with pytest.raises(eng.MiError, match=what):
            eng.thermo_model(thermo="janaf", **given)
    eng.thermo_model(Hf=-1.0e6)                                    # Hf and the janaf coefficients may have any finite sign
    eng.thermo_model(thermo="janaf", Tcommon=6000.0)               # Tcommon == Thigh passes checkInputData
    with pytest.raises(TypeError, match="unknown name Cmu"):
        eng.thermo_model(Cmu=0.09)
    for given in (dict(energy="absoluteEnthalpy"), dict(thermo="hPolynomial"), dict(transport="polynomial")):
        with pytest.raises(eng.MiError, match="unknown"):
            eng.thermo_model(**given)
    for given, what in ((dict(energy=2), "energy form"), (dict(thermo=3), "thermodynamics"), (dict(transport=-1), "transport")):
        with pytest.raises(eng.MiError, match=what):
            eng.thermo_model(**given)


@pytest.mark.parametrize("numbers", sorted(SETS))
@pytest.mark.parametrize("model", MODELS, ids=_id)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg, model, numbers):
    c = _case(pkg, model, numbers)
    M, I, R = c["M"], c["I"], c["R"]
    lit = literal_calculate(M, I["he"], I["p"], I["t0"], 2)
    assert all(same_bits(lit[k], R[k]) for k in OUT) and np.array_equal(lit["iters"], R["iters"])
    for form in (0, 1):
        a, b = literal_calculate(M, I["he"], I["p"], I["t0"], form), restate_calculate(M, I["he"], I["p"], I["t0"], form)
        assert all(same_bits(a[k], b[k]) for k in OUT)
    it, T = R["iters"], R["T"]
    assert np.any(it == 1) and np.any(it == 2)
    neg, nan_he = I["t0"] <= 0, np.isnan(I["he"])
    assert np.any(neg) and np.all(it[neg] == 102) and np.all(np.isnan(T[neg]))
    assert np.any(nan_he) and np.all(it[nan_he] == 1) and np.all(np.isnan(T[nan_he]))
    plain = ~neg & ~nan_he
    assert np.all(np.isfinite(T[plain])) and np.all(it[plain] < 10)
    if model[1] == "janaf":
        assert np.any((it >= 3) & (it < 102))
        assert np.any(R["lo_hit"] & (T == M["Tlow"])) and np.any(R["hi_hit"] & (T == M["Thigh"]))
        assert np.any(R["crossed"] & plain)
        assert np.any(T[plain] < M["Tcommon"]) and np.any(T[plain] > M["Tcommon"])
    else:                                                          # the identity limit: Newton on a straight line lands within one step
        assert np.all(it[plain] <= 2)
    # away from the clamp the iteration finds the temperature he was formed from, to its own tolerance
    inside = plain & ~R["lo_hit"] & ~R["hi_hit"]
    assert np.all(np.abs(T[inside] - I["Tt"][inside]) <= 1.0e-4 * np.abs(I["t0"][inside]))
    for kind in PROPERTIES:
        Tp = np.where(plain, T, 300.0)
        assert same_bits(literal_property(M, kind, I["p"], Tp), restate_property(M, kind, I["p"], Tp)), kind


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("model", FULL_GRID, ids=_id)
def test_boundary_restatement_and_patch_layout(pkg, model, name):
    c = _bcase(pkg, model, name)
    M, sizes, B, kinds = c["M"], c["sizes"], c["B"], c["kinds"]
    assert any(k == 1 and 2 in kinds[:i] and 2 in kinds[i + 1:] for i, k in enumerate(kinds)), "a kind-1 patch between kind-2 patches"
    assert 0 in kinds and all(s > 0 for s in sizes)
    kind = np.concatenate([np.full(s, k) for k, s in zip(kinds, sizes)])
    for into_he, R in ((False, c["R"]), (True, c["Rhe"])):
        lit = literal_boundary(M, kinds, sizes, B, 2, t_into_he=into_he)
        assert all(same_bits(lit[k], R[k]) for k in lit)
        for k in ("psi", "mu", "alpha", "rho"):
            assert np.all(np.isnan(R[k][kind == 0])) and np.all(np.isfinite(R[k][kind != 0])), k
        assert same_bits(R["he"][kind == 0], B["he"][kind == 0]) and same_bits(R["T"][kind != 2], B["T"][kind != 2])
        assert not np.any(R["he"][kind == 1] == B["he"][kind == 1])
        moved, kept = ("he", "T") if into_he else ("T", "he")
        assert not np.any(R[moved][kind == 2] == B[moved][kind == 2]) and same_bits(R[kept][kind == 2], B[kept][kind == 2])
    assert same_bits(c["R"]["T"][kind == 2], c["Rhe"]["he"][kind == 2])


def _differs(pkg, model, alt, numbers="air", rho_form=2):
    c = _case(pkg, model, numbers)
    other = restate_calculate(c["M"], c["I"]["he"], c["I"]["p"], c["I"]["t0"], rho_form, alt=(alt,))
    return not all(same_bits(other[k], c["R"][k]) for k in OUT)


def test_each_stated_rounding_changes_a_compared_bit(pkg):
    """every fma of the header comment, turned into a multiply and an add, changes a compared bit; so do (p*W)/rho against p*(W/rho), rho_form 1
    against 2, and the constants formed once on the host against their regrouping inside the expression.  The reverse case: gamma's
    cp - cpMcv is stated as NOT contracted (its product has two uses), and contracting it as Cv's changes a bit.  The other sums stated as plain
    -- Cv_ + cpMcv, 1.32 + (1.77*R)/Cv_, the Newton update -- meet no product directly.  The quotients a1/2.0 and a3/4.0 are EQUAL to a1*0.5
    and a3*0.25: halving is exact"""
    for numbers in sorted(SETS):
        for e in ("h", "e"):
            for tr in ("const", "sutherland"):
                for alt in ("ha_chain", "ha_hc"):
                    assert _differs(pkg, (e, "janaf", tr), alt, numbers), (numbers, e, tr, alt)
                # cp, and cv = fma(8314.4621, chain, -cpMcv): with the enthalpy and const transport they are at most the Newton step's divisor,
                # where one ulp moves a converged T by far less than one; they show in alpha with sutherland, in the internal energy's
                # divisor, and in the Cp / Cv / Cpv / kappa that mi_thermo_property returns from the same device functions
                c = _case(pkg, (e, "janaf", tr), numbers)
                M, p = c["M"], c["I"]["p"]
                Tf = np.where(np.isfinite(c["R"]["T"]), c["R"]["T"], 300.0)
                assert not same_bits(v_cp(M, Tf, ("cp_chain",)), v_cp(M, Tf)), (numbers, e, tr)
                assert tr == "const" or _differs(pkg, (e, "janaf", tr), "cp_chain", numbers), (numbers, e, tr)
                for kind in ("Cv", "kappa") + (("Cpv",) if e == "e" else ()):
                    if kind == "kappa" and (e, tr) == ("h", "const"):
                        continue                                   # Cpv*mu*rPr with Cpv = Cp: no cv in it
                    assert not same_bits(restate_property(M, kind, p, Tf, ("cv",)), restate_property(M, kind, p, Tf)), (numbers, e, tr, kind)
                assert (e, tr) == ("h", "const") or _differs(pkg, (e, "janaf", tr), "cv", numbers), (numbers, e, tr)
                # the reverse: gamma's product stays rounded, and the contraction of Cv would show
                assert not same_bits(restate_property(M, "gamma", p, Tf, ("gamma",)), restate_property(M, "gamma", p, Tf)), (numbers, e, tr)
                assert same_bits(restate_property(M, "Cp", p, Tf, ("cv",)), restate_property(M, "Cp", p, Tf))
                assert _differs(pkg, (e, "hConst", tr), "psi_regroup", numbers)
            for th in ("hConst", "eConst", "janaf"):
                assert _differs(pkg, ("e", th, "sutherland"), "q_regroup", numbers), (numbers, th)
            for th in ("hConst", "eConst"):
                assert _differs(pkg, ("e", th, "const"), "es", numbers), (numbers, th)
                assert not _differs(pkg, (e, th, "sutherland"), "cv", numbers)     # no product in hConst's / eConst's cv
            assert _differs(pkg, ("h", "hConst", "const"), "per_mass", numbers)
        for model in MODELS:
            c = _case(pkg, model, numbers)
            one = restate_calculate(c["M"], c["I"]["he"], c["I"]["p"], c["I"]["t0"], 1)
            assert not same_bits(one["rho"], c["R"]["rho"]) and all(same_bits(one[k], c["R"][k]) for k in OUT[:4]), model
    # the host-formed constants against their regrouping, on the compared outputs.  mu*rPr against mu/Pr is alpha itself with const transport:
    # carbon dioxide's numbers show it, air's 1.84e-05 and 0.7 happen to give the same double both ways, asserted so that a change shows
    for model in MODELS:
        if model[2] == "const":
            assert _differs(pkg, model, "rpr_regroup", "co2"), model
            assert not _differs(pkg, model, "rpr_regroup", "air"), model
    # a4/5.0 against a4*0.2 shows in T of the internal-energy janaf models with carbon dioxide's coefficients; a2/3.0 and a2*(1.0/3.0) are
    # the same double for all four a2 of the two sets (asserted: other coefficients would need the case added)
    for tr in ("const", "sutherland"):
        assert _differs(pkg, ("e", "janaf", tr), "fifth", "co2"), tr
    for S in SETS.values():
        M = host_model("h", "janaf", "const", S)
        for key in ("high", "low"):
            a, h = M[key + "CpCoeffs"], M[key + "H"]
            assert h[0] == a[1] * 0.5 and h[2] == a[3] * 0.25 and h[1] == a[2] * (1.0 / 3.0)
        assert M["CpW"] == 0.0 and M["hc"] != 0.0


def test_mirror_declares_the_class(pkg):
    """foam/miFoam: the class hePsiThermo with the reference's members is declared and in the library, and the driver is built"""
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    for word in ("class hePsiThermo", "he()", "T()", "psi()", "mu()", "alpha()", "rho()", "void correct(", "void init(", "void calculate("):
        assert word in text, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    for name in ("Foam::hePsiThermo::hePsiThermo(", "Foam::hePsiThermo::correct(", "Foam::hePsiThermo::init(", "Foam::hePsiThermo::calculate("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name
    assert os.path.exists(os.path.join(PKG, "thermoBox"))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert got.shape == want.shape and same_bits(got, want), (tag, int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))))


def _odd(dev, a):
    """the same values at an address that is 8 bytes past a 16-byte boundary: the one-by-one form of the cell pass"""
    return dev(np.concatenate([[0.0], a]))[1:]


def _addr(pkg, eng, ctx):
    case = pkg.synthetic.box_case(3, 2, 2)
    return eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)


def _run_cell(eng, A, K, c, put, out, rho_form, place, tag):
    import torch
    I = c["I"]
    n = I["he"].shape[0]
    he, p, t0 = put(I["he"]), put(I["p"]), put(I["t0"])
    t = {"separate": out(n), "t0": t0, "he": he}[place]
    psi, mu, alpha, rho = [out(n) for _ in range(4)]
    iters = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    A.thermo_calculate(K, he, p, t0, t, psi, mu, alpha, rho if rho_form else None, rho_form, iters)
    torch.cuda.synchronize()
    if ("R", rho_form) not in c:                                   # rho_form changes rho alone; restated once per case and kept
        c[("R", rho_form)] = c["R"] if rho_form == 2 else restate_calculate(c["M"], I["he"], I["p"], I["t0"], rho_form)
    want = c[("R", rho_form)]
    for name, got in zip(OUT, (t, psi, mu, alpha, rho)):
        _eq(got.cpu().numpy(), want[name] if (name != "rho" or rho_form) else np.full(n, NAN), tag + (name,))
    assert np.array_equal(iters.cpu().numpy(), want["iters"]), tag
    if place != "he":
        assert same_bits(he.cpu().numpy(), I["he"])
    assert same_bits(p.cpu().numpy(), I["p"]) and (place == "t0" or same_bits(t0.cpu().numpy(), I["t0"]))


@pytest.mark.gpu
@pytest.mark.parametrize("numbers", sorted(SETS))
@pytest.mark.parametrize("model", MODELS, ids=_id)
def test_cell_pass_base_shape(pkg, model, numbers):
    """every model and both sets of numbers at the base shape: 257 elements, 16-byte aligned, T written in place, rho = psi*p"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, model, numbers)
    _run_cell(eng, eng.Assembly(_addr(pkg, eng, ctx)), engine_model(eng, *model, SETS[numbers]), c, dev, E, 2, "t0", (model, numbers))


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("model", FULL_GRID, ids=_id)
def test_cell_pass_every_form(pkg, monkeypatch, model, blocks):
    """one hConst and one janaf model: n = 0, 1, 2, 257, 1537; MI_FACE_GRID at its default and forced to 1 and 3 workgroups; 16-byte aligned
    arrays and arrays 8 bytes off; T separate, over t0 and over he; rho_form 0, 1, 2; the evaluation counts"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    A, K = eng.Assembly(_addr(pkg, eng, ctx)), engine_model(eng, *model)
    for n in N_ALL:
        c = _case(pkg, model, "air", n)
        for put, out, how in ((dev, E, "aligned"), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:], "odd")):
            for place in ("separate", "t0", "he"):
                for rho_form in (0, 1, 2):
                    _run_cell(eng, A, K, c, put, out, rho_form, place, (model, n, blocks, how, place, rho_form))


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_boundary_pass(pkg, monkeypatch, name, blocks):
    """every patch in one launch on the four meshes: the new temperature of a kind-2 patch into b_T (OpenFOAM's meaning) and into b_he (the
    reference's transform); the faces of kind-0 patches and every array's untouched faces bit for bit as they were"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    for model in FULL_GRID:
        c = _bcase(pkg, model, name)
        L, B = c["L"], c["B"]
        addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
        bnd = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(L["patches"]))
        A, K = eng.Assembly(addr), engine_model(eng, *model)
        for into_he, want in ((False, c["R"]), (True, c["Rhe"])):
            D = {k: dev(v) for k, v in B.items()}
            A.thermo_calculate_boundary(bnd, K, c["kinds"], D["he"], D["p"], D["T"], D["psi"], D["mu"], D["alpha"], D["rho"], 2,
                                        b_t_out=D["he"] if into_he else None)
            for k in want:
                _eq(host(D[k]), want[k], (model, name, blocks, into_he, k))
        bnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", THREE, ids=_id)
def test_he_and_every_property(pkg, model):
    """mi_thermo_he and every kind of mi_thermo_property on cells (aligned, 8 bytes off) and on each patch's slice of the boundary arrays"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    A, K = eng.Assembly(_addr(pkg, eng, ctx)), engine_model(eng, *model)
    c = _case(pkg, model)
    M, p = c["M"], c["I"]["p"]
    T = np.where(np.isfinite(c["R"]["T"]), c["R"]["T"], 300.0)
    for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
        he = out(p.shape[0])
        A.thermo_he(K, put(p), put(T), he)
        _eq(host(he), v_he(M, p, T), (model, "he"))
        for kind in PROPERTIES:
            x = out(p.shape[0])
            A.thermo_property(K, kind, put(p), put(T), x)
            _eq(host(x), restate_property(M, kind, p, T), (model, kind))
    L = mesh(pkg, "box")
    sizes, B = boundary_inputs(pkg.synthetic, M, L, BSEED["box"])
    bp, bT, off = dev(B["p"]), dev(B["T"]), 0
    for size in sizes:                                             # a patch is a slice of the patch-ordered arrays
        s = slice(off, off + size)
        he = E(size)
        A.thermo_he(K, bp[s], bT[s], he)
        _eq(host(he), v_he(M, B["p"][s], B["T"][s]), (model, "patch he", off))
        for kind in PROPERTIES:
            x = E(size)
            A.thermo_property(K, kind, bp[s], bT[s], x)
            _eq(host(x), restate_property(M, kind, B["p"][s], B["T"][s]), (model, "patch", kind, off))
        off += size


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS, ids=_id)
def test_calculate_inverts_he(pkg, model):
    """mi_thermo_calculate applied to he = mi_thermo_he(p, T) returns a temperature within the algorithm's own tolerance 1e-4*T0 of T"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    A, K = eng.Assembly(_addr(pkg, eng, ctx)), engine_model(eng, *model)
    syn, n = pkg.synthetic, 1537
    T = 300.0 + syn.splitmix_uniform(SEED + 50, n) * 2200.0
    p = 5.0e4 + syn.splitmix_uniform(SEED + 51, n) * 1.5e5
    t0 = T * (0.7 + 0.6 * syn.splitmix_uniform(SEED + 52, n))
    he, out = E(n), [E(n) for _ in range(4)]
    A.thermo_he(K, dev(p), dev(T), he)
    A.thermo_calculate(K, he, dev(p), dev(t0), *out)
    got = host(out[0])
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - T) <= 1.0e-4 * t0), float(np.max(np.abs(got - T) / t0))


def _walk_inputs(pkg, M):
    L = mesh(pkg, "box")
    syn, n = pkg.synthetic, L["n"]
    sizes = [fc.shape[0] for fc, _ in L["patches"]]
    nb = sum(sizes)
    T = 300.0 + 600.0 * syn.splitmix_uniform(SEED + 60, n)
    p = 9.0e4 + 2.0e4 * syn.splitmix_uniform(SEED + 61, n)
    bT = 300.0 + 600.0 * syn.splitmix_uniform(SEED + 62, nb)
    bp = 9.0e4 + 2.0e4 * syn.splitmix_uniform(SEED + 63, nb)
    return L, sizes, T, p, bT, bp


@pytest.mark.gpu
@pytest.mark.parametrize("model", FULL_GRID, ids=_id)
def test_walk_through_the_c_abi(pkg, model):
    """the constructor (init + calculate) and three correct() on the box, he and p changed between them by the driver's rule"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    M, K = host_model(*model), engine_model(eng, *model)
    L, sizes, T0, p0, bT0, bp0 = _walk_inputs(pkg, M)
    kinds = patch_kinds(L)
    want = restate_walk(M, kinds, sizes, T0, p0, bT0, bp0)
    addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    bnd = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(sizes))
    A = eng.Assembly(addr)
    n, nb = L["n"], sum(sizes)
    T, p, bT, bp = dev(T0), dev(p0), dev(bT0), dev(bp0)
    he, psi, mu, alpha, rho = [E(n) for _ in range(5)]
    bhe, bpsi, bmu, balpha, brho = [E(nb) for _ in range(5)]
    A.thermo_he(K, p, T, he)
    off = 0
    for kind, size in zip(kinds, sizes):
        if kind:
            A.thermo_he(K, bp[off:off + size], bT[off:off + size], bhe[off:off + size])
        off += size
    for step, W in enumerate(want):
        if step:
            f, g = 1.0 + 0.03125 * step, 1.0 - 0.015625 * step
            he.mul_(f); bhe.mul_(f); p.mul_(g); bp.mul_(g)
            assert same_bits(host(he), walk_rule(step, want[step - 1]["he"], want[step - 1]["p"])[0])
        A.thermo_calculate(K, he, p, T, T, psi, mu, alpha, rho, 2)
        A.thermo_calculate_boundary(bnd, K, kinds, bhe, bp, bT, bpsi, bmu, balpha, brho, 2)
        for name, got in (("T", T), ("psi", psi), ("mu", mu), ("alpha", alpha), ("rho", rho), ("bhe", bhe), ("bT", bT), ("bpsi", bpsi),
                          ("bmu", bmu), ("balpha", balpha), ("brho", brho)):
            _eq(host(got), W[name], (model, step, name))
    bnd.close()


@pytest.mark.gpu
def test_mirror_driver_reproduces_the_walk(pkg, tmp_path):
    """foam/thermoBox.C in a process of its own: the mirror's hePsiThermo on the same box, bit for bit the restated walk"""
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    for mi, model in enumerate(FULL_GRID):
        M = host_model(*model)
        L, sizes, T0, p0, bT0, bp0 = _walk_inputs(pkg, M)
        kinds = patch_kinds(L)
        want = restate_walk(M, kinds, sizes, T0, p0, bT0, bp0)
        src, dst = tmp_path / f"in{mi}.bin", tmp_path / f"out{mi}.bin"
        with open(src, "wb") as f:
            np.array([L["n"], L["lo"].shape[0], len(sizes), M["energy"], M["thermo"], M["transport"]], dtype=np.int32).tofile(f)
            L["lo"].tofile(f); L["up"].tofile(f)
            np.array(sizes, dtype=np.int32).tofile(f); np.array(kinds, dtype=np.int32).tofile(f)
            for fc, _ in L["patches"]:
                fc.tofile(f)
            for a in (T0, p0, bT0, bp0):
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        r = subprocess.run([os.path.join(PKG, "thermoBox"), str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(dst, dtype=np.float64)
        n, nb = L["n"], sum(sizes)
        at = 0
        for step, W in enumerate(want):
            for name, m in (("T", n), ("psi", n), ("mu", n), ("alpha", n), ("rho", n), ("bT", nb), ("bpsi", nb), ("bmu", nb), ("balpha", nb), ("bhe", nb)):
                _eq(got[at:at + m], W[name], (model, step, name))
                at += m
        assert at == got.shape[0]


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    model = FULL_GRID[1]
    c = _case(pkg, model)
    I, n = c["I"], N_BASE
    L = mesh(pkg, "box")
    addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    A, K = eng.Assembly(addr), engine_model(eng, *model)
    he, p, t0 = dev(I["he"]), dev(I["p"]), dev(I["t0"])
    big = E(6 * n + 8)
    o = [big[k * n:(k + 1) * n] for k in range(5)]                # offsets k*257*8 bytes: aligned for a double
    iters = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")

    def refused(match, *args, **kw):
        with pytest.raises(eng.MiError, match=match):
            A.thermo_calculate(*args, **kw)
        assert np.all(np.isnan(host(big))) and np.all(iters.cpu().numpy() == -7), match
        assert same_bits(host(he), I["he"]) and same_bits(host(t0), I["t0"]) and same_bits(host(p), I["p"])

    refused("missing", K, None, p, t0, *o[:4])
    refused("missing", K, he, p, t0, o[0], None, o[2], o[3])
    refused("model is missing", None, he, p, t0, *o[:4])
    refused("rho array is missing", K, he, p, t0, *o[:4], None, 2)
    refused("unknown rho_form", K, he, p, t0, *o[:5], 3)
    refused("unknown rho_form", K, he, p, t0, *o[:5], -1)
    refused("overlap", K, he, p, t0, p, *o[1:4])                   # T over p: not one of the two allowed
    refused("overlap", K, he, p, t0, o[0], t0, o[2], o[3])         # psi over t0
    refused("overlap", K, he, p, t0, o[0], o[0], o[2], o[3])       # two outputs in one array
    refused("overlap", K, he, p, t0, big[1:n + 1], o[1], o[2], o[3])          # shifted by one element into the next output
    refused("overlap", K, he, p, t0[:n - 1], t0[1:], *o[1:4])      # over t0, but shifted: elements would be written before they are read
    for field, value, what in (("energy", 2, "energy form"), ("thermo", 3, "thermodynamics"), ("transport", 2, "transport"), ("W", 0.0, "finite"),
                               ("R", NAN, "finite"), ("Tcommon", 100.0, "Tcommon <= Tlow"), ("hc", float("inf"), "finite")):
        bad = engine_model(eng, *model)
        setattr(bad, field, value)
        refused(what, bad, he, p, t0, *o[:4])
        with pytest.raises(eng.MiError, match=what):
            A.thermo_he(bad, p, t0, o[0])
        with pytest.raises(eng.MiError, match=what):
            A.thermo_property(bad, "Cp", p, t0, o[0])
    # an array 4 bytes off is not aligned for a double; the iteration counts 2 bytes off not for an int32 (torch makes no such view: raw pointers)
    import ctypes as C
    lib, P = eng.lib(), lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def raw_call(*ptrs):
        eng._chk(lib.mi_thermo_calculate(ctx.h, C.byref(K), 0, C.c_int64(n - 1), *ptrs))

    for ptrs, what in (((P(he, 4), P(p), P(t0), P(o[0]), P(o[1]), P(o[2]), P(o[3]), None, None), "8 bytes"),
                       ((P(he), P(p), P(t0), P(o[0]), P(o[1], 4), P(o[2]), P(o[3]), None, None), "8 bytes"),
                       ((P(he), P(p), P(t0), P(o[0]), P(o[1]), P(o[2]), P(o[3]), None, P(iters, 2)), "4 bytes")):
        with pytest.raises(eng.MiError, match=what):
            raw_call(*ptrs)
    for entry, kind_arg in ((lib.mi_thermo_he, ()), (lib.mi_thermo_property, (C.c_int(0),))):
        head = (ctx.h, C.byref(K)) + kind_arg + (C.c_int64(n - 1),)
        for ptrs in ((P(p, 4), P(t0), P(o[0])), (P(p), P(t0, 4), P(o[0])), (P(p), P(t0), P(o[0], 4))):
            with pytest.raises(eng.MiError, match="8 bytes"):
                eng._chk(entry(*head, *ptrs))
    assert np.all(np.isnan(host(big)))
    for kind in (-1, 6):
        with pytest.raises(eng.MiError, match="property kind"):
            A.thermo_property(K, kind, p, t0, o[0])
    with pytest.raises(eng.MiError, match="overlap"):
        A.thermo_he(K, p, t0, t0)
    with pytest.raises(eng.MiError, match="missing"):
        A.thermo_property(K, "Cp", p, None, o[0])
    assert np.all(np.isnan(host(big)))
    # zero elements: MI_OK without a launch, whatever the arrays
    A.thermo_calculate(K, he[:0], None, None, None, None, None, None)
    A.thermo_he(K, p[:0], None, None)
    A.thermo_property(K, "kappa", p[:0], None, None)

    # the boundary
    cb = _bcase(pkg, model, "box")
    kinds, sizes, B = cb["kinds"], cb["sizes"], cb["B"]
    bnd = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(sizes))
    D = {k: dev(v) for k, v in B.items()}

    def b_refused(match, boundary, model_, kinds_, *args, **kw):
        with pytest.raises(eng.MiError, match=match):
            A.thermo_calculate_boundary(boundary, model_, kinds_, *args, **kw)
        for k in D:
            assert same_bits(host(D[k]), B[k]), (match, k)

    full = (D["he"], D["p"], D["T"], D["psi"], D["mu"], D["alpha"])
    b_refused("patch kind", bnd, K, [2, 1, 3, 0, 2, 1], *full)
    b_refused("patch kind", bnd, K, [2, 1, -1, 0, 2, 1], *full)
    b_refused("patch_kind is missing", bnd, K, None, *full)
    b_refused("boundary arrays needed", bnd, K, kinds, None, D["p"], D["T"], D["psi"], D["mu"], D["alpha"])
    b_refused("boundary arrays needed", bnd, K, kinds, D["he"], D["p"], D["T"], D["psi"], None, D["alpha"])
    b_refused("rho array is missing", bnd, K, kinds, *full, None, 1)
    b_refused("unknown rho_form", bnd, K, kinds, *full, D["rho"], 5)
    b_refused("overlap", bnd, K, kinds, *full, b_t_out=D["p"])
    b_refused("overlap", bnd, K, kinds, D["he"], D["he"], D["T"], D["psi"], D["mu"], D["alpha"])
    b_refused("overlap", bnd, K, kinds, D["he"], D["p"], D["T"], D["psi"], D["psi"], D["alpha"])
    b_refused("model is missing", bnd, None, kinds, *full)
    pk = (C.c_int32 * len(kinds))(*kinds)
    names = ("he", "p", "T", "T", "psi", "mu", "alpha")              # b_t_out = b_T
    for bad in (0, 1, 4, 6):                                       # he, p, psi, alpha 4 bytes off: not aligned for a double
        with pytest.raises(eng.MiError, match="8 bytes"):
            eng._chk(lib.mi_thermo_calculate_boundary(addr.h, bnd.h, C.byref(K), pk, 0, *[P(D[k], 4 if i == bad else 0) for i, k in enumerate(names)], None))
        for k in D:
            assert same_bits(host(D[k]), B[k]), (bad, k)
    other = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    b_refused("another addressing", eng.GradBoundary(other, [fc for fc, _ in L["patches"]], ["other"] * len(sizes)), K, kinds, *full)
    # every patch of kind 0, and no patches at all: MI_OK without a launch, NULL arrays allowed
    A.thermo_calculate_boundary(bnd, K, [0] * len(sizes), None, None, None, None, None, None)
    none = eng.GradBoundary(addr, [], [])
    A.thermo_calculate_boundary(none, K, [], None, None, None, None, None, None)
    for k in D:
        assert same_bits(host(D[k]), B[k]), k
