"""The kOmegaSST model on the device (kOmegaSST.C:47-111, :284-296, :398-468 with the omegaWallFunction, nutkWallFunction and kqRWallFunction
patches): mi_sst_production, mi_sst_wall_cells, mi_sst_blend, mi_sst_omega_sources, mi_sst_k_terms and mi_sst_nut, bit for bit against the
restatement of tests/komegasst_support.py; what follows a tanh is compared once the restatement continues from the device's F1
and F23."""
import os
import re

import numpy as np
import pytest

from assembly_support import bits, gpu_env, same, set_face_grid
from komegasst_support import (MODEL, MODEL_DEFAULTS, TANH_BOUND, WALL, WALL_DEFAULTS, blend_arms, coeffs, inputs, literal_args, literal_blend,
                               literal_k_terms, literal_nut, literal_omega_sources, literal_production, literal_wall_cells, restate_blend,
                               restate_k_terms, restate_nut, restate_omega_sources, restate_production, restate_wall_cells)
from turbulence_support import ALL_MESHES, BIG, MESHES, SMALL, boundary_cells, mesh, restate_production as ke_production, wall_mask, wall_tables

EXPORTS = ("mi_sst_coeffs_init", "mi_sst_production", "mi_sst_wall_cells", "mi_sst_blend", "mi_sst_omega_sources", "mi_sst_k_terms", "mi_sst_nut")
NAN = float("nan")
SEED = {"box": 2500, "edge_257": 2540, "isolated": 2580, BIG: 2620}
NUS = ("nu", "nu_f")                        # a number, a cell array
_CACHE = {}


def _case(pkg, name):
    """the mesh, its inputs and the restated results, computed once and left unchanged"""
    if name not in _CACHE:
        L = mesh(pkg, name)
        I = inputs(pkg.synthetic, L, SEED[name])
        S = I["S"]
        S2, G, mag = restate_production(I["nut"], I["grad"])
        blend = {(f3, nu): restate_blend(S, f3, I["gradK"], I["gradOmega"], I["k"], I["omega"], I["y"], I["nut"], S2, I[nu]) for f3 in (False, True) for nu in NUS}
        B = blend[(False, "nu")]
        R = dict(S2=S2, G=G, mag=mag, wall=restate_wall_cells(L, I, I["G0"], I["omega0"]), blend=blend,
                 sources=restate_omega_sources(I["V"], B["su"], B["sp"], B["susp"], I["omega"], I["diagL"], I["sourceL"]),
                 k_terms=restate_k_terms(S, G, I["k"], I["omega"]))
        _CACHE[name] = dict(L=L, I=I, R=R)
    return _CACHE[name]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    for word in ("kOmegaSST", "omegaWallFunction", "mi_sst_coeffs", "mi_sst_wall", "mi_sst_blend_arrays", "wallDist"):
        assert word in header, word


def test_coefficients_against_the_host_formulas(pkg):
    eng = pkg.engine
    K, want = eng.sst_coeffs(), coeffs()
    assert len(want) == len(K._fields_)
    for name, value in want.items():
        assert same(np.array([getattr(K, name)]), np.array([value])), name
    assert tuple(getattr(K, n) for n in MODEL) == MODEL_DEFAULTS and tuple(getattr(K, n) for n in WALL) == WALL_DEFAULTS
    assert K.twoAlphaOmega2 == 1.712 and K.c1BetaStar == 10.0 * 0.09 and K.c1a1BetaStar == (10.0 / 0.31) * 0.09 and K.dGamma == 5.0 / 9.0 - 0.44
    assert K.yPlusLam == eng.ke_coeffs().yPlusLam and K.Cmu25 == eng.ke_coeffs().Cmu25
    other = dict(alphaK1=0.85034, alphaOmega2=0.85616, gamma1=0.5532, gamma2=0.4403, betaStar=0.085, a1=0.3, b1=1.5, c1=9.0, kappa=0.4187, E=9.0, wallBeta1=0.08)
    K2, w2 = eng.sst_coeffs(**other), coeffs(**other)
    assert all(same(np.array([getattr(K2, n)]), np.array([v])) for n, v in w2.items())
    for bad in (dict(alphaK1=0.0), dict(betaStar=-0.09), dict(a1=NAN), dict(c1=float("inf")), dict(kappa=0.0), dict(wallBeta1=-1.0), dict(Cmu=NAN)):
        with pytest.raises(eng.MiError, match="above zero"):
            eng.sst_coeffs(**bad)
    with pytest.raises(TypeError):
        eng.sst_coeffs(sigmaEps=1.3)


@pytest.mark.parametrize("name", ALL_MESHES)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg, name):
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    S = I["S"]
    assert all(same(a, b) for a, b in zip(literal_production(I["nut"], I["grad"]), (R["S2"], R["G"], R["mag"])))
    assert all(same(a, b) for a, b in zip(literal_wall_cells(L, I, I["G0"], I["omega0"]), R["wall"]))
    # the wall layout: the conditions of the kEpsilon tests
    W, wall = wall_tables(L), wall_mask(L)
    faces_per_cell = np.array([len(f) for f in W["faces"]])
    assert {1, 2, 3} <= set(faces_per_cell.tolist())
    flags = [w for _, w in L["patches"]]
    assert any(not w and any(flags[:i]) and any(flags[i + 1:]) for i, w in enumerate(flags)), "a non-wall patch between wall patches"
    G, om, bom = R["wall"]
    off_wall = np.setdiff1d(np.arange(L["n"]), W["cells"])
    assert off_wall.size and same(G[off_wall], I["G0"][off_wall]) and same(om[off_wall], I["omega0"][off_wall])
    assert np.all(np.isnan(bom[~wall])) and np.all(bom[wall] > 0) and np.all(G[W["cells"]] >= 0)
    # the blending pass: the arguments of every tanh from literal loops; what follows from the same F1 / F23
    least = 0.05 * L["n"] if name == BIG else 1
    seen = {}
    for (f3, nu), B in R["blend"].items():
        lit = literal_args(S, I["gradK"], I["gradOmega"], I["k"], I["omega"], I["y"], I[nu])
        assert all(same(a, B[key]) for a, key in zip(lit, ("CD", "arg1", "arg2", "arg3"))), (f3, nu)
        rest = literal_blend(S, B["F1"], B["F23"], B["CD"], I["omega"], I["nut"], R["S2"], I[nu])
        assert all(same(a, B[key]) for a, key in zip(rest, ("su", "sp", "susp", "domega", "dk"))), (f3, nu)
        assert np.all(np.isfinite(B["su"])) and np.all(B["F1"] >= 0) and np.all(B["F1"] <= 1) and np.all(B["F23"] >= 0) and np.all(B["F23"] <= 1)
        for arm, mask in blend_arms(S, B, I["omega"], R["S2"]).items():
            assert mask.sum() >= least, (name, f3, nu, arm, int(mask.sum()))
            seen[arm] = seen.get(arm, 0) + int(mask.sum())
        assert np.any((B["CD"] > 0) & ~(B["CD"] > 1.0e-10)), "a positive CDkOmega below 1e-10"
        if f3:
            assert np.any(B["t3"] > 0) and np.any(B["F23"] < R["blend"][(False, nu)]["F23"])
    assert len(seen) == 18
    B = R["blend"][(False, "nu")]
    assert all(same(a, b) for a, b in zip(literal_omega_sources(I["V"], B["su"], B["sp"], B["susp"], I["omega"], I["diagL"], I["sourceL"]), R["sources"]))
    assert all(same(a, b) for a, b in zip(literal_k_terms(S, R["G"], I["k"], I["omega"]), R["k_terms"]))
    g_arm = R["G"] < (S["c1BetaStar"] * I["k"]) * I["omega"]
    assert g_arm.sum() >= least and (~g_arm).sum() >= least
    for f3 in (False, True):
        for ctor, s in ((False, R["S2"]), (True, R["mag"])):
            nut, F23, _, _ = restate_nut(S, f3, I["k"], I["omega"], I["y"], s, I["nu"], ctor)
            assert same(literal_nut(S, F23, I["k"], I["omega"], s, ctor), nut) and np.all(nut > 0) and np.all(np.isfinite(nut))
            assert same(F23, R["blend"][(f3, "nu")]["F23"])


@pytest.mark.parametrize("name", MESHES)
def test_each_stated_rounding_changes_a_compared_bit(pkg, name):
    """the fma of CDkOmega's dot product, the contraction in the omega functor, the grouping of the omega equation's right-hand side against
    fvm::Sp followed by fvm::SuSp, the order of the wall sum across patches and the host-formed constants against their regrouping inside the
    expression each change a compared bit when altered.  2*(alphaOmega2*x) and (2*alphaOmega2)*x are EQUAL: doubling is exact"""
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    S, B = I["S"], R["blend"][(False, "nu")]
    args = (S, False, I["gradK"], I["gradOmega"], I["k"], I["omega"], I["y"], I["nut"], R["S2"], I["nu"])
    plain = restate_blend(*args, plain_dot=True)
    assert not same(plain["CD"], B["CD"]) and not same(plain["susp"], B["susp"])
    assert not same(restate_wall_cells(L, I, I["G0"], I["omega0"], contracted=False)[1], R["wall"][1])
    rev = restate_wall_cells(L, I, I["G0"], I["omega0"], reverse_patches=True)
    assert not same(rev[0], R["wall"][0]) and not same(rev[1], R["wall"][1]) and not same(rev[2], R["wall"][2])
    seq = restate_omega_sources(I["V"], B["su"], B["sp"], B["susp"], I["omega"], I["diagL"], I["sourceL"], sequential=True)
    assert not same(seq[0], R["sources"][0]) and not same(seq[1], R["sources"][1])
    assert np.allclose(seq[0], R["sources"][0], rtol=1e-12, atol=0) and np.allclose(seq[1], R["sources"][1], rtol=1e-9, atol=1e-9)   # the same sum, grouped otherwise
    re_ = restate_blend(*args, cont=dict(F1=B["F1"], F23=B["F23"]), regroup=True)
    for key in ("arg1", "su", "sp", "domega", "dk"):
        assert not same(re_[key], B[key]), key
    assert not same(restate_k_terms(S, R["G"], I["k"], I["omega"], regroup=True)[0], R["k_terms"][0])
    dot = B["CD"] * I["omega"]
    with np.errstate(all="ignore"):
        assert same(2 * (S["alphaOmega2"] * dot), S["twoAlphaOmega2"] * dot) and same(4 * (S["alphaOmega2"] * I["k"]), S["fourAlphaOmega2"] * I["k"])


@pytest.mark.parametrize("name", MESHES)
def test_the_stated_equalities_hold(pkg, name):
    """mi_sst_production's G = nut*(2*magSqr) has the bits of mi_ke_production's (nut*2)*magSqr; the k equation's su - fvm::Sp(sp) formed as a
    matrix and subtracted (the operator sequence of mi_sst_omega_sources with susp = 0 taken out) equals what mi_fvm_assemble does with su
    and sp: diag + V*sp, source + V*su"""
    c = _case(pkg, name)
    I, R = c["I"], c["R"]
    assert same(R["G"], ke_production(I["nut"], I["grad"]))
    su, sp = R["k_terms"]
    V, diag, source = I["V"], I["diagL"], I["sourceL"]
    assert same(diag - (-(V * sp)), diag + V * sp) and same(source - ((-0.0) - V * su), source + V * su)


def test_mirror_declares_the_model(pkg):
    """foam/miFoam: the class incompressible::RASModels::kOmegaSST with the reference's members is declared and in the library"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    body = text[text.index("class kOmegaSST"):]
    for word in ("F1(", "F2(", "F3(", "F23(", "blend(", "alphaK(", "alphaOmega(", "beta(", "gamma(", "DkEff(", "DomegaEff(", "k()", "omega()", "nut()",
                 "void correct("):
        assert word in body, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    model = "Foam::incompressible::RASModels::kOmegaSST::"
    for name in ("kOmegaSST(", "correct(", "F2(", "F3(", "F23(", "blend(", "DkEff(", "DomegaEff("):      # F1() is the inline accessor of the last correct()'s field
        assert len(re.findall(r" T " + re.escape(model + name), syms)) >= 1, name


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _boundary(eng, addr, L):
    return eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other" if w else "fixesValue" for _, w in L["patches"]])


def _odd(dev, a):
    """the same values at an address that is 8 bytes past a 16-byte boundary: the one-cell-at-a-time form of the cell passes"""
    return dev(np.concatenate([[0.0], a]))[1:]


def _tanh_deviation(got, arg):
    """the largest relative deviation of the device's tanh from numpy's, in units of 2^-52"""
    want = np.tanh(arg)
    return float(np.max(np.abs(got / want - 1.0))) * 2.0 ** 52


def _blend(A, K, f3, put, out, I, S2, nu, n):
    o = {key: out(n) for key in ("F1", "su", "sp", "susp", "domega", "dk", "CD", "arg1", "F23", "t3")}
    A.sst_blend(K, f3, [put(g) for g in I["gradK"]], [put(g) for g in I["gradOmega"]], put(I["k"]), put(I["omega"]), put(I["y"]), put(I["nut"]), put(S2),
                nu, o["F1"], o["su"], o["sp"], o["susp"], o["domega"], o["dk"], o["CD"], o["arg1"], o["F23"], o["t3"])
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_cell_passes(pkg, monkeypatch, name, blocks):
    """production, blending (F3 off and on, nu a number and an array), the omega equation's right-hand side, the k terms and nut in both
    forms; 16-byte aligned arrays (two cells per thread) and arrays 8 bytes off (one by one); MI_FACE_GRID at its default and forced to 1 and
    3 workgroups.  S2, G, mag, CDkOmega, arg1, the right-hand side and the k terms bit for bit; what follows a tanh bit for bit from the
    device's F1 / F23; the device's tanh within TANH_BOUND of numpy's"""
    import torch
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, K, S = L["n"], eng.sst_coeffs(), I["S"]
    worst = 0.0
    for tag, addr in _addressings(eng, ctx, L):
        A = eng.Assembly(addr)
        for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
            S2, G, mag = out(n), out(n), out(n)
            A.sst_production(put(I["nut"]), [put(g) for g in I["grad"]], S2, G, mag)
            _eq(host(S2), R["S2"], (name, tag, blocks, "S2")); _eq(host(G), R["G"], (name, tag, blocks, "G")); _eq(host(mag), R["mag"], (name, tag, blocks, "mag"))
            S2b, Gb = out(n), out(n)
            A.sst_production(put(I["nut"]), [put(g) for g in I["grad"]], S2b, Gb)          # without the optional output: the same
            _eq(host(S2b), R["S2"], "S2 alone"); _eq(host(Gb), R["G"], "G alone")
            f2 = {}
            for f3 in (False, True):
                for key in NUS:
                    B = R["blend"][(f3, key)]
                    o = {k_: host(v) for k_, v in _blend(A, K, f3, put, out, I, R["S2"], I[key] if key == "nu" else put(I[key]), n).items()}
                    _eq(o["CD"], B["CD"], (name, tag, blocks, f3, key, "CDkOmega")); _eq(o["arg1"], B["arg1"], (name, tag, blocks, f3, key, "arg1"))
                    worst = max(worst, _tanh_deviation(o["F1"], B["p1"]))
                    if f3:
                        worst = max(worst, _tanh_deviation(o["t3"], B["p3"]))
                        with np.errstate(all="ignore"):
                            _eq(o["F23"], f2[key] * (1.0 - o["t3"]), (name, tag, blocks, key, "F23 = F2*F3"))
                    else:
                        f2[key] = o["F23"]
                        worst = max(worst, _tanh_deviation(o["F23"], B["p2"]))
                        assert np.all(o["t3"] == 0.0)
                    want = restate_blend(S, f3, I["gradK"], I["gradOmega"], I["k"], I["omega"], I["y"], I["nut"], R["S2"], I[key], cont=dict(F1=o["F1"], F23=o["F23"]))
                    for what in ("su", "sp", "susp", "domega", "dk"):
                        _eq(o[what], want[what], (name, tag, blocks, f3, key, what))
                    nut, F23 = out(n), out(n)
                    nu = I[key] if key == "nu" else put(I[key])
                    A.sst_nut(K, f3, put(I["k"]), put(I["omega"]), put(I["y"]), put(R["S2"]), nu, nut, F23)
                    _eq(host(F23), o["F23"], (name, tag, blocks, f3, key, "F23 of nut"))
                    _eq(host(nut), restate_nut(S, f3, I["k"], I["omega"], I["y"], R["S2"], I[key], False, o["F23"])[0], (name, tag, blocks, f3, key, "nut"))
                    nut0 = out(n)
                    A.sst_nut(K, f3, put(I["k"]), put(I["omega"]), put(I["y"]), put(R["mag"]), nu, nut0, constructor_form=True)
                    _eq(host(nut0), restate_nut(S, f3, I["k"], I["omega"], I["y"], R["mag"], I[key], True, o["F23"])[0], (name, tag, blocks, f3, key, "nut0"))
            B = R["blend"][(False, "nu")]
            diag, source = put(I["diagL"]), put(I["sourceL"])
            A.sst_omega_sources(put(I["V"]), put(B["su"]), put(B["sp"]), put(B["susp"]), put(I["omega"]), diag, source)
            _eq(host(diag), R["sources"][0], (name, tag, blocks, "diag")); _eq(host(source), R["sources"][1], (name, tag, blocks, "source"))
            su, sp = out(n), out(n)
            A.sst_k_terms(K, put(R["G"]), put(I["k"]), put(I["omega"]), su, sp)
            _eq(host(su), R["k_terms"][0], (name, tag, blocks, "su_k")); _eq(host(sp), R["k_terms"][1], (name, tag, blocks, "sp_k"))
    torch.cuda.synchronize()
    print(f"{name} {blocks}: the device's tanh deviates from numpy's by at most {worst:.2f} units of 2^-52")
    assert worst * 2.0 ** -52 <= TANH_BOUND, worst


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_wall_cells(pkg, monkeypatch, name, blocks):
    """the omega wall function on every wall patch in one launch: G, omega and the boundary values bit for bit (no transcendental), non-wall
    cells and faces untouched, under the caller's numbering and under ordered addressing"""
    set_face_grid(monkeypatch, blocks)
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    K, wall = eng.sst_coeffs(), wall_mask(L)
    nb = wall.shape[0]
    assert name != BIG or wall_tables(L)["cells"].shape[0] > 256
    for tag, addr in _addressings(eng, ctx, L):
        A, B = eng.Assembly(addr), _boundary(eng, addr, L)
        H = eng.KEpsilon(addr, B, [w for _, w in L["patches"]])
        for put in (dev, lambda a: _odd(dev, a)):
            G, om, bom = put(I["G0"]), put(I["omega0"]), E(nb)
            A.sst_wall_cells(H, K, put(I["k"]), [put(x) for x in I["U"]], [put(x) for x in I["Uw"]], put(I["bdc"]), put(I["by"]), put(I["bnuw"]),
                             put(I["bnutw"]), G, om, bom)
            _eq(host(G), R["wall"][0], (name, tag, blocks, "G")); _eq(host(om), R["wall"][1], (name, tag, blocks, "omega"))
            _eq(host(bom)[wall], R["wall"][2][wall], (name, tag, blocks, "b_omega"))
            assert np.all(host(bom)[~wall] == fill)
        H.close(); B.close()


def _channel_walk(pkg, orc, ordered):
    """The constructor's lines (kOmegaSST.C:284-296) and three correct() steps (:412-467) on the 6 x 5 x 4 channel of turbulence_support with a
    fixed-value inlet, a zero-gradient outlet and four walls, driven through the Python binding: gradK / gradOmega from mi_gauss_grad each
    step, their boundary values, the blending pass on the cells and on the boundary faces, both equations up to the arrays handed to the
    solver equal to the restatement bit for bit; each solve is the engine's PBiCG and the restatement continues from its solution and from
    the device's F1 / F23 / log values; k, omega and nut stay finite and positive -> the engine's fields after the constructor's lines and
    after every step"""
    import torch
    from komegasst_support import channel, restate_correct, restate_nut_update
    from turbulence_support import patch_coeffs
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    M, St = channel(pkg)
    L, n, nf, nb, f3 = M["L"], M["n"], M["nf"], M["nb"], M["f3"]
    K, Kw, wall = eng.sst_coeffs(), eng.ke_coeffs(), wall_mask(L)
    nu, rdt = M["nu"], 1.0 / M["dt"]
    fcs = [fc for fc, _ in L["patches"]]
    addr = eng.Addressing(ctx, n, M["lo"], M["up"], ordered=ordered)
    A = eng.Assembly(addr)
    Bd = eng.GradBoundary(addr, fcs, ["fixesValue" if kd == "inlet" else "other" for kd in M["kinds"]])
    H = eng.KEpsilon(addr, Bd, [kd == "wall" for kd in M["kinds"]])
    patches = [eng.Patch(ctx, n, fc) for fc in fcs]
    cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
    g = {key: dev(M[key]) for key in ("V", "magSf", "dc", "lam", "bms", "bdc", "by", "phi", "bnuw", "y")}
    Sf, bSf = [dev(x) for x in M["Sf"]], [dev(x) for x in M["bSf"]]
    AV = eng.Average(addr, Bd, g["magSf"], g["bms"])
    U, Uw, grad, bgrad = [dev(x) for x in M["U"]], [dev(x) for x in M["Uw"]], [dev(x) for x in M["grad"]], [dev(x) for x in M["bgrad"]]
    inlet = torch.from_numpy(M["kind_of"] == "inlet").to("cuda:0")
    bcells = torch.from_numpy(boundary_cells(L).astype(np.int64)).to("cuda:0")
    mat = eng.Matrix(addr)

    def boundary_of(cell, inlet_value):
        out = E(nb)
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            p.internal_field(cell, out[a:b])
        out[inlet] = inlet_value
        return out

    def bound(v, bv, lb):
        lo = min(A.min_max(v)[0], A.min_max(bv)[0])
        if not lo < lb:
            return False
        A.vec_max_value(bv, lb, bv)
        A.bound(AV, lb, g["lam"], g["magSf"], v, g["bms"], bv)
        return True

    def full_grad(vf, bvf):
        """fvc::grad(vf) with `Gauss linear` and its boundary values (gaussGrad::correctBoundaryConditions)"""
        ssf, gr, bg = E(nf), [E(n) for _ in range(3)], [E(nb) for _ in range(3)]
        A.face_interpolate(g["lam"], vf, ssf)
        A.gauss_grad(Sf, ssf, None, gr)
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            for d in range(3):
                p.add_product(bSf[d][a:b], bvf[a:b], gr[d], 0)
        gr = [x / g["V"] for x in gr]
        sn = g["bdc"] * (bvf - vf[bcells])
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            p.gauss_grad_correct([x[a:b] for x in bSf], g["bms"][a:b], [sn[a:b]], gr, [x[a:b] for x in bg])
        return gr, bg

    def nut_update(k, om, bk, bom, s, bs, ctor):
        nut, bnut, blog, F23, bF23 = E(n), E(nb), E(nb), E(n), E(nb)
        A.sst_nut(K, f3, k, om, g["y"], s, nu, nut, F23, constructor_form=ctor)
        A.sst_nut(K, f3, bk, bom, g["by"], bs, nu, bnut, bF23, constructor_form=ctor)
        A.ke_nut_wall(H, Kw, k, g["by"], g["bnuw"], bnut, blog)
        return nut, bnut, blog, F23, bF23

    def equation(psi_old, psi, gamma, bgamma_h, inlet_value, alpha, sp_su=None, rhs=None, labels=None):
        gam = E(nf)
        A.face_interpolate(g["lam"], gamma, gam)
        gam = gam * g["magSf"]
        upper, lower, diag, source = E(nf), E(nf), E(n), E(n)
        extra = {} if sp_su is None else dict(sp=(sp_su[0], 1.0), su=[(-1.0, [sp_su[1]])])
        A.assemble(upper, diag, lower, [source], ddt=dict(r_delta_t=rdt, vol=g["V"], psi_old=[psi_old]), div=dict(flux=g["phi"], weights=g["lam"]),
                   laplacian=dict(delta_coeffs=g["dc"], gamma_magsf=gam), **extra)
        out = dict(gam=host(gam), upper0=host(upper), lower0=host(lower), diagL=host(diag), sourceL=host(source))
        if rhs is not None:
            A.sst_omega_sources(g["V"], rhs["su"], rhs["sp"], rhs["susp"], psi, diag, source)
        out.update(diag0=host(diag), source0=host(source))
        ich, bch = patch_coeffs(M, bgamma_h, inlet_value)
        ic, bc = [dev(x) for x in ich], [dev(x) for x in bch]
        A.relax(alpha, diag, lower, upper, source, psi, patches, ic, bc, [0] * len(patches))
        out.update(diag1=host(diag), source1=host(source))
        if labels is not None:
            values, u2, l2 = E(labels.numel()), E(nf), E(nf)
            H.wall_values(psi, values)
            A.set_values(labels, values, psi, diag, source, upper, lower, u2, l2, patches, ic, bc)
            upper, lower = u2, l2
        ds, ss = diag.clone(), source.clone()
        for p, i, b in zip(patches, ic, bc):
            p.add(i, ds, 0); p.add(b, ss, 0)
        out.update(psi=host(psi), upper=host(upper), lower=host(lower), source=host(source), ic=np.concatenate([host(x) for x in ic]),
                   bc=np.concatenate([host(x) for x in bc]), diag_solve=host(ds), source_solve=host(ss))
        mat.set_coeffs(ds, upper, lower)
        perf = mat.pbicg(psi, ss, "diagonal", tolerance=1e-10, relTol=0.0, maxIter=300)
        assert 0 < perf["nIterations"] < 300
        return out

    # the constructor: bound(k), bound(omega) (nothing to do on positive fields), nut from mag(symm(gradU)) and its boundary conditions
    k, om, bk, bom = dev(St["k"]), dev(St["omega"]), dev(St["bk"]), dev(St["bomega"])
    assert not bound(k, bk, SMALL) and not bound(om, bom, SMALL)
    S2, G0, mag, bS2, bG0, bmag = E(n), E(n), E(n), E(nb), E(nb), E(nb)
    A.sst_production(dev(np.ones(n)), grad, S2, G0, mag)
    A.sst_production(dev(np.ones(nb)), bgrad, bS2, bG0, bmag)
    _eq(host(mag), restate_production(np.ones(n), M["grad"])[2], "mag"); _eq(host(bmag), restate_production(np.ones(nb), M["bgrad"])[2], "bmag")
    nut, bnut, blog, F23, bF23 = nut_update(k, om, bk, bom, mag, bmag, True)
    St["nut"], St["bnut"], taken = restate_nut_update(M, St["k"], St["omega"], St["bk"], St["bomega"], host(mag), host(bmag), host(blog), host(F23), host(bF23),
                                                      ctor=True)
    _eq(host(nut), St["nut"], "nut0"); _eq(host(bnut), St["bnut"], "bnut0")
    assert 0.2 <= taken[wall].mean() <= 0.8
    labels = H.wall_cell_labels()
    keys = ("k", "omega", "nut", "bk", "bomega", "bnut")
    states = [{key: np.array(St[key]) for key in keys}]
    for step in range(M["steps"]):
        D = {}
        S2, G, bG = E(n), E(n), E(nb)
        A.sst_production(nut, grad, S2, G)
        A.sst_production(bnut, bgrad, bS2, bG)
        om_old, k_old = om.clone(), k.clone()
        A.sst_wall_cells(H, K, k, U, Uw, g["bdc"], g["by"], g["bnuw"], bnut, G, om, bom)
        D.update(S2=host(S2), bS2=host(bS2), G=host(G), omega_wall=host(om), bomega_wall=host(bom))
        gk, bgk = full_grad(k, bk)
        go, bgo = full_grad(om, bom)
        for d in range(3):
            D.update({"gradK%d" % d: host(gk[d]), "gradOmega%d" % d: host(go[d]), "bgradK%d" % d: host(bgk[d]), "bgradOmega%d" % d: host(bgo[d])})
        o = {key: E(n) for key in ("F1", "su", "sp", "susp", "domega", "dk", "CD", "arg1", "F23")}
        A.sst_blend(K, f3, gk, go, k, om, g["y"], nut, S2, nu, o["F1"], o["su"], o["sp"], o["susp"], o["domega"], o["dk"], o["CD"], o["arg1"], o["F23"])
        b = {key: E(nb) for key in ("F1", "su", "sp", "susp", "domega", "dk", "CD", "arg1", "F23")}
        A.sst_blend(K, f3, bgk, bgo, bk, bom, g["by"], bnut, bS2, nu, b["F1"], b["su"], b["sp"], b["susp"], b["domega"], b["dk"], b["CD"], b["arg1"], b["F23"])
        D.update({key: host(o[key]) for key in ("su", "sp", "susp", "domega", "dk", "CD", "arg1")})
        D.update(bCD=host(b["CD"]), barg1=host(b["arg1"]), bdomega=host(b["domega"]), bdk=host(b["dk"]))
        X = dict(F1=host(o["F1"]), F23=host(o["F23"]), bF1=host(b["F1"]), bF23=host(b["F23"]))
        e = equation(om_old, om, o["domega"], D["bdomega"], M["omega_in"], M["alpha_omega"], rhs=o, labels=labels)
        D.update({"omega_" + key: v for key, v in e.items()})
        X["omega_solved"] = host(om).copy()
        bom = boundary_of(om, M["omega_in"])
        D["omega_bounded"] = bound(om, bom, SMALL)
        suk, spk = E(n), E(n)
        A.sst_k_terms(K, G, k, om, suk, spk)
        q = equation(k_old, k, o["dk"], D["bdk"], M["k_in"], M["alpha_k"], sp_su=(spk, suk))
        D.update({"k_" + key: v for key, v in q.items()})
        D.update(su_k=host(suk), sp_k=host(spk), omega_new=host(om), bomega_new=host(bom))
        X["k_solved"] = host(k).copy()
        bk = boundary_of(k, M["k_in"])
        D["k_bounded"] = bound(k, bk, SMALL)
        nut, bnut, blog, F23, bF23 = nut_update(k, om, bk, bom, S2, bS2, False)
        D.update(k_new=host(k), bk_new=host(bk), nut=host(nut), bnut=host(bnut))
        X.update(blog=host(blog), nutF23=host(F23), bnutF23=host(bF23))
        want, St, taken = restate_correct(orc, M, St, X)
        assert set(want) == set(D), set(want) ^ set(D)
        for key in sorted(want):
            if isinstance(want[key], bool):
                assert D[key] == want[key], (step, key)
            else:
                _eq(D[key], want[key], (step, key))
        for key in ("k", "omega", "nut", "bk", "bomega"):
            assert np.all(np.isfinite(St[key])) and np.all(St[key] > 0), (step, key)
        assert np.all(np.isfinite(St["bnut"])) and np.all(St["bnut"] >= 0)
        print(f"step {step}: k {St['k'].min():.3e}..{St['k'].max():.3e}  omega {St['omega'].min():.3e}..{St['omega'].max():.3e}  "
              f"nut {St['nut'].min():.3e}..{St['nut'].max():.3e}  F1 {X['F1'].min():.3f}..{X['F1'].max():.3f}  log branch on {taken[wall].mean():.2f} of the wall faces")
        states.append({key: np.array(St[key]) for key in keys})
    for h in (AV, H, Bd):
        h.close()
    return M, states


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["caller", "ordered"])
def test_channel_walk(pkg, orc, ordered):
    """_channel_walk under the caller's numbering and under ordered addressing"""
    _channel_walk(pkg, orc, ordered)


@pytest.mark.gpu
def test_mirror_komegasst_walks_the_channel(pkg, orc, tmp_path):
    """foam/miFoam's incompressible::RASModels::kOmegaSST -- its constructor and three correct() calls, through the driver
    foam/kOmegaSSTChannel.C in a process of its own, with the solver of the walk (PBiCG, diagonal, 1e-10) -- gives k, omega, nut and their
    boundary values of the Python walk bit for bit after the constructor and after every step"""
    import subprocess
    M, states = _channel_walk(pkg, orc, False)
    L = M["L"]
    types = {"inlet": 0, "outlet": 1, "wall": 2}
    d = str(tmp_path)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{M['n']} {M['nf']} {M['steps']} {repr(1.0 / M['dt'])} {repr(M['nu'])} {repr(M['alpha_omega'])} {repr(M['alpha_k'])} {len(M['kinds'])}\n")
        for (fc, _), kd in zip(L["patches"], M["kinds"]):
            f.write(f"{fc.shape[0]} {types[kd]}\n")
    put = lambda name, a, dt=np.float64: np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name + ".bin"))
    put("lower", M["lo"], np.int32); put("upper", M["up"], np.int32); put("faceCells", boundary_cells(L), np.int32)
    for name, key in (("weights", "lam"), ("deltaCoeffs", "dc"), ("magSf", "magSf"), ("V", "V"), ("bMagSf", "bms"), ("bDeltaCoeffs", "bdc"), ("y", "by"),
                      ("yCell", "y"), ("phi", "phi"), ("bPhi", "bphi")):
        put(name, M[key])
    for c in range(3):
        put(f"U{c}", M["U"][c]); put(f"bU{c}", M["Uw"][c]); put(f"Sf{c}", M["Sf"][c]); put(f"bSf{c}", M["bSf"][c])
        for k in range(3):
            put(f"gradU{c}_{k}", M["grad"][3 * c + k]); put(f"bgradU{c}_{k}", M["bgrad"][3 * c + k])
    first = states[0]
    put("k", first["k"]); put("bk", first["bk"]); put("omega", first["omega"]); put("bomega", first["bomega"])
    app = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "kOmegaSSTChannel")
    run = subprocess.run([app, d], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    for step, want in enumerate(states):
        for key in ("k", "omega", "nut", "bk", "bomega", "bnut"):
            got = np.fromfile(os.path.join(d, f"{key}_{step}.bin"), dtype=np.float64)
            _eq(got, want[key], (step, key))


class Misaligned:
    """a device address four bytes into a float64 tensor, as engine._ptr takes one: not aligned for a double"""

    def __init__(self, t):
        self.t, self.dtype = t, t.dtype

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def numel(self):
        return self.t.numel() - 1

    def data_ptr(self):
        return self.t.data_ptr() + 4


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, "box")
    L, I, R = c["L"], c["I"], c["R"]
    n, K = L["n"], eng.sst_coeffs()
    nb = I["by"].shape[0]
    addr, other = eng.Addressing(ctx, n, L["lo"], L["up"]), eng.Addressing(ctx, n, L["lo"], L["up"])
    A, Bd = eng.Assembly(addr), _boundary(eng, addr, L)
    bad = Misaligned(E(n + 1))
    broken = eng.sst_coeffs()
    broken.betaStar = NAN
    negative = eng.sst_coeffs()
    negative.a1 = -0.31
    nut, grad, k, om, y, S2, nu_f = dev(I["nut"]), [dev(g) for g in I["grad"]], dev(I["k"]), dev(I["omega"]), dev(I["y"]), dev(R["S2"]), dev(I["nu_f"])
    gk, go = [dev(g) for g in I["gradK"]], [dev(g) for g in I["gradOmega"]]
    o = [E(n) for _ in range(10)]
    for args, why in (((None, grad, o[0], o[1]), "missing"), ((nut, grad[:8] + [None], o[0], o[1]), "missing"), ((nut, grad, None, o[1]), "missing"),
                      ((nut, grad, o[0], None), "missing"), ((nut, grad, nut, o[1]), "alias"), ((nut, grad, o[0], grad[4]), "alias"), ((nut, grad, o[0], o[0]), "differ"),
                      ((nut, grad, o[0], o[1], o[1]), "differ"), ((nut, grad, o[0], o[1], nut), "alias"), ((bad, grad, o[0], o[1]), "aligned"),
                      ((nut, grad, o[0], bad), "aligned"), ((nut, grad, o[0], o[1], bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.sst_production(*args)
    good = dict(coeffs=K, f3=True, grad_k=gk, grad_omega=go, k=k, omega=om, y=y, nut=nut, s2=S2, nu=1e-4, f1_out=o[0], su_out=o[1], sp_out=o[2], susp_out=o[3],
                domega_out=o[4], dk_out=o[5], cdkomega_out=o[6], arg1_out=o[7], f23_out=o[8], tanh3_out=o[9])
    for kw, why in ((dict(k=None), "missing"), (dict(grad_k=[gk[0], None, gk[2]]), "missing"), (dict(grad_omega=None), "missing"), (dict(y=None), "missing"),
                    (dict(s2=None), "missing"), (dict(f1_out=None), "missing"), (dict(dk_out=None), "missing"), (dict(coeffs=None), "coefficients"),
                    (dict(coeffs=broken), "above zero"), (dict(coeffs=negative), "above zero"), (dict(nu=0.0), "nu"), (dict(nu=NAN), "nu"),
                    (dict(su_out=k), "alias"), (dict(nu=nu_f, dk_out=nu_f), "alias"), (dict(arg1_out=y), "alias"), (dict(sp_out=o[1]), "differ"),
                    (dict(f23_out=o[0]), "differ"), (dict(tanh3_out=o[6]), "differ"), (dict(omega=bad), "aligned"), (dict(nu=bad), "aligned"),
                    (dict(susp_out=bad), "aligned"), (dict(cdkomega_out=bad), "aligned")):
        args = dict(good)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            A.sst_blend(**args)
    V, su, sp, susp = dev(I["V"]), dev(R["blend"][(False, "nu")]["su"]), dev(R["blend"][(False, "nu")]["sp"]), dev(R["blend"][(False, "nu")]["susp"])
    for args, why in (((None, su, sp, susp, om, o[0], o[1]), "missing"), ((V, su, sp, None, om, o[0], o[1]), "missing"), ((V, su, sp, susp, om, None, o[1]), "missing"),
                      ((V, su, sp, susp, om, o[0], None), "missing"), ((V, su, sp, susp, om, om, o[1]), "alias"), ((V, su, sp, susp, om, o[0], su), "alias"),
                      ((V, su, sp, susp, om, o[0], o[0]), "differ"), ((V, su, sp, susp, bad, o[0], o[1]), "aligned"), ((V, su, sp, susp, om, o[0], bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.sst_omega_sources(*args)
    G = dev(R["G"])
    for args, why in (((K, None, k, om, o[0], o[1]), "missing"), ((K, G, k, om, o[0], None), "missing"), ((K, G, k, om, k, o[1]), "alias"),
                      ((K, G, k, om, o[0], o[0]), "differ"), ((K, G, k, bad, o[0], o[1]), "aligned"), ((None, G, k, om, o[0], o[1]), "coefficients"),
                      ((broken, G, k, om, o[0], o[1]), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            A.sst_k_terms(*args)
    for args, why in (((K, False, None, om, y, S2, 1e-4, o[0]), "missing"), ((K, False, k, om, y, None, 1e-4, o[0]), "missing"), ((K, False, k, om, y, S2, 1e-4, None), "missing"),
                      ((K, False, k, om, y, S2, 1e-4, k), "alias"), ((K, True, k, om, y, S2, nu_f, o[0], nu_f), "alias"), ((K, True, k, om, y, S2, 1e-4, o[0], o[0]), "differ"),
                      ((K, False, k, om, y, S2, -1e-4, o[0]), "nu"), ((K, False, k, om, bad, S2, 1e-4, o[0]), "aligned"), ((K, False, k, om, y, S2, 1e-4, o[0], bad), "aligned"),
                      ((None, False, k, om, y, S2, 1e-4, o[0]), "coefficients"), ((broken, False, k, om, y, S2, 1e-4, o[0]), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            A.sst_nut(*args)
    # the wall pass: a handle of another addressing cannot be made; the arrays
    flags = [w for _, w in L["patches"]]
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.KEpsilon(other, Bd, flags)
    W = eng.KEpsilon(addr, Bd, flags)
    U, Uw, bdc, by, bnuw, bnutw = [dev(x) for x in I["U"]], [dev(x) for x in I["Uw"]], dev(I["bdc"]), dev(I["by"]), dev(I["bnuw"]), dev(I["bnutw"])
    Gw, omw, bom = E(n), E(n), E(nb)
    wgood = dict(coeffs=K, k=k, u=U, b_uw=Uw, b_delta_coeffs=bdc, b_y=by, b_nuw=bnuw, b_nutw=bnutw, g_inout=Gw, omega_inout=omw, b_omega_out=bom)
    for kw, why in ((dict(k=None), "missing"), (dict(u=[U[0], None, U[2]]), "missing"), (dict(b_uw=None), "missing"), (dict(b_y=None), "missing"),
                    (dict(g_inout=None), "missing"), (dict(b_omega_out=None), "missing"), (dict(coeffs=None), "coefficients"), (dict(coeffs=broken), "above zero"),
                    (dict(g_inout=k), "alias"), (dict(b_omega_out=by), "alias"), (dict(omega_inout=Gw), "differ"), (dict(b_nuw=bad), "aligned"),
                    (dict(omega_inout=bad), "aligned")):
        args = dict(wgood)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            W.sst_wall_cells(**args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == fill)) for t in o + [Gw, omw, bom, bad.t])
    assert same(host(k), I["k"]) and same(host(om), I["omega"]) and same(host(nu_f), I["nu_f"]) and same(host(su), R["blend"][(False, "nu")]["su"])
    A.sst_production(nut, grad, o[0], o[1], o[2])                 # the valid calls after them write every value
    A.sst_blend(**dict(good, f1_out=o[3], su_out=o[4], sp_out=o[5], susp_out=o[6], domega_out=o[7], dk_out=o[8], cdkomega_out=o[9], arg1_out=None, f23_out=None,
                       tanh3_out=None))
    W.sst_wall_cells(**wgood)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(t == fill)) for t in o)
    wall = torch.from_numpy(wall_mask(L)).to("cuda:0")
    assert not bool(torch.any(bom[wall] == fill)) and bool(torch.all(bom[~wall] == fill))
    # zero wall patches, zero cells: MI_OK and nothing written
    none = eng.KEpsilon(addr, Bd, [False] * len(flags))
    G0 = E(n)
    none.sst_wall_cells(K, k, U, Uw, bdc, by, bnuw, bnutw, G0, E(n), E(nb))
    torch.cuda.synchronize()
    assert bool(torch.all(G0 == fill))
    empty = E(0)
    A.sst_k_terms(K, empty, empty, empty, empty, empty)
    A.sst_nut(K, False, empty, empty, empty, empty, 1e-4, empty)
    A.sst_omega_sources(empty, empty, empty, empty, empty, empty, empty)
    for h in (none, W, Bd):
        h.close()
