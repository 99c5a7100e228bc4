"""The LES block on the device (Smagorinsky, oneEqEddy, dynOneEqEddy, cubeRootVolDelta, simpleFilter): mi_les_simple_filter,
mi_les_delta_cube_root_vol, mi_les_smagorinsky, mi_les_k_terms, mi_les_nusgs and the four maps of the dynamic procedure, bit for bit against
the restatement of tests/les_support.py."""
import os
import re

import numpy as np
import pytest

import les_support as S
from assembly_support import bits, gpu_env, same, set_face_grid
from turbulence_support import ALL_MESHES, BIG, POW_LOG_BOUND, boundary_cells, mesh, restate_production

EXPORTS = ("mi_les_coeffs_init", "mi_les_simple_filter", "mi_les_delta_cube_root_vol", "mi_les_smagorinsky", "mi_les_k_terms", "mi_les_nusgs",
           "mi_les_dyn_moments", "mi_les_dyn_level1", "mi_les_dyn_level2", "mi_les_dyn_coeffs")
NAN = float("nan")
SEED = {"box": 5000, "edge_257": 5100, "isolated": 5200, BIG: 5300}
WIDTHS = (1, 2, 3, 6, 8, 9)
_CACHE, _CHAINS = {}, {}


def same_n(a, b):
    """bit for bit, signed zeros included; a NaN equals a NaN (the sign and payload of a NaN are the machine's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def same_all(xs, ys):
    """same_n over nested lists of arrays"""
    if isinstance(xs, (list, tuple)):
        return len(xs) == len(ys) and all(same_all(x, y) for x, y in zip(xs, ys))
    return same_n(xs, ys)


def _case(pkg, name):
    """the mesh, its inputs and the restated results, computed once and left unchanged"""
    if name not in _CACHE:
        L = mesh(pkg, name)
        I = S.inputs(pkg.synthetic, L, SEED[name])
        delta, root = S.restate_delta(I["delta_coeff"], 0.0, I["V"])
        I["delta"], I["nueff"] = delta, I["nusgs"] + I["nu"]
        ck, ce = S.DEFAULTS
        R = dict(filter=S.restate_filter(L, I["lam"], I["magSf"], I["bms"], I["vf"], I["bvf"]), delta=(delta, root),
                 delta2=S.restate_delta(I["delta_coeff"], I["thickness"], I["V"]), smag=S.restate_smagorinsky(ck, ce, delta, I["grad"]),
                 kt=S.restate_k_terms(ce, I["nusgs"], I["grad"], I["k"], delta, I["nu"]),
                 kt_f=S.restate_k_terms(I["ce_f"], I["nusgs"], I["grad"], I["k"], delta, I["nu_f"]), nusgs=S.restate_nusgs(ck, I["k"], delta),
                 nusgs_f=S.restate_nusgs(I["ck_f"], I["k"], delta), coeffs=S.restate_coeffs(I["lm"], I["mmmm"], I["num"], I["den"]))
        _CACHE[name] = dict(L=L, I=I, R=R)
    return _CACHE[name]


def _chain(pkg, name, clip, p15=None, bp15=None):
    """the dynamic procedure restated on the case's inputs, once per (mesh, clip, the pow values it continues from)"""
    key = (name, clip, None if p15 is None else p15.tobytes(), None if bp15 is None else bp15.tobytes())
    if key not in _CHAINS:
        c = _case(pkg, name)
        _CHAINS[key] = S.restate_chain(c["L"], c["I"], c["I"]["delta"], c["I"]["nueff"], clip, p15=p15, bp15=bp15)
    return _CHAINS[key]


def _faceless(L):
    return (np.bincount(L["lo"], minlength=L["n"]) + np.bincount(L["up"], minlength=L["n"]) + np.bincount(boundary_cells(L), minlength=L["n"])) == 0


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    for word in ("Smagorinsky", "oneEqEddy", "dynOneEqEddy", "simpleFilter", "cubeRootVolDelta", "mi_les_coeffs"):
        assert word in header, word
    ke_block = header[header.index("the kEpsilon turbulence model"):header.index("typedef struct mi_ke_coeffs")]
    assert "LES models" not in ke_block


def test_coefficients(pkg):
    K = pkg.engine.les_coeffs()
    assert (K.ck, K.ce) == S.DEFAULTS == (0.094, 1.048)
    K2 = pkg.engine.les_coeffs(0.07, 1.05)
    assert (K2.ck, K2.ce) == (0.07, 1.05)
    for bad in (dict(ck=0.0), dict(ck=-0.094), dict(ck=NAN), dict(ck=float("inf")), dict(ce=0.0), dict(ce=-1.0), dict(ce=NAN), dict(ce=float("inf"))):
        with pytest.raises(pkg.engine.MiError, match="above zero"):
            pkg.engine.les_coeffs(**bad)


@pytest.mark.parametrize("name", ALL_MESHES)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg, name):
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    ck, ce = S.DEFAULTS
    delta, root = R["delta"]
    assert same_all(S.literal_filter(L, I["lam"], I["magSf"], I["bms"], I["vf"], I["bvf"]), R["filter"])
    # the roots: math.pow and numpy's power may differ, so the literal form continues from the restatement's; sqrt is correctly rounded
    assert same_all(S.literal_delta(I["delta_coeff"], 0.0, I["V"], root=root), list(R["delta"]))
    assert same_all(S.literal_delta(I["delta_coeff"], I["thickness"], I["V"]), list(R["delta2"]))
    assert same_all(S.literal_smagorinsky(ck, ce, delta, I["grad"]), list(R["smag"]))
    assert same_all(S.literal_k_terms(ce, I["nusgs"], I["grad"], I["k"], delta, I["nu"]), list(R["kt"]))
    assert same_all(S.literal_k_terms(I["ce_f"], I["nusgs"], I["grad"], I["k"], delta, I["nu_f"]), list(R["kt_f"]))
    assert same_n(S.literal_nusgs(ck, I["k"], delta), R["nusgs"]) and same_n(S.literal_nusgs(I["ck_f"], I["k"], delta), R["nusgs_f"])
    assert same_all(S.literal_coeffs(I["lm"], I["mmmm"], I["num"], I["den"]), list(R["coeffs"]))
    # mi_les_dyn_coeffs alone: each coefficient clipped to exactly +0 in 10 to 90 % of the cells; f_mmmm == 0 reached, VSMALL decides
    for x in R["coeffs"]:
        zero = (x == 0.0)
        assert 0.1 <= zero.mean() <= 0.9 and not np.any(np.signbit(x[zero])) and np.all(x[~zero] > 0)
    at0 = I["mmmm"] == 0.0
    assert np.any(at0 & (I["lm"] > 0)) and np.all(np.isfinite(R["coeffs"][0])) and np.any(R["coeffs"][0][at0] > 1e290)
    assert np.any(at0 & (I["lm"] == 0.0)) and np.all(R["coeffs"][0][at0 & (I["lm"] == 0.0)] == 0.0)    # 0/VSMALL, not 0/0
    # the chain, clipped (correct()) and not (the constructor): the literal maps and filter against the vectorised ones from the same pow values
    faceless = _faceless(L)
    assert np.any(faceless) == (name == "isolated")
    lit = dict(moments=S.literal_moments, level1=S.literal_level1, level2=S.literal_level2, coeffs=S.literal_coeffs)
    for clip in (1, 0):
        C = _chain(pkg, name, clip)
        D = S.restate_chain(L, I, delta, I["nueff"], clip, p15=C["p"], bp15=C["bp"], flt=S.literal_filter, maps=lit)
        assert set(C) == set(D)
        for key in sorted(C):
            assert same_all(D[key], C[key]), (clip, key)
    C1, C0 = _chain(pkg, name, 1), _chain(pkg, name, 0)
    quiet, c0 = I["quiet"], I["c0"]
    assert np.any(C1["KK"] == S.SMALL) and np.any(C1["KK"] > S.SMALL) and np.all(C1["KK"][~faceless] >= S.SMALL)
    assert np.all(C1["KK"][~quiet & ~faceless] > S.SMALL), "off the quiet region KK is a variance of seeded values"
    # without the clip: KK of the quiet region is rounding noise of either sign, and the square root of a negative one is not a number
    neg = C0["KK"] < 0
    assert np.any(neg) and np.all(np.isnan(C0["MM"][0][neg])) and np.all(np.isnan(C0["p"][neg])) and not np.any(neg & ~quiet)
    assert np.all(np.isfinite(C1["MM"][0][~faceless]))
    # three levels in: f_mmmm is exactly 0 at the centre of the quiet region and VSMALL decides the quotient
    assert C1["fmmmm"][c0] == 0.0 and C1["flm"][c0] == 0.0 and C1["ck"][c0] == 0.0 and not np.signbit(C1["ck"][c0])
    for key in ("ck", "ce"):
        x = C1[key][~faceless]
        print(f"{name}: {key} of the chain is exactly 0 in {np.mean(x == 0.0):.2f} of the cells with faces")
    ckz = (C1["ck"][~faceless] == 0.0).mean()
    assert 0.1 <= ckz <= 0.9, ckz
    # ce of the chain: ce_num is a variance under convex weights and so not negative, except where D is constant (the flat region): there it
    # is rounding noise of either sign, the filtered numerator goes negative and ce is clipped to exactly +0
    # (edge_257 has no room for a flat region beside its quiet one)
    below = C1["f2"][12] < 0
    assert np.any(I["flat"]) == (name != "edge_257") and not np.any((C1["num"] < 0) & ~I["flat"])
    if np.any(I["flat"]):
        assert np.any(C1["num"] < 0)
    assert np.any(below) or name not in ("box", BIG)            # where three rings fit, the filtered numerator is negative in some cell
    assert np.all(C1["ce"][below] == 0.0) and not np.any(np.signbit(C1["ce"][below])) and np.any(C1["ce"] > 0)
    # the boundary's delta is SMALL: MM_b all but vanishes, ce_den_b is enormous
    live = ~quiet[boundary_cells(L)]
    assert np.all(np.abs(C1["bMM"][0][live]) < 1e-12) and np.all(C1["bden"][live] > 1e8)
    if name == "isolated":                                        # 0/0 in the cells without faces, for every filtered component
        for key in ("f1", "f2"):
            assert all(np.all(np.isnan(x[faceless])) for x in C1[key])
        assert all(np.all(np.isnan(x[faceless])) for x in R["filter"]) and np.all(np.isnan(C1["flm"][faceless])) and np.all(np.isnan(C1["fmmmm"][faceless]))
        assert not any(np.any(np.isnan(x[~faceless])) for x in R["filter"])


@pytest.mark.parametrize("name", ALL_MESHES)
def test_each_stated_rounding_changes_a_compared_bit(pkg, name):
    """the contraction of &&, of magSqr(Vector) and of magSqr(SymmTensor), the uncontracted dev and difference fSqrU - sqr(fU), the rounded
    product of the filter, its division, its interpolate and the grouping of nuSgs each change a compared bit when altered; the doubling of
    nuSgs in G and the halving of ce_den are exact, hence EQUAL"""
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    ck, ce = S.DEFAULTS
    delta = I["delta"]
    C = _chain(pkg, name, 1)
    f1 = C["f1"]
    fU, fS, fMU, fD, fMD = f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16]
    args = (1, delta, I["nueff"], fU, fS, fMU, fD, fMD)
    base = S.restate_level1(*args, p15=C["p"])
    assert same_all(list(base), [C[k] for k in ("KK", "LL", "MM", "num", "den", "p")])
    assert not same_all(S.restate_level1(*args, p15=C["p"], dev_contracted=True)[1], C["LL"])
    assert not same_all(S.restate_level1(*args, p15=C["p"], fused_difference=True)[1], C["LL"])
    assert not same_n(S.restate_level1(0, *args[1:], p15=C["p"], magsqr_contracted=False)[0], S.restate_level1(0, *args[1:], p15=C["p"])[0])
    assert not same_n(S.restate_smagorinsky(ck, ce, delta, I["grad"], dev_contracted=True)[1], R["smag"][1])
    assert not same_n(S.restate_moments(I["U"], I["grad"], contracted=False)[1], C["mu"])
    assert not same_n(S.magsqr_st(C["D"], contracted=False), C["md"])
    f2 = C["f2"]
    assert not same_n(S.restate_level2(f2[0:6], f2[6:12], contracted=False)[0], C["lm"])
    flt = (L, I["lam"], I["magSf"], I["bms"], I["vf"], I["bvf"])
    for alt in (dict(fused=True), dict(reciprocal=True), dict(plain_interpolate=True)):
        other = S.restate_filter(*flt, **alt)
        assert all(not same_n(a, b) for a, b in zip(other, R["filter"])), alt
    assert not same_n(S.restate_nusgs(ck, I["k"], delta, regroup=True), R["nusgs"])
    # exact: (2.0*nuSgs)*m is (nuSgs*2.0)*m, the bits of mi_ke_production; p/(2.0*delta) is 0.5*(p/delta)
    assert same_n(R["kt"][0], restate_production(I["nusgs"], I["grad"]))
    with np.errstate(all="ignore"):
        assert same_n(0.5 * (C["p"] / delta), C["den"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert same_n(got, want), (tag, int(np.sum(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))) if got.shape == want.shape else "shape")


def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _boundary(eng, addr, L):
    return eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(L["patches"]))


def _odd(dev, a):
    """the same values at an address that is 8 bytes past a 16-byte boundary: the one-cell-at-a-time form of the cell passes"""
    return dev(np.concatenate([[0.0], a]))[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_simple_filter(pkg, monkeypatch, name, blocks):
    """n_cmpt = 1, 2, 3, 6, 8, 9 against the restatement and against the engine's own unfused sequence (mi_face_interpolate, then
    mi_fvc_average, per component); the outputs beyond n_cmpt and a fill pattern around the output arrays stay untouched"""
    import torch
    set_face_grid(monkeypatch, blocks)
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, nf, pad = L["n"], L["lo"].shape[0], 6
    for tag, addr in _addressings(eng, ctx, L):
        A, B = eng.Assembly(addr), _boundary(eng, addr, L)
        magSf, bms, lam = dev(I["magSf"]), dev(I["bms"]), dev(I["lam"])
        H = eng.Average(addr, B, magSf, bms)
        vf, bvf = [dev(x) for x in I["vf"]], [dev(x) for x in I["bvf"]]
        unfused = []
        for x, bx in zip(vf, bvf):
            face, avg = E(max(nf, 1)), E(n)
            A.face_interpolate(lam, x, face)
            A.fvc_average(H, magSf, face, avg, bms, bx)
            unfused.append(host(avg))
        for w in WIDTHS:
            slab = E(9 * (n + pad) + pad)                         # nine outputs with a fill pattern before, between and after them
            out = [slab[pad + k * (n + pad):pad + k * (n + pad) + n] for k in range(9)]
            A.les_simple_filter(H, lam, magSf, vf, out, bms, bvf, n_cmpt=w)
            got = host(slab)
            keep = np.ones(got.shape[0], dtype=bool)
            for k in range(w):
                a = pad + k * (n + pad)
                keep[a:a + n] = False
                _eq(got[a:a + n], R["filter"][k], (name, tag, blocks, w, k, "restatement"))
                _eq(got[a:a + n], unfused[k], (name, tag, blocks, w, k, "unfused sequence"))
            assert np.all(got[keep] == fill), (name, tag, blocks, w)
        H.close(); B.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_cell_passes(pkg, monkeypatch, name, blocks):
    """every cell pass with 16-byte aligned arrays (two cells per thread) and with arrays 8 bytes off (one by one); MI_FACE_GRID at its default
    and forced to 1 and 3 workgroups.  The device's pow is not the host's: the root of delta and pow(KK, 1.5) within POW_LOG_BOUND of numpy,
    everything after them bit for bit when the restatement continues from the device's values.  G against mi_ke_production bit for bit."""
    import torch
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, K = L["n"], eng.les_coeffs()
    ck, ce = S.DEFAULTS
    C = _chain(pkg, name, 1)
    f1, f2 = C["f1"], C["f2"]
    worst = 0.0
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    A = eng.Assembly(addr)
    for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
        tag = (name, blocks, "aligned" if put is dev else "8 bytes off")
        puts = lambda xs: [put(x) for x in xs]
        outs = lambda m: [out(n) for _ in range(m)]
        # delta: 3-D and 2-D
        d, r = out(n), out(n)
        A.les_delta_cube_root_vol(I["delta_coeff"], 0.0, put(I["V"]), d, r)
        rh = host(r)
        dev_rel = np.max(np.abs(rh / R["delta"][1] - 1.0))
        worst = max(worst, dev_rel)
        assert dev_rel <= POW_LOG_BOUND, dev_rel * 2.0 ** 52
        _eq(host(d), S.restate_delta(I["delta_coeff"], 0.0, I["V"], root=rh)[0], tag + ("delta",))
        d1 = out(n)
        A.les_delta_cube_root_vol(I["delta_coeff"], 0.0, put(I["V"]), d1)
        _eq(host(d1), host(d), tag + ("delta without the root",))
        d2, r2 = out(n), out(n)
        A.les_delta_cube_root_vol(I["delta_coeff"], I["thickness"], put(I["V"]), d2, r2)
        _eq(host(d2), R["delta2"][0], tag + ("delta 2-D",)); _eq(host(r2), R["delta2"][1], tag + ("sqrt",))
        # Smagorinsky, the k equation's terms, nuSgs
        delta, grad, k, nusgs = put(I["delta"]), puts(I["grad"]), put(I["k"]), put(I["nusgs"])
        nus, ks = out(n), out(n)
        A.les_smagorinsky(K, delta, grad, nus, ks)
        _eq(host(nus), R["smag"][0], tag + ("nuSgs",)); _eq(host(ks), R["smag"][1], tag + ("k",))
        nus1 = out(n)
        A.les_smagorinsky(K, delta, grad, nus1)
        _eq(host(nus1), R["smag"][0], tag + ("nuSgs alone",))
        for cev, nuv, key in ((ce, I["nu"], "kt"), (put(I["ce_f"]), put(I["nu_f"]), "kt_f")):
            G, sp, dk = outs(3)
            A.les_k_terms(cev, nusgs, grad, k, delta, nuv, G, sp, dk)
            for got, want, what in zip((G, sp, dk), R[key], ("G", "sp", "dk")):
                _eq(host(got), want, tag + (key, what))
            Gk = out(n)
            A.ke_production(nusgs, grad, Gk)
            _eq(host(G), host(Gk), tag + ("G against mi_ke_production",))
        for ckv, key in ((ck, "nusgs"), (put(I["ck_f"]), "nusgs_f")):
            o = out(n)
            A.les_nusgs(ckv, k, delta, o)
            _eq(host(o), R[key], tag + (key,))
        # the maps of the dynamic procedure on the chain's own intermediates
        sq, D = outs(6), outs(6)
        mu, md = out(n), out(n)
        A.les_dyn_moments(puts(I["U"]), grad, sq, mu, D, md)
        for got, want, what in ((sq, C["sq"], "sqr(U)"), (D, C["D"], "D")):
            for g, w_ in zip(got, want):
                _eq(host(g), w_, tag + (what,))
        _eq(host(mu), C["mu"], tag + ("magSqr(U)",)); _eq(host(md), C["md"], tag + ("magSqr(D)",))
        for clip in (1, 0):
            KK, num, den, pw = outs(4)
            LL, MM = outs(6), outs(6)
            A.les_dyn_level1(clip, delta, put(I["nueff"]), puts(f1[0:3]), puts(f1[3:9]), put(f1[9]), puts(f1[10:16]), put(f1[16]), KK, LL, MM, num, den, pw)
            ph = host(pw)
            want = S.restate_level1(clip, I["delta"], I["nueff"], f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16], p15=ph)
            ref = _chain(pkg, name, clip)["p"]
            ok = np.isfinite(ref) & (ref > 0)
            assert np.array_equal(np.isnan(ph), np.isnan(ref))
            rel = np.max(np.abs(ph[ok] / ref[ok] - 1.0))
            worst = max(worst, rel)
            assert rel <= POW_LOG_BOUND, rel * 2.0 ** 52
            _eq(host(KK), want[0], tag + (clip, "KK")); _eq(host(num), want[3], tag + (clip, "ce_num")); _eq(host(den), want[4], tag + (clip, "ce_den"))
            for g, w_ in zip(LL + MM, want[1] + want[2]):
                _eq(host(g), w_, tag + (clip, "LL / MM"))
            if clip:
                KK1, num1, den1 = outs(3)
                LL1, MM1 = outs(6), outs(6)
                A.les_dyn_level1(clip, delta, put(I["nueff"]), puts(f1[0:3]), puts(f1[3:9]), put(f1[9]), puts(f1[10:16]), put(f1[16]), KK1, LL1, MM1, num1, den1)
                _eq(host(den1), host(den), tag + ("ce_den without the pow output",)); _eq(host(MM1[5]), host(MM[5]), tag + ("MM without the pow output",))
        lm, mmmm = outs(2)
        A.les_dyn_level2(puts(f2[0:6]), puts(f2[6:12]), lm, mmmm)
        _eq(host(lm), C["lm"], tag + ("lm",)); _eq(host(mmmm), C["mmmm"], tag + ("mmmm",))
        cko, ceo = outs(2)
        A.les_dyn_coeffs(put(I["lm"]), put(I["mmmm"]), put(I["num"]), put(I["den"]), cko, ceo)
        _eq(host(cko), R["coeffs"][0], tag + ("ck",)); _eq(host(ceo), R["coeffs"][1], tag + ("ce",))
    print(f"{name}: largest relative deviation of the device's pow from numpy in units of 2^-52: {worst * 2.0 ** 52:.2f}")
    torch.cuda.synchronize()


def _device_chain(eng, A, H, g, dev, host, E, L, I, clip):
    """dynOneEqEddy.C:56-100 on the device: four cell passes (each also over the boundary arrays, delta_b = SMALL) and five filter launches"""
    import torch
    n, nb = L["n"], I["bms"].shape[0]
    bc = torch.from_numpy(boundary_cells(L).astype(np.int64)).to("cuda:0")
    F = lambda vf, bvf: (lambda out: (H.les_simple_filter(g["lam"], g["magSf"], vf, out, g["bms"], bvf), out)[1])([E(n) for _ in vf])
    zg = lambda xs: [x[bc].contiguous() for x in xs]              # the zero-gradient boundary values of a filtered field
    devs = lambda xs: [dev(x) for x in xs]
    out = {}
    fields = {}
    for side, m, U, grad in (("", n, devs(I["U"]), devs(I["grad"])), ("b", nb, devs(I["bU"]), devs(I["bgrad"]))):
        sq, D, mu, md = [E(m) for _ in range(6)], [E(m) for _ in range(6)], E(m), E(m)
        A.les_dyn_moments(U, grad, sq, mu, D, md)
        fields[side] = (U, sq, mu, D, md)
        out.update({side + "sq": sq, side + "mu": mu, side + "D": D, side + "md": md})
    (U, sq, mu, D, md), (bU, bsq, bmu, bD, bmd) = fields[""], fields["b"]
    f1 = F(U + sq, bU + bsq) + F([mu] + D + [md], [bmu] + bD + [bmd])                    # 9 + 8
    out["f1"] = f1
    fU, fS, fMU, fD, fMD = f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16]
    lv = {}
    for side, m, delta, nueff, a in (("", n, dev(I["delta"]), dev(I["nueff"]), (fU, fS, [fMU], fD, [fMD])),
                                     ("b", nb, dev(np.full(nb, S.SMALL)), dev(I["bnueff"]), tuple(zg(x) for x in (fU, fS, [fMU], fD, [fMD])))):
        KK, num, den, pw = [E(m) for _ in range(4)]
        LL, MM = [E(m) for _ in range(6)], [E(m) for _ in range(6)]
        A.les_dyn_level1(clip, delta, nueff, a[0], a[1], a[2][0], a[3], a[4][0], KK, LL, MM, num, den, pw)
        lv[side] = (LL, MM, num, den)
        out.update({side + "KK": KK, side + "LL": LL, side + "MM": MM, side + "num": num, side + "den": den, side + "p": pw})
    (LL, MM, num, den), (bLL, bMM, bnum, bden) = lv[""], lv["b"]
    f2 = F(LL + MM[0:3], bLL + bMM[0:3]) + F(MM[3:6] + [num, den], bMM[3:6] + [bnum, bden])   # 9 + 5
    out["f2"] = f2
    fLL, fMM = f2[0:6], f2[6:12]
    lm, mmmm, blm, bmmmm = E(n), E(n), E(nb), E(nb)
    A.les_dyn_level2(fLL, fMM, lm, mmmm)
    A.les_dyn_level2(zg(fLL), zg(fMM), blm, bmmmm)
    flm, fmmmm = F([lm, mmmm], [blm, bmmmm])
    ck, ce = E(n), E(n)
    A.les_dyn_coeffs(flm, fmmmm, f2[12], f2[13], ck, ce)
    out.update(lm=lm, mmmm=mmmm, blm=blm, bmmmm=bmmmm, flm=flm, fmmmm=fmmmm, ck=ck, ce=ce)
    return {key: [host(x) for x in v] if isinstance(v, list) else host(v) for key, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_dynamic_procedure_end_to_end(pkg, monkeypatch, name, blocks):
    """the chain of dynOneEqEddy::ck and ::ce on the cells and on the boundary arrays with delta_b = SMALL, clipped as correct() and unclipped
    as the constructor: every intermediate, ck and ce bit for bit against the restatement continued from the device's pow values"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I = c["L"], c["I"]
    for tag, addr in _addressings(eng, ctx, L):
        A, B = eng.Assembly(addr), _boundary(eng, addr, L)
        g = {key: dev(I[key]) for key in ("lam", "magSf", "bms")}
        H = eng.Average(addr, B, g["magSf"], g["bms"])
        for clip in (1, 0):
            got = _device_chain(eng, A, H, g, dev, host, E, L, I, clip)
            want = _chain(pkg, name, clip, p15=got["p"], bp15=got["bp"])
            assert set(got) == set(want)
            for key in sorted(want):
                if isinstance(want[key], list):
                    for k, (a, b) in enumerate(zip(got[key], want[key])):
                        _eq(a, b, (name, tag, blocks, clip, key, k))
                else:
                    _eq(got[key], want[key], (name, tag, blocks, clip, key))
        H.close(); B.close()


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
    L, I = c["L"], c["I"]
    n, K = L["n"], eng.les_coeffs()
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    A, B = eng.Assembly(addr), _boundary(eng, addr, L)
    bad = Misaligned(E(n + 1))
    magSf, bms, lam = dev(I["magSf"]), dev(I["bms"]), dev(I["lam"])
    H = eng.Average(addr, B, magSf, bms)
    vf, bvf = [dev(x) for x in I["vf"]], [dev(x) for x in I["bvf"]]
    o = [E(n) for _ in range(16)]
    # the filter: n_cmpt, missing, alias (before alignment), alignment, the boundary arrays
    for kw, why in ((dict(n_cmpt=0), "1 to 9"), (dict(n_cmpt=10), "1 to 9"), (dict(lam=None), "missing"), (dict(mag_sf=None), "missing"),
                    (dict(vf=None), "missing"), (dict(vf=vf[:2] + [None]), "missing"), (dict(out=None), "missing"), (dict(out=o[:2] + [None]), "missing"),
                    (dict(b_mag_sf=None), "boundary has faces"), (dict(b_face=None), "boundary has faces"), (dict(b_face=bvf[:2] + [None]), "boundary has faces"),
                    (dict(out=[o[0], o[1], vf[0]]), "alias"), (dict(out=[o[0], o[1], vf[2]]), "alias"), (dict(out=[o[0], lam, o[2]]), "alias"),
                    (dict(out=[o[0], bvf[1], o[2]]), "alias"), (dict(out=[o[0], o[1], o[0]]), "differ"), (dict(out=[o[0], o[1], bad]), "aligned"),
                    (dict(vf=[vf[0], bad, vf[2]]), "aligned"), (dict(lam=bad), "aligned"), (dict(vf=[vf[0], bad, vf[2]], out=[o[0], o[1], vf[0]]), "alias")):
        args = dict(lam=lam, mag_sf=magSf, vf=vf[:3], out=o[:3], b_mag_sf=bms, b_face=bvf[:3])
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            H.les_simple_filter(**args)
    # the cell passes
    delta, grad, k, nusgs, nu_f, U = dev(I["delta"]), [dev(x) for x in I["grad"]], dev(I["k"]), dev(I["nusgs"]), dev(I["nu_f"]), [dev(x) for x in I["U"]]
    broken = eng.les_coeffs()
    broken.ce = NAN
    for args, why in (((1.0, 0.0, None, o[0]), "missing"), ((1.0, 0.0, k, None), "missing"), ((1.0, 0.0, k, k), "alias"), ((1.0, 0.0, k, o[0], o[0]), "differ"),
                      ((1.0, 0.0, k, bad), "aligned"), ((NAN, 0.0, k, o[0]), "finite"), ((1.0, -1.0, k, o[0]), "finite")):
        with pytest.raises(eng.MiError, match=why):
            A.les_delta_cube_root_vol(*args)
    for args, why in (((K, None, grad, o[0]), "missing"), ((K, delta, grad[:8] + [None], o[0]), "missing"), ((K, delta, None, o[0]), "missing"),
                      ((K, delta, grad, None), "missing"), ((K, delta, grad, grad[3]), "alias"), ((K, delta, grad, o[0], o[0]), "differ"),
                      ((K, delta, grad, bad), "aligned"), ((None, delta, grad, o[0]), "coefficients"), ((broken, delta, grad, o[0]), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            A.les_smagorinsky(*args)
    for args, why in (((1.048, None, grad, k, delta, 1e-5, *o[:3]), "missing"), ((1.048, nusgs, grad, k, delta, 1e-5, o[0], o[1], None), "missing"),
                      ((1.048, nusgs, grad, k, delta, nu_f, o[0], o[1], nu_f), "alias"), ((1.048, nusgs, grad, k, delta, 1e-5, o[0], o[0], o[2]), "differ"),
                      ((1.048, nusgs, grad, k, delta, bad, *o[:3]), "aligned"), ((0.0, nusgs, grad, k, delta, 1e-5, *o[:3]), "above zero"),
                      ((NAN, nusgs, grad, k, delta, 1e-5, *o[:3]), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            A.les_k_terms(*args)
    for args, why in (((0.094, None, delta, o[0]), "missing"), ((0.094, k, delta, delta), "alias"), ((0.094, k, delta, bad), "aligned"), ((-1.0, k, delta, o[0]), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            A.les_nusgs(*args)
    for args, why in (((None, grad, o[0:6], o[6], o[7:13], o[13]), "missing"), ((U, grad, o[0:5] + [None], o[6], o[7:13], o[13]), "missing"),
                      ((U, grad, o[0:6], U[0], o[7:13], o[13]), "alias"), ((U, grad, o[0:6], o[6], o[7:13], o[0]), "differ"), ((U, grad, o[0:6], bad, o[7:13], o[13]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.les_dyn_moments(*args)
    f = [dev(x) for x in I["vf"]] + [dev(x) for x in I["vf"]]
    good1 = (1, delta, nusgs, f[0:3], f[3:9], f[9], f[10:16], f[16], o[0], o[1:7], o[7:13], o[13], o[14], o[15])
    for pos, value, why in ((1, None, "missing"), (4, f[3:8] + [None], "missing"), (8, None, "missing"), (8, delta, "alias"), (12, o[0], "differ"), (13, o[0], "differ"),
                            (11, bad, "aligned"), (2, bad, "aligned")):
        args = list(good1)
        args[pos] = value
        with pytest.raises(eng.MiError, match=why):
            A.les_dyn_level1(*args)
    for args, why in (((f[0:6], None, o[0], o[1]), "missing"), ((f[0:6], f[6:12], f[0], o[1]), "alias"), ((f[0:6], f[6:12], o[0], o[0]), "differ"),
                      ((f[0:6], f[6:12], o[0], bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.les_dyn_level2(*args)
    for args, why in (((None, f[1], f[2], f[3], o[0], o[1]), "missing"), ((f[0], f[1], f[2], f[3], f[3], o[1]), "alias"), ((f[0], f[1], f[2], f[3], o[0], o[0]), "differ"),
                      ((f[0], bad, f[2], f[3], o[0], o[1]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.les_dyn_coeffs(*args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(y == fill)) for y in o + [bad.t])
    assert same(host(vf[0]), I["vf"][0]) and same(host(delta), I["delta"]) and same(host(lam), I["lam"]) and same(host(nu_f), I["nu_f"])
    # the valid calls after them write every value
    H.les_simple_filter(lam, magSf, vf[:3], o[:3], bms, bvf[:3])
    A.les_dyn_level1(*good1)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == fill)) for y in o)
    for h in (H, B):
        h.close()


def _les_channel_walk(pkg, orc, model, ordered):
    """The constructor and three correct() steps of one model (Smagorinsky.C:76-89, oneEqEddy.C:90-122, dynOneEqEddy.C:134-172) on the 6 x 5 x 4
    channel of turbulence_support.channel, driven through the Python binding with the engine's assembly, relaxation, PBiCG, mi_bound and the
    zero-gradient nuSgs: every intermediate up to and including the assembled and relaxed matrix and what the solver is handed equals the
    restatement bit for bit; the restatement continues from the engine's solution (and from the device's pow values); k and nuSgs stay finite
    and k >= kMin -> the engine's fields after the constructor and after every step"""
    import torch
    from turbulence_support import channel, patch_coeffs
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    M, S0 = channel(pkg)
    L, n, nf, nb = M["L"], M["n"], M["nf"], M["nb"]
    nu, rdt = M["nu"], 1.0 / M["dt"]
    K = eng.les_coeffs()
    fcs = [fc for fc, _ in L["patches"]]
    addr = eng.Addressing(ctx, n, M["lo"], M["up"], ordered=ordered)
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, fcs, ["fixesValue" if kd == "inlet" else "other" for kd in M["kinds"]])
    patches = [eng.Patch(ctx, n, fc) for fc in fcs]
    cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
    g = {key: dev(M[key]) for key in ("V", "magSf", "dc", "lam", "bms", "phi")}
    AV = eng.Average(addr, B, g["magSf"], g["bms"])
    inlet = torch.from_numpy(M["kind_of"] == "inlet").to("cuda:0")
    mat = eng.Matrix(addr)
    delta = E(n)
    A.les_delta_cube_root_vol(1.0, 0.0, g["V"], delta)
    X0 = dict(delta=host(delta))

    def zero_gradient(cell, inlet_value=None):
        out = E(nb)
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            p.internal_field(cell, out[a:b])
        if inlet_value is not None:
            out[inlet] = inlet_value
        return out

    def bound(v, bv, lb):
        lo = min(A.min_max(v)[0], A.min_max(bv)[0])
        if not lo < lb:
            return False
        A.vec_max_value(bv, lb, bv)
        A.bound(AV, lb, g["lam"], g["magSf"], v, g["bms"], bv)
        return True

    def chain(F, nueff, bnueff, clip):
        I = dict(F, delta=X0["delta"], nueff=nueff, bnueff=bnueff, bms=M["bms"])
        return _device_chain(eng, A, AV, g, dev, host, E, L, I, clip)

    def equation(psi_old, psi, su, sp, gamma, bgamma_h, inlet_value, alpha):
        gam = E(nf)
        A.face_interpolate(g["lam"], gamma, gam)
        gam = gam * g["magSf"]
        upper, lower, diag, source = E(nf), E(nf), E(n), E(n)
        A.assemble(upper, diag, lower, [source], ddt=dict(r_delta_t=rdt, vol=g["V"], psi_old=[psi_old]), div=dict(flux=g["phi"], weights=g["lam"]),
                   laplacian=dict(delta_coeffs=g["dc"], gamma_magsf=gam), sp=(sp, 1.0), su=[(-1.0, [su])])
        out = dict(gam=host(gam), upper0=host(upper), lower0=host(lower), diag0=host(diag), source0=host(source))
        ich, bch = patch_coeffs(M, bgamma_h, inlet_value)
        ic, bc = [dev(x) for x in ich], [dev(x) for x in bch]
        A.relax(alpha, diag, lower, upper, source, psi, patches, ic, bc, [0] * len(patches))
        out.update(diag1=host(diag), source1=host(source))
        ds, ss = diag.clone(), source.clone()
        for p, i, b in zip(patches, ic, bc):
            p.add(i, ds, 0); p.add(b, ss, 0)
        out.update(psi=host(psi), upper=host(upper), lower=host(lower), source=host(source), ic=np.concatenate([host(x) for x in ic]),
                   bc=np.concatenate([host(x) for x in bc]), diag_solve=host(ds), source_solve=host(ss))
        mat.set_coeffs(ds, upper, lower)
        perf = mat.pbicg(psi, ss, "diagonal", tolerance=1e-10, relTol=0.0, maxIter=300)
        assert 0 < perf["nIterations"] < 300
        return out

    def compare(D, want, where):
        assert set(want) == set(D), (where, set(want) ^ set(D))
        for key in sorted(want):
            if isinstance(want[key], bool):
                assert D[key] == want[key], (where, key)
            elif isinstance(want[key], list):
                for j, (a, b) in enumerate(zip(D[key], want[key])):
                    _eq(a, b, (where, key, j))
            else:
                _eq(D[key], want[key], (where, key))

    # the constructor
    St = dict(k=S0["k"], bk=S0["bk"])
    k, bk = dev(St["k"]), dev(St["bk"])
    assert not bound(k, bk, S.SMALL)
    F = S.channel_flow(M, -1)
    D, nusgs = {}, E(n)
    if model == "Smagorinsky":
        A.les_smagorinsky(K, delta, [dev(x) for x in F["grad"]], nusgs, k)
    elif model == "oneEqEddy":
        A.les_nusgs(K.ck, k, delta, nusgs)
    else:
        C = chain(F, np.full(n, nu), np.full(nb, nu), 0)
        X0.update(p=C["p"], bp=C["bp"])
        D.update({"dyn_" + key: v for key, v in C.items()})
        A.les_nusgs(dev(C["ck"]), k, delta, nusgs)
    bnusgs = zero_gradient(nusgs)
    D.update(nusgs=host(nusgs), bnusgs=host(bnusgs))
    want, St = S.restate_les_constructor(model, M, St, X0)
    compare(D, want, "constructor")
    states = [{key: np.array(v) for key, v in St.items()}]
    for step in range(M["steps"]):
        F = S.channel_flow(M, step)
        grad = [dev(x) for x in F["grad"]]
        D, X = {}, dict(delta=X0["delta"])
        if model == "Smagorinsky":
            A.les_smagorinsky(K, delta, grad, nusgs, k)
            bnusgs = zero_gradient(nusgs)
            D.update(k_new=host(k), nusgs=host(nusgs), bnusgs=host(bnusgs))
        else:
            ckv, cev = K.ck, K.ce
            if model == "dynOneEqEddy":
                C = chain(F, host(nusgs) + nu, host(bnusgs) + nu, 1)
                X.update(p=C["p"], bp=C["bp"])
                D.update({"dyn_" + key: v for key, v in C.items()})
                ckv, cev = dev(C["ck"]), dev(C["ce"])
            G, sp, dk = E(n), E(n), E(n)
            A.les_k_terms(cev, nusgs, grad, k, delta, nu, G, sp, dk)
            D.update(G=host(G), sp=host(sp), dk=host(dk))
            q = equation(k.clone(), k, G, sp, dk, host(bnusgs) + nu, M["k_in"], M["alpha_k"])
            D.update({"k_" + key: v for key, v in q.items()})
            X["k_solved"] = host(k).copy()
            bk = zero_gradient(k, M["k_in"])
            D["k_bounded"] = bound(k, bk, S.SMALL)
            A.les_nusgs(ckv, k, delta, nusgs)
            bnusgs = zero_gradient(nusgs)
            D.update(k_new=host(k), bk_new=host(bk), nusgs=host(nusgs), bnusgs=host(bnusgs))
        want, St = S.restate_les_correct(model, orc, M, St, X, step)
        compare(D, want, (model, step))
        for key in ("k", "bk", "nusgs", "bnusgs"):
            assert np.all(np.isfinite(St[key])), (step, key)
        assert np.all(St["k"] >= S.SMALL) and np.all(St["nusgs"] >= 0)
        print(f"{model} step {step}: k {St['k'].min():.3e}..{St['k'].max():.3e}  nuSgs {St['nusgs'].min():.3e}..{St['nusgs'].max():.3e}")
        states.append({key: np.array(v) for key, v in St.items()})
    for h in (AV, B):
        h.close()
    return M, states


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["caller", "ordered"])
@pytest.mark.parametrize("model", S.MODELS)
def test_channel_walk(pkg, orc, model, ordered):
    """_les_channel_walk for each model under the caller's numbering and under ordered addressing"""
    _les_channel_walk(pkg, orc, model, ordered)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------
def test_mirror_declares_the_les_classes(pkg):
    """foam/miFoam: LESdelta / cubeRootVolDelta, simpleFilter and incompressible::LESModels::Smagorinsky, oneEqEddy and dynOneEqEddy with the
    reference's members are declared and in the library"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    for word in ("class LESdelta", "class cubeRootVolDelta", "class simpleFilter", "namespace LESModels", "class GenEddyVisc", "class Smagorinsky",
                 "class oneEqEddy", "class dynOneEqEddy", "k() const", "nuSgs() const", "nuEff(", "DkEff(", "divDevReff(", "void correct("):
        assert word in text, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    les = "Foam::incompressible::LESModels::"
    for name in ("Foam::LESdelta::LESdelta(", "Foam::cubeRootVolDelta::cubeRootVolDelta(", "Foam::simpleFilter::simpleFilter(", "Foam::simpleFilter::operator()(",
                 les + "GenEddyVisc::nuEff(", les + "GenEddyVisc::DkEff(", les + "GenEddyVisc::divDevReff(", les + "Smagorinsky::Smagorinsky(",
                 les + "Smagorinsky::correct(", les + "oneEqEddy::oneEqEddy(", les + "oneEqEddy::correct(", les + "dynOneEqEddy::dynOneEqEddy(",
                 les + "dynOneEqEddy::correct("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("model", S.MODELS)
def test_mirror_les_walks_the_channel(pkg, orc, tmp_path, model):
    """foam/miFoam's LES classes -- the constructor and three correct() calls of each model, through the driver foam/lesChannel.C in a process
    of its own, with the solver of the walk (PBiCG, diagonal, 1e-10) -- give k, nuSgs and their boundary values of the Python walk bit for bit
    after the constructor and after every step"""
    import subprocess
    from turbulence_support import channel
    M, states = _les_channel_walk(pkg, orc, model, False)
    L, S0 = M["L"], channel(pkg)[1]
    d = str(tmp_path)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{model} {M['n']} {M['nf']} {M['steps']} {repr(1.0 / M['dt'])} {repr(M['nu'])} {repr(M['alpha_k'])} {len(M['kinds'])}\n")
        for (fc, _), kd in zip(L["patches"], M["kinds"]):
            f.write(f"{fc.shape[0]} {0 if kd == 'inlet' else 1}\n")
    put = lambda name, a, dt=np.float64: np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name + ".bin"))
    put("lower", M["lo"], np.int32); put("upper", M["up"], np.int32); put("faceCells", boundary_cells(L), np.int32)
    for name, key in (("weights", "lam"), ("deltaCoeffs", "dc"), ("magSf", "magSf"), ("V", "V"), ("bMagSf", "bms"), ("bDeltaCoeffs", "bdc"), ("phi", "phi"),
                      ("bPhi", "bphi")):
        put(name, M[key])
    put("k", S0["k"]); put("bk", S0["bk"])
    for stage in range(M["steps"] + 1):
        F = S.channel_flow(M, stage - 1)
        for c in range(3):
            put(f"s{stage}_U{c}", F["U"][c]); put(f"s{stage}_bU{c}", F["bU"][c])
            for k in range(3):
                put(f"s{stage}_gradU{c}_{k}", F["grad"][3 * c + k]); put(f"s{stage}_bGradU{c}_{k}", F["bgrad"][3 * c + k])
    app = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "lesChannel")
    run = subprocess.run([app, d], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    names = dict(k="k", bk="bk", nusgs="nuSgs", bnusgs="bnuSgs")
    for step, want in enumerate(states):
        for key, name in names.items():
            got = np.fromfile(os.path.join(d, f"{name}_{step}.bin"), dtype=np.float64)
            _eq(got, want[key], (model, step, key))


# ---- refusals that need no device, and zero cells -----------------------------------------------------------------------------------------------
def test_host_side_refusals_need_no_device(pkg):
    """what the entries refuse before any device call: missing or broken coefficients, a deltaCoeff or thickness that is not finite, a ck / ce
    that is not above zero, a missing context or handle"""
    import ctypes as C
    eng = pkg.engine
    lib = eng.lib()
    null, one = C.c_void_p(0), C.c_int64(1)
    broken = eng.les_coeffs()
    broken.ck = NAN
    good = eng.les_coeffs()
    d = C.c_double
    for call, why in ((lambda: lib.mi_les_smagorinsky(null, one, None, null, None, null, null), "coefficients"),
                      (lambda: lib.mi_les_smagorinsky(null, one, C.byref(broken), null, None, null, null), "above zero"),
                      (lambda: lib.mi_les_smagorinsky(null, one, C.byref(good), null, None, null, null), "bad argument"),
                      (lambda: lib.mi_les_delta_cube_root_vol(null, one, d(NAN), d(0.0), null, null, null), "finite"),
                      (lambda: lib.mi_les_delta_cube_root_vol(null, one, d(1.0), d(float("inf")), null, null, null), "finite"),
                      (lambda: lib.mi_les_delta_cube_root_vol(null, one, d(1.0), d(-0.1), null, null, null), "finite"),
                      (lambda: lib.mi_les_delta_cube_root_vol(null, one, d(1.0), d(0.0), null, null, null), "bad argument"),
                      (lambda: lib.mi_les_k_terms(null, one, d(0.0), null, null, None, null, null, null, d(1e-5), null, null, null), "above zero"),
                      (lambda: lib.mi_les_k_terms(null, one, d(NAN), null, null, None, null, null, null, d(1e-5), null, null, null), "above zero"),
                      (lambda: lib.mi_les_k_terms(null, one, d(1.048), null, null, None, null, null, null, d(1e-5), null, null, null), "bad argument"),
                      (lambda: lib.mi_les_nusgs(null, one, d(-0.094), null, null, null, null), "above zero"),
                      (lambda: lib.mi_les_nusgs(null, one, d(0.094), null, null, null, null), "bad argument"),
                      (lambda: lib.mi_les_dyn_moments(null, one, None, None, None, null, None, null), "bad argument"),
                      (lambda: lib.mi_les_dyn_level1(null, one, C.c_int(1), null, null, None, None, null, None, null, null, None, None, null, null, null), "bad argument"),
                      (lambda: lib.mi_les_dyn_level2(null, one, None, None, null, null), "bad argument"),
                      (lambda: lib.mi_les_dyn_coeffs(null, one, null, null, null, null, null, null), "bad argument"),
                      (lambda: lib.mi_les_dyn_coeffs(null, C.c_int64(-1), null, null, null, null, null, null), "bad argument"),
                      (lambda: lib.mi_les_simple_filter(null, C.c_int(3), null, null, null, None, None, None), "bad argument"),
                      (lambda: lib.mi_les_coeffs_init(d(0.094), d(1.048), None), "bad argument")):
        assert call() != 0
        assert why in lib.mi_last_error().decode(), (why, lib.mi_last_error().decode())


@pytest.mark.gpu
def test_zero_cells_are_ok(pkg):
    """MI_OK and nothing read or written: every cell pass on empty arrays.  The filter's own zero-cell return cannot be reached: mi_addr_create
    refuses an addressing without cells ("n_cells must be positive"), so no mi_average_t without cells exists"""
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    L = _case(pkg, "box")["L"]
    A = eng.Assembly(eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    e, K = E(0), eng.les_coeffs()
    A.les_delta_cube_root_vol(1.0, 0.0, e, e)
    A.les_delta_cube_root_vol(1.0, 0.05, e, e, e)
    A.les_smagorinsky(K, e, [e] * 9, e, e)
    A.les_k_terms(1.048, e, [e] * 9, e, e, 1e-5, e, e, e)
    A.les_nusgs(0.094, e, e, e)
    A.les_dyn_moments([e] * 3, [e] * 9, [e] * 6, e, [e] * 6, e)
    A.les_dyn_level1(1, e, e, [e] * 3, [e] * 6, e, [e] * 6, e, e, [e] * 6, [e] * 6, e, e, e)
    A.les_dyn_level2([e] * 6, [e] * 6, e, e)
    A.les_dyn_coeffs(e, e, e, e, e, e)
