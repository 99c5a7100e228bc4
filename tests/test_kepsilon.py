"""The kEpsilon model on the device (kEpsilon.C:132-136, :229-280 with the epsilonWallFunction, nutkWallFunction and kqRWallFunction patches,
bound.C, fvcAverage.C): mi_ke_production, mi_ke_wall_cells, mi_ke_epsilon_terms, mi_ke_k_terms, mi_ke_nut, mi_ke_nut_wall, mi_fvc_average,
mi_bound, mi_min_max and mi_vec_max_value, bit for bit against the restatement of tests/turbulence_support.py."""
import math
import os
import re

import numpy as np
import pytest

from assembly_support import bits, gpu_env, same, set_face_grid
from turbulence_support import (ALL_MESHES, BIG, DEFAULTS, MESHES, POW_LOG_BOUND, SMALL, bound_cell, boundary_cells, coeffs, inputs, literal_average,
                                literal_bound, literal_nut_wall, literal_production, literal_terms, literal_wall_cells, mesh, needs_bound,
                                restate_average, restate_bound, restate_nut_wall, restate_production, restate_terms, restate_wall_cells, rmax_v,
                                wall_mask, wall_tables, y_plus_lam)

EXPORTS = ("mi_ke_coeffs_init", "mi_min_max", "mi_vec_max_value", "mi_average_create", "mi_average_destroy", "mi_fvc_average", "mi_bound",
           "mi_ke_production", "mi_ke_create", "mi_ke_destroy", "mi_ke_wall_cells", "mi_ke_wall_cell_labels", "mi_ke_wall_values",
           "mi_ke_epsilon_terms", "mi_ke_k_terms", "mi_ke_nut", "mi_ke_nut_wall")
NAN = float("nan")
SEED = {"box": 2000, "edge_257": 2040, "isolated": 2080, BIG: 2120}
_CACHE = {}


def _case(pkg, name):
    """the mesh, its inputs and the restated results, computed once and left unchanged"""
    if name not in _CACHE:
        L = mesh(pkg, name)
        I = inputs(pkg.synthetic, L, SEED[name])
        bface = rmax_v(I["bv"], I["lb"])
        R = dict(G=restate_production(I["nut"], I["grad"]), wall=restate_wall_cells(L, I, I["G0"], I["eps0"]),
                 terms=restate_terms(I["K"], I["G0"], I["eps"], I["k"], I["nut"], I["nu"]),
                 terms_f=restate_terms(I["K"], I["G0"], I["eps"], I["k"], I["nut"], I["nu_f"]), nutw=restate_nut_wall(L, I, I["k"]),
                 avg=restate_average(L, I["magSf"], I["bms"], I["ssf"], I["bssf"]), bface=bface,
                 bound=restate_bound(L, I["lb"], I["lam"], I["magSf"], I["bms"], bface, I["v"]))
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
    for word in ("kEpsilon", "nutkWallFunction", "epsilonWallFunction", "kqRWallFunction", "mi_ke_coeffs", "mi_ke_wall"):
        assert word in header, word


def test_coefficients_against_the_host_formulas(pkg):
    K = pkg.engine.ke_coeffs()
    want = coeffs()
    for name, value in want.items():
        assert same(np.array([getattr(K, name)]), np.array([value])), name
    assert tuple(getattr(K, n) for n in ("Cmu", "C1", "C2", "sigmaEps", "kappa", "E")) == DEFAULTS
    assert K.yPlusLam == y_plus_lam(0.41, 9.8) and 11.5 < K.yPlusLam < 11.6
    K2 = pkg.engine.ke_coeffs(0.085, 1.5, 1.9, 1.2, 0.4187, 9.0)
    w2 = coeffs(0.085, 1.5, 1.9, 1.2, 0.4187, 9.0)
    assert all(same(np.array([getattr(K2, n)]), np.array([v])) for n, v in w2.items())
    for bad in (dict(Cmu=0.0), dict(C1=-1.0), dict(C2=NAN), dict(sigmaEps=float("inf")), dict(kappa=0.0), dict(E=-9.8)):
        with pytest.raises(pkg.engine.MiError, match="above zero"):
            pkg.engine.ke_coeffs(**bad)


@pytest.mark.parametrize("name", MESHES)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg, name):
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    assert same(literal_production(I["nut"], I["grad"]), R["G"])
    for nu, key in ((I["nu"], "terms"), (I["nu_f"], "terms_f")):
        assert all(same(a, b) for a, b in zip(literal_terms(I["K"], I["G0"], I["eps"], I["k"], I["nut"], nu), R[key]))
    # the wall cells: from the same pow values the two forms agree bit for bit (math.pow and numpy's power may differ)
    G, eps, beps, bpow = R["wall"]
    wall = wall_mask(L)
    lit = literal_wall_cells(L, I, I["G0"], I["eps0"], p15=bpow)
    assert all(same(a, b) for a, b in zip(lit, R["wall"]))
    W = wall_tables(L)
    faces_per_cell = np.array([len(f) for f in W["faces"]])
    assert {1, 2, 3} <= set(faces_per_cell.tolist()) and set(W["weight"].tolist()) >= {1.0, 0.5, 1.0 / 3.0}
    pid = np.concatenate([np.full(fc.shape[0], i) for i, (fc, _) in enumerate(L["patches"])])
    patches_per_cell = np.array([len(set(pid[f].tolist())) for f in W["faces"]])
    assert np.any(patches_per_cell < faces_per_cell), "a cell with two faces in the same wall patch"
    assert np.any(patches_per_cell >= 2) and (name != "box" or {1, 2, 3} <= set(patches_per_cell.tolist()))
    flags = [w for _, w in L["patches"]]
    assert any(not w and any(flags[:i]) and any(flags[i + 1:]) for i, w in enumerate(flags)), "a non-wall patch between wall patches"
    off_wall = np.setdiff1d(np.arange(L["n"]), W["cells"])
    assert off_wall.size and same(G[off_wall], I["G0"][off_wall]) and same(eps[off_wall], I["eps0"][off_wall])
    assert np.all(np.isnan(beps[~wall])) and np.all(beps[wall] > 0) and np.all(G[W["cells"]] >= 0)
    # nut on the walls: both sides of yPlusLam, exact zeros on the laminar side
    nutw, blog, taken = R["nutw"]
    lnut, llog = literal_nut_wall(L, I, I["k"], lg=blog)
    assert same(lnut, nutw) and same(llog, blog)
    share = taken[wall].mean()
    assert 0.2 <= share <= 0.8, share
    assert np.all(nutw[wall & ~taken] == 0.0) and not np.any(np.signbit(nutw[wall & ~taken])) and np.all(nutw[taken] > 0)
    # average and bound
    assert all(same(a, b) for a, b in zip(literal_average(L, I["magSf"], I["bms"], I["ssf"], I["bssf"]), R["avg"]))
    v, b = I["v"], R["bound"]
    assert same(literal_bound(L, I["lb"], I["lam"], I["magSf"], I["bms"], R["bface"], v), b)
    assert needs_bound(v, I["bv"], I["lb"])
    zero = (v == 0.0)
    assert np.any(zero & np.signbit(v)) and np.any(zero & ~np.signbit(v)) and np.any(v < 0)
    c0, nbrs = bound_cell(L)
    assert np.all(v[nbrs] < 0) and I["lb"] <= b[c0] < 1.0        # every neighbour negative: the average sees max(v, lb) = lb across every internal face
    changed = bits(b) != bits(v)
    assert changed.mean() >= 0.1 and (~changed).mean() >= 0.1, (changed.mean(),)
    assert np.all(b >= I["lb"]) and np.all(np.isfinite(b))
    faceless = (np.bincount(L["lo"], minlength=L["n"]) + np.bincount(L["up"], minlength=L["n"]) + np.bincount(boundary_cells(L), minlength=L["n"])) == 0
    assert np.any(faceless) == (name == "isolated")
    if name == "isolated":                                        # 0/0: NaN*pos is NaN, max(v, NaN) is NaN, max(NaN, lb) is lb -- also where v > lb
        assert np.all(np.isnan(R["avg"][0][faceless])) and np.all(b[faceless] == I["lb"]) and np.any(v[faceless] > I["lb"])


@pytest.mark.parametrize("name", MESHES)
def test_each_stated_rounding_changes_a_compared_bit(pkg, name):
    """the magSqr chain, the accumulation order across patches, the grouping of the wall sums, the products of the average, the interpolate of
    bound and pos(-v) each change a compared bit when altered; (nut*2)*m and nut*(2*m) are EQUAL: doubling is exact"""
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    assert not same(restate_production(I["nut"], I["grad"], contracted=False), R["G"])
    assert same(restate_production(I["nut"], I["grad"], late_double=True), R["G"])
    bpow = R["wall"][3]
    for alt in (dict(reverse_patches=True), dict(regroup=True)):
        other = restate_wall_cells(L, I, I["G0"], I["eps0"], p15=bpow, **alt)
        assert not same(other[1], R["wall"][1]) and not same(other[2], R["wall"][2]), alt
    assert not same(restate_wall_cells(L, I, I["G0"], I["eps0"], p15=bpow, reverse_patches=True)[0], R["wall"][0])
    assert not same(restate_average(L, I["magSf"], I["bms"], I["ssf"], I["bssf"], fused=True)[0], R["avg"][0])
    args = (L, I["lb"], I["lam"], I["magSf"], I["bms"], R["bface"], I["v"])
    for alt in (dict(plain_interpolate=True), dict(strict_pos=True)):
        assert not same(restate_bound(*args, **alt), R["bound"]), alt
    # the product avg*pos(-v) against a selection: visible exactly where the average is not a number
    assert same(restate_bound(*args, select=True), R["bound"]) == (name != "isolated")


def test_mirror_declares_the_model_bound_and_average(pkg):
    """foam/miFoam: the class incompressible::RASModels::kEpsilon with the reference's members, bound(), fvc::average and their mesh object are
    declared and in the library"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    for word in ("class averageData", "bool bound(", "void average(", "namespace incompressible", "namespace RASModels", "class kEpsilon",
                 "nuEff(", "DkEff(", "DepsilonEff(", "divDevReff(", "void correct("):
        assert word in text, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    model = "Foam::incompressible::RASModels::kEpsilon::"
    for name in ("Foam::bound(", "Foam::fvc::average(", "Foam::averageData::averageData(", model + "kEpsilon(", model + "correct(", model + "nuEff(",
                 model + "DkEff(", model + "DepsilonEff(", model + "divDevReff("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name


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


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_cell_passes(pkg, monkeypatch, name, blocks):
    """production, the source terms of both equations, nut, max(x, value) and the min / max reduction; 16-byte aligned arrays (two cells per
    thread) and arrays 8 bytes off (one by one); MI_FACE_GRID at its default and forced to 1 and 3 workgroups"""
    import torch
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, K = L["n"], eng.ke_coeffs()
    for tag, addr in _addressings(eng, ctx, L):
        A = eng.Assembly(addr)
        for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
            G = out(n)
            A.ke_production(put(I["nut"]), [put(g) for g in I["grad"]], G)
            _eq(host(G), R["G"], (name, tag, blocks, "G"))
            for nu, key in ((I["nu"], "terms"), (put(I["nu_f"]), "terms_f")):
                su, sp, de, spk, dk, nt = [out(n) for _ in range(6)]
                g0, eps, k, nut = put(I["G0"]), put(I["eps"]), put(I["k"]), put(I["nut"])
                A.ke_epsilon_terms(K, g0, eps, k, nut, nu, su, sp, de)
                A.ke_k_terms(eps, k, nut, nu, spk, dk)
                A.ke_nut(K.Cmu, k, eps, nt)
                for got, want, what in zip((su, sp, de, spk, dk, nt), R[key], ("su", "sp", "deps", "sp_k", "dk", "nut")):
                    _eq(host(got), want, (name, tag, blocks, key, what))
            v = put(I["v"])
            lo, hi = A.min_max(v)
            assert lo == I["v"].min() and hi == I["v"].max(), (name, tag, blocks)
            m = out(n)
            A.vec_max_value(v, I["lb"], m)
            _eq(host(m), rmax_v(I["v"], I["lb"]), (name, tag, blocks, "max"))
            A.vec_max_value(v, I["lb"], v)                        # in place
            _eq(host(v), rmax_v(I["v"], I["lb"]), (name, tag, blocks, "max in place"))
        assert A.min_max(None) == (math.inf, -math.inf)
        one = dev(np.array([-3.5]))
        assert A.min_max(one) == (-3.5, -3.5)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_average_and_bound(pkg, monkeypatch, name, blocks):
    """against the restatement, and mi_bound against the engine's own unfused sequence: mi_vec_max_value, mi_face_interpolate,
    mi_fvc_average and the cell algebra on the host"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, nf = L["n"], L["lo"].shape[0]
    for tag, addr in _addressings(eng, ctx, L):
        A, B = eng.Assembly(addr), _boundary(eng, addr, L)
        magSf, bms, lam = dev(I["magSf"]), dev(I["bms"]), dev(I["lam"])
        H = eng.Average(addr, B, magSf, bms)
        out = E(n)
        A.fvc_average(H, magSf, dev(I["ssf"]), out, bms, dev(I["bssf"]))
        _eq(host(out), R["avg"][0], (name, tag, blocks, "average"))
        bface = E(I["bv"].shape[0])
        A.vec_max_value(dev(I["bv"]), I["lb"], bface)
        _eq(host(bface), R["bface"], (name, tag, blocks, "boundary values"))
        v = dev(I["v"])
        A.bound(H, I["lb"], lam, magSf, v, bms, bface)
        got = host(v)
        _eq(got, R["bound"], (name, tag, blocks, "bound"))
        m, face, avg = E(n), E(max(nf, 1)), E(n)
        A.vec_max_value(dev(I["v"]), I["lb"], m)
        if nf:
            A.face_interpolate(lam, m, face)
        A.fvc_average(H, magSf, face, avg, bms, bface)
        with np.errstate(all="ignore"):
            t = host(avg) * np.where(-I["v"] >= 0, 1.0, 0.0)
        _eq(got, rmax_v(rmax_v(I["v"], t), I["lb"]), (name, tag, blocks, "unfused sequence"))
        H.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_wall_functions(pkg, monkeypatch, name, blocks):
    """The device's pow and log are not the host's, so: b_pow_out / b_log_out against numpy within 16 units of 2^-52 relative (the OpenCL
    full-profile bound for pow, the looser of the two functions), and everything computed after them -- every sum, G, epsilon, the boundary
    values, nut on the walls and the exact zeros of the laminar branch -- bit for bit when the restatement continues from the device's values"""
    set_face_grid(monkeypatch, blocks)
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, name)
    L, I, R = c["L"], c["I"], c["R"]
    n, K, wall = L["n"], eng.ke_coeffs(), wall_mask(L)
    nb = wall.shape[0]
    W = wall_tables(L)
    assert name != BIG or W["cells"].shape[0] > 256
    for tag, addr in _addressings(eng, ctx, L):
        A, B = eng.Assembly(addr), _boundary(eng, addr, L)
        H = eng.KEpsilon(addr, B, [w for _, w in L["patches"]])
        nw = H.wall_cell_labels().numel()
        assert nw == W["cells"].shape[0]
        labels = E(nw)
        H.wall_values(dev(np.arange(n, dtype=np.float64)), labels)
        _eq(host(labels), W["cells"].astype(np.float64), (name, tag, "labels"))
        G, eps, beps, bpow = dev(I["G0"]), dev(I["eps0"]), E(nb), E(nb)
        k, by, bnuw = dev(I["k"]), dev(I["by"]), dev(I["bnuw"])
        A.ke_wall_cells(H, K, k, [dev(x) for x in I["U"]], [dev(x) for x in I["Uw"]], dev(I["bdc"]), by, bnuw, dev(I["bnutw"]), G, eps, beps, bpow)
        bpow_h = host(bpow)
        assert np.all(bpow_h[~wall] == fill) and np.all(host(beps)[~wall] == fill)
        want = restate_wall_cells(L, I, I["G0"], I["eps0"], p15=np.where(wall, bpow_h, NAN))
        _eq(host(G), want[0], (name, tag, blocks, "G")); _eq(host(eps), want[1], (name, tag, blocks, "epsilon"))
        _eq(host(beps)[wall], want[2][wall], (name, tag, blocks, "b_eps"))
        dpow = np.max(np.abs(bpow_h[wall] / R["wall"][3][wall] - 1.0))
        G2, eps2, beps2 = dev(I["G0"]), dev(I["eps0"]), E(nb)     # without the optional output: the same
        A.ke_wall_cells(H, K, k, [dev(x) for x in I["U"]], [dev(x) for x in I["Uw"]], dev(I["bdc"]), by, bnuw, dev(I["bnutw"]), G2, eps2, beps2)
        _eq(host(G2), want[0], "G alone"); _eq(host(eps2), want[1], "epsilon alone"); _eq(host(beps2)[wall], want[2][wall], "b_eps alone")
        vals = E(nw)
        H.wall_values(eps, vals)
        _eq(host(vals), want[1][W["cells"]], (name, tag, "setValues' values"))
        bnut, blog = E(nb), E(nb)
        A.ke_nut_wall(H, K, k, by, bnuw, bnut, blog)
        blog_h = host(blog)
        nutw, rlog, taken = restate_nut_wall(L, I, I["k"], lg=blog_h)
        assert np.all(blog_h[~taken] == fill) and np.all(host(bnut)[~wall] == fill)
        _eq(host(bnut)[wall], nutw[wall], (name, tag, blocks, "nutw"))
        assert not np.any(np.signbit(host(bnut)[wall & ~taken]))
        dlog = np.max(np.abs(blog_h[taken] / R["nutw"][1][taken] - 1.0))
        bnut2 = E(nb)
        A.ke_nut_wall(H, K, k, by, bnuw, bnut2)
        _eq(host(bnut2)[wall], nutw[wall], "nutw alone")
        print(f"{name} {tag}: largest relative deviation from numpy in units of 2^-52: pow {dpow * 2.0 ** 52:.2f}, log {dlog * 2.0 ** 52:.2f}")
        assert dpow <= POW_LOG_BOUND and dlog <= POW_LOG_BOUND, (dpow * 2.0 ** 52, dlog * 2.0 ** 52)
        H.close(); B.close()


def _channel_walk(pkg, orc, ordered):
    """Three correct() steps (kEpsilon.C:229-280, after the constructor's bound + nut lines :132-136) on a 6 x 5 x 4 channel with a fixed-value
    inlet, a zero-gradient outlet and four walls, driven through the Python binding: every intermediate up to and including the assembled,
    relaxed and value-set matrices of both equations and what the solver is handed equals the restatement bit for bit; each solve is the
    engine's PBiCG and the restatement continues from its solution (and from the device's pow / log values); k, epsilon and nut stay finite
    and positive -> the engine's fields after the constructor's lines and after every step"""
    import torch
    from turbulence_support import channel, patch_coeffs, restate_correct, restate_nut_update
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    M, S = channel(pkg)
    L, n, nf, nb = M["L"], M["n"], M["nf"], M["nb"]
    K, wall = eng.ke_coeffs(), wall_mask(L)
    nu, rdt = M["nu"], 1.0 / M["dt"]
    fcs = [fc for fc, _ in L["patches"]]
    addr = eng.Addressing(ctx, n, M["lo"], M["up"], ordered=ordered)
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, fcs, ["fixesValue" if kd == "inlet" else "other" for kd in M["kinds"]])
    H, AV = eng.KEpsilon(addr, B, [kd == "wall" for kd in M["kinds"]]), None
    patches = [eng.Patch(ctx, n, fc) for fc in fcs]
    cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
    g = {key: dev(M[key]) for key in ("V", "magSf", "dc", "lam", "bms", "bdc", "by", "phi", "bnuw")}
    AV = eng.Average(addr, B, g["magSf"], g["bms"])
    U, Uw, grad = [dev(x) for x in M["U"]], [dev(x) for x in M["Uw"]], [dev(x) for x in M["grad"]]
    inlet = torch.from_numpy(M["kind_of"] == "inlet").to("cuda:0")
    mat = eng.Matrix(addr)

    def boundary_of(cell, inlet_value):
        """the boundary values after a solve: patchInternalField per patch, the fixed value on the inlet"""
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

    def nut_update(k, eps, bk, beps):
        nut, bnut, blog = E(n), E(nb), E(nb)
        A.ke_nut(K.Cmu, k, eps, nut)
        A.ke_nut(K.Cmu, bk, beps, bnut)
        A.ke_nut_wall(H, K, k, g["by"], g["bnuw"], bnut, blog)
        return nut, bnut, blog

    def equation(psi_old, psi, su, sp, gamma, bgamma_h, inlet_value, alpha, labels=None):
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

    # the constructor: bound(k), bound(epsilon) (nothing to do on positive fields), nut and its boundary conditions
    k, eps, bk, beps = dev(S["k"]), dev(S["eps"]), dev(S["bk"]), dev(S["beps"])
    assert not bound(k, bk, SMALL) and not bound(eps, beps, SMALL)
    nut, bnut, blog = nut_update(k, eps, bk, beps)
    S["nut"], S["bnut"], taken = restate_nut_update(M, S["k"], S["eps"], S["bk"], S["beps"], host(blog))
    _eq(host(nut), S["nut"], "nut0"); _eq(host(bnut), S["bnut"], "bnut0")
    assert 0.2 <= taken[wall].mean() <= 0.8
    labels = H.wall_cell_labels()
    states = [{key: np.array(S[key]) for key in ("k", "eps", "nut", "bk", "beps", "bnut")}]
    for step in range(M["steps"]):
        D = {}
        G, bpow = E(n), E(nb)
        A.ke_production(nut, grad, G)
        eps_old, k_old = eps.clone(), k.clone()
        A.ke_wall_cells(H, K, k, U, Uw, g["bdc"], g["by"], g["bnuw"], bnut, G, eps, beps, bpow)
        su, sp, de = E(n), E(n), E(n)
        A.ke_epsilon_terms(K, G, eps, k, nut, nu, su, sp, de)
        D.update(G=host(G), eps_wall=host(eps), beps_wall=host(beps), su=host(su), sp=host(sp), deps=host(de))
        bnut_h = host(bnut)
        e = equation(eps_old, eps, su, sp, de, bnut_h / K.sigmaEps + nu, M["eps_in"], M["alpha_eps"], labels)
        D.update({"eps_" + key: v for key, v in e.items()})
        X = dict(bpow=np.where(wall, host(bpow), NAN), eps_solved=host(eps).copy())
        beps = boundary_of(eps, M["eps_in"])
        D["eps_bounded"] = bound(eps, beps, SMALL)
        spk, dk = E(n), E(n)
        A.ke_k_terms(eps, k, nut, nu, spk, dk)
        q = equation(k_old, k, G, spk, dk, bnut_h + nu, M["k_in"], M["alpha_k"])
        D.update({"k_" + key: v for key, v in q.items()})
        D.update(sp_k=host(spk), dk=host(dk), eps_new=host(eps), beps_new=host(beps))
        X["k_solved"] = host(k).copy()
        bk = boundary_of(k, M["k_in"])
        D["k_bounded"] = bound(k, bk, SMALL)
        nut, bnut, blog = nut_update(k, eps, bk, beps)
        D.update(k_new=host(k), bk_new=host(bk), nut=host(nut), bnut=host(bnut))
        X["blog"] = host(blog)
        want, S, taken = restate_correct(orc, M, S, X)
        assert set(want) == set(D)
        for key in sorted(want):
            if isinstance(want[key], bool):
                assert D[key] == want[key], (step, key)
            else:
                _eq(D[key], want[key], (step, key))
        for key in ("k", "eps", "nut", "bk", "beps"):
            assert np.all(np.isfinite(S[key])) and np.all(S[key] > 0), (step, key)
        assert np.all(np.isfinite(S["bnut"])) and np.all(S["bnut"] >= 0)
        print(f"step {step}: k {S['k'].min():.3e}..{S['k'].max():.3e}  epsilon {S['eps'].min():.3e}..{S['eps'].max():.3e}  "
              f"nut {S['nut'].min():.3e}..{S['nut'].max():.3e}  log branch on {taken[wall].mean():.2f} of the wall faces")
        states.append({key: np.array(S[key]) for key in ("k", "eps", "nut", "bk", "beps", "bnut")})
    for h in (AV, H, B):
        h.close()
    return M, states


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["caller", "ordered"])
def test_channel_walk(pkg, orc, ordered):
    """_channel_walk under the caller's numbering and under ordered addressing"""
    _channel_walk(pkg, orc, ordered)


@pytest.mark.gpu
def test_mirror_kepsilon_walks_the_channel(pkg, orc, tmp_path):
    """foam/miFoam's incompressible::RASModels::kEpsilon -- its constructor and three correct() calls, through the driver foam/kEpsilonChannel.C
    in a process of its own, with the solver of the walk (PBiCG, diagonal, 1e-10) -- gives k, epsilon, nut and their boundary values of the
    Python walk bit for bit after the constructor and after every step"""
    import subprocess
    M, states = _channel_walk(pkg, orc, False)
    L = M["L"]
    types = {"inlet": 0, "outlet": 1, "wall": 2}
    d = str(tmp_path)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{M['n']} {M['nf']} {M['steps']} {repr(1.0 / M['dt'])} {repr(M['nu'])} {repr(M['alpha_eps'])} {repr(M['alpha_k'])} {len(M['kinds'])}\n")
        for (fc, _), kd in zip(L["patches"], M["kinds"]):
            f.write(f"{fc.shape[0]} {types[kd]}\n")
    put = lambda name, a, dt=np.float64: np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name + ".bin"))
    put("lower", M["lo"], np.int32); put("upper", M["up"], np.int32); put("faceCells", boundary_cells(L), np.int32)
    for name, key in (("weights", "lam"), ("deltaCoeffs", "dc"), ("magSf", "magSf"), ("V", "V"), ("bMagSf", "bms"), ("bDeltaCoeffs", "bdc"), ("y", "by"),
                      ("phi", "phi"), ("bPhi", "bphi")):
        put(name, M[key])
    for c in range(3):
        put(f"U{c}", M["U"][c]); put(f"bU{c}", M["Uw"][c])
        for k in range(3):
            put(f"gradU{c}_{k}", M["grad"][3 * c + k])
    first = states[0]
    put("k", first["k"]); put("bk", first["bk"]); put("epsilon", first["eps"]); put("bepsilon", first["beps"])
    app = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "kEpsilonChannel")
    run = subprocess.run([app, d], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    names = dict(k="k", eps="epsilon", nut="nut", bk="bk", beps="bepsilon", bnut="bnut")
    for step, want in enumerate(states):
        for key, name in names.items():
            got = np.fromfile(os.path.join(d, f"{name}_{step}.bin"), dtype=np.float64)
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
    L, I = c["L"], c["I"]
    n, nf, K = L["n"], L["lo"].shape[0], eng.ke_coeffs()
    nb = I["bv"].shape[0]
    addr, other = eng.Addressing(ctx, n, L["lo"], L["up"]), eng.Addressing(ctx, n, L["lo"], L["up"])
    A, B = eng.Assembly(addr), _boundary(eng, addr, L)
    bad = Misaligned(E(n + 1))
    nut, grad, k, eps, g0, nu_f = dev(I["nut"]), [dev(g) for g in I["grad"]], dev(I["k"]), dev(I["eps"]), dev(I["G0"]), dev(I["nu_f"])
    o = [E(n) for _ in range(3)]
    for args, why in (((None, grad, o[0]), "missing"), ((nut, grad[:8] + [None], o[0]), "missing"), ((nut, grad, None), "missing"),
                      ((nut, grad, nut), "alias"), ((nut, grad, grad[4]), "alias"), ((bad, grad, o[0]), "aligned"), ((nut, grad, bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.ke_production(*args)
    for args, why in (((K, None, eps, k, nut, 1e-5, *o), "missing"), ((K, g0, eps, k, nut, 1e-5, o[0], o[1], None), "missing"),
                      ((K, g0, eps, k, nut, nu_f, o[0], o[1], nu_f), "alias"), ((K, g0, eps, k, nut, 1e-5, o[0], o[0], o[2]), "differ"),
                      ((K, g0, eps, k, nut, bad, *o), "aligned"), ((None, g0, eps, k, nut, 1e-5, *o), "coefficients")):
        with pytest.raises(eng.MiError, match=why):
            A.ke_epsilon_terms(*args)
    broken = eng.ke_coeffs()
    broken.C2 = NAN
    with pytest.raises(eng.MiError, match="above zero"):
        A.ke_epsilon_terms(broken, g0, eps, k, nut, 1e-5, *o)
    for args, why in (((eps, None, nut, 1e-5, o[0], o[1]), "missing"), ((eps, k, nut, 1e-5, o[0], k), "alias"), ((eps, k, nut, 1e-5, o[0], o[0]), "differ"),
                      ((eps, k, nut, 1e-5, bad, o[1]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.ke_k_terms(*args)
    for args, why in (((0.09, None, eps, o[0]), "missing"), ((0.09, k, eps, eps), "alias"), ((0.0, k, eps, o[0]), "Cmu"), ((NAN, k, eps, o[0]), "Cmu"),
                      ((0.09, k, bad, o[0]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.ke_nut(*args)
    for args, why in (((None, 0.0, o[0]), "missing"), ((k, 0.0, None), "missing"), ((k, 0.0, bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.vec_max_value(*args)
    with pytest.raises(eng.MiError, match="aligned"):
        A.min_max(bad)
    session = eng.Matrix(addr)                                    # a PCG session owns the context's reduction scratch: MI_ERR_STATE
    case = pkg.synthetic.box_case(5, 4, 3)
    sd, su_, psi0, src = dev(case.diag), dev(case.upper), dev(np.zeros(n)), dev(case.source)
    session.set_coeffs(sd, su_, None)
    session.pcg_begin(psi0, src, "diagonal")
    with pytest.raises(eng.MiError, match="PCG session"):
        A.min_max(k)
    session.pcg_end(psi0)
    assert A.min_max(k) == (I["k"].min(), I["k"].max())
    # the average handle and bound
    magSf, bms, lam, ssf, bssf, bface, v = (dev(I[x]) for x in ("magSf", "bms", "lam", "ssf", "bssf", "bv", "v"))
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.Average(other, B, magSf, bms)
    for args, why in (((addr, B, None, bms), "missing"), ((addr, B, magSf, None), "boundary has faces"), ((addr, B, bad, bms), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            eng.Average(*args)
    H = eng.Average(addr, B, magSf, bms)
    for args, why in (((None, ssf, o[0], bms, bssf), "missing"), ((magSf, None, o[0], bms, bssf), "missing"), ((magSf, ssf, o[0], None, bssf), "boundary has faces"),
                      ((magSf, ssf, o[0], bms, None), "boundary has faces"), ((magSf, ssf, None, bms, bssf), "missing"), ((magSf, ssf, bms, bms, bssf), "alias"),
                      ((magSf, ssf, bad, bms, bssf), "aligned"), ((magSf, bad, o[0], bms, bssf), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            H.fvc_average(*args)
    for args, why in (((SMALL, None, magSf, v, bms, bface), "missing"), ((SMALL, lam, None, v, bms, bface), "missing"), ((SMALL, lam, magSf, None, bms, bface), "missing"),
                      ((SMALL, lam, magSf, v, None, bface), "boundary has faces"), ((SMALL, lam, magSf, v, bms, None), "boundary has faces"),
                      ((SMALL, lam, magSf, lam, bms, bface), "alias"), ((SMALL, lam, magSf, bface, bms, bface), "alias"), ((NAN, lam, magSf, v, bms, bface), "lower_bound"),
                      ((SMALL, lam, magSf, bad, bms, bface), "aligned"), ((SMALL, bad, magSf, v, bms, bface), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            H.bound(*args)
    # the wall handle
    flags = [w for _, w in L["patches"]]
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.KEpsilon(other, B, flags)
    with pytest.raises(eng.MiError, match="bad argument"):
        eng.KEpsilon(addr, None, flags)
    Bc = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["coupled"] + ["other"] * (len(flags) - 1))
    with pytest.raises(eng.MiError, match="coupled"):
        eng.KEpsilon(addr, Bc, flags)
    W = eng.KEpsilon(addr, B, flags)
    U, Uw, bdc, by, bnuw, bnutw = [dev(x) for x in I["U"]], [dev(x) for x in I["Uw"]], dev(I["bdc"]), dev(I["by"]), dev(I["bnuw"]), dev(I["bnutw"])
    G, ep, beps, bpow, bnut, blog = E(n), E(n), E(nb), E(nb), E(nb), E(nb)
    good = dict(coeffs=K, k=k, u=U, b_uw=Uw, b_delta_coeffs=bdc, b_y=by, b_nuw=bnuw, b_nutw=bnutw, g_inout=G, eps_inout=ep, b_eps_out=beps, b_pow_out=bpow)
    for kw, why in ((dict(k=None), "missing"), (dict(u=[U[0], None, U[2]]), "missing"), (dict(b_uw=None), "missing"), (dict(b_y=None), "missing"),
                    (dict(g_inout=None), "missing"), (dict(b_eps_out=None), "missing"), (dict(coeffs=None), "coefficients"), (dict(coeffs=broken), "above zero"),
                    (dict(g_inout=k), "alias"), (dict(b_eps_out=by), "alias"), (dict(eps_inout=G), "differ"), (dict(b_pow_out=beps), "differ"),
                    (dict(b_nuw=bad), "aligned"), (dict(eps_inout=bad), "aligned")):
        args = dict(good)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            W.wall_cells(**args)
    for args, why in (((K, None, by, bnuw, bnut, blog), "missing"), ((K, k, None, bnuw, bnut, blog), "missing"), ((K, k, by, bnuw, None, blog), "missing"),
                      ((K, k, by, bnuw, by, blog), "alias"), ((K, k, by, bnuw, bnut, bnut), "differ"), ((K, k, by, bnuw, bad, blog), "aligned"),
                      ((None, k, by, bnuw, bnut, blog), "coefficients"), ((broken, k, by, bnuw, bnut, blog), "above zero")):
        with pytest.raises(eng.MiError, match=why):
            W.nut_wall(*args)
    vals = E(W.wall_cell_labels().numel())
    for args, why in (((None, vals), "missing"), ((ep, None), "missing"), ((ep, ep), "alias"), ((ep, bad), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            W.wall_values(*args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(y == fill)) for y in o + [G, ep, beps, bpow, bnut, blog, vals, bad.t])
    assert same(host(v), I["v"]) and same(host(k), I["k"]) and same(host(magSf), I["magSf"]) and same(host(nu_f), I["nu_f"])
    A.ke_production(nut, grad, o[0])                              # the valid calls after them write every value
    A.ke_epsilon_terms(K, g0, eps, k, nut, 1e-5, *o)
    W.wall_cells(**good)
    W.nut_wall(K, k, by, bnuw, bnut, blog)
    H.bound(SMALL, lam, magSf, v, bms, bface)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == fill)) for y in o)
    wall = torch.from_numpy(wall_mask(L)).to("cuda:0")
    assert not bool(torch.any(beps[wall] == fill)) and not bool(torch.any(bnut[wall] == fill)) and not same(host(v), I["v"])
    # zero wall patches, zero cells: MI_OK and nothing written
    none = eng.KEpsilon(addr, B, [False] * len(flags))
    assert none.wall_cell_labels().numel() == 0
    G0 = E(n)
    none.wall_cells(K, k, U, Uw, bdc, by, bnuw, bnutw, G0, E(n), E(nb))
    none.nut_wall(K, k, by, bnuw, E(nb))
    torch.cuda.synchronize()
    assert bool(torch.all(G0 == fill))
    empty = E(0)
    A.ke_nut(0.09, empty, empty, empty)
    for h in (none, W, H, Bc, B):
        h.close()
