"""Explicit MULES (finiteVolume/fvMatrices/solvers/MULES/MULESTemplates.C, MULESFunctors.H): the limiter, limit and explicitSolve on the device
(mi_mules_*), bit for bit against the restatement of tests/mules_support.py -- restated, not pinned by a compiled reference."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from assembly_support import (DEGENERATE_MESHES, OTHER_TABLES, ROW_MODES, bits, gpu_env, same, set_face_grid, set_row_blocks, set_row_tables, shape_case,
                              shaped_addressing)
from least_squares_support import all_finite
from reconstruct_support import faceless_cells, seeded_rc, skewed_rc
from mules_support import (COUPLED, OTHER, SMALL, VARIANTS, WEDGE, Events, boundary_cells, channel, channel_inputs, channel_run, channel_step_field, cyclic_pair,
                           face_kinds, literal_bounds, literal_form, literal_integrate, literal_iterate, literal_limit, literal_solve, make_inputs,
                           pair_inputs, plain_patches, restate_form, restate_limit, restate_solve)

EXPORTS = ("mi_mules_create", "mi_mules_destroy", "mi_mules_work", "mi_mules_begin", "mi_mules_iterate", "mi_mules_apply", "mi_mules_limiter",
           "mi_mules_limit", "mi_mules_explicit_solve", "mi_vec_min")
WEDGE_PATCH = 4                                                 # of the skewed box's six patches, in the plain form


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    assert "typedef struct mi_mules_s *mi_mules_t;" in header
    assert "enum { MI_MULES_LIMITER, MI_MULES_LIMIT };" in header
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "Foam::mulesData::mulesData(" in syms and "Foam::mulesData::work(" in syms
    assert " T Foam::MULES::limiter(" in syms and " T Foam::MULES::limit(" in syms
    assert syms.count(" T Foam::MULES::explicitSolve(") == 2                 # the solve alone, and limit + solve


def _skewed(pkg, wedge=True):
    return plain_patches(skewed_rc(pkg.synthetic), WEDGE_PATCH if wedge else None)


def _graph(pkg, name="edge_257", seed=400):
    case = shape_case(pkg, name)
    return seeded_rc(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, seed)


def _cols(x):
    return np.array(x, dtype=np.float64)


def _literal_equals_restatement(L, I, form):
    R = restate_limit(L, I, 3, False) if form == "limit" else None
    if form == "limiter":                                       # the limiter form: phiBD / phiCorr / lambda as given, lambda not all ones
        bd, corr, lam = restate_form(L, I)
        lam = (np.where(np.arange(lam[0].shape[0]) % 5 == 0, 0.5, 1.0), np.where(np.arange(lam[1].shape[0]) % 4 == 0, 0.75, 1.0))
        R = restate_limit(L, I, 3, False, given=(bd, corr, lam))
        tl = lambda pair: tuple(a.tolist() for a in pair)
        phiBD, phiCorr, llam = tl(bd), tl(corr), tl(lam)
    else:
        phiBD, phiCorr, llam = literal_form(L, I)
    for got, want in zip(phiBD + phiCorr, R["phiBD"] + R["phiCorr"]):
        assert same(_cols(got), want)
    work = literal_bounds(L, I, phiBD, phiCorr)
    for got, want in zip(work, R["work"]):
        assert same(_cols(got), want)
    for j in range(3):
        lp, lm, llam = literal_iterate(L, work, phiBD, phiCorr, llam)
        wp, wm, wl = R["steps"][j]
        assert same(_cols(lp), wp) and same(_cols(lm), wm) and same(_cols(llam[0]), wl[0]) and same(_cols(llam[1]), wl[1]), j
    out = R["out"]
    assert same(_cols(literal_solve(L, I, tuple(x.tolist() for x in out))), restate_solve(L, I, out))
    assert all_finite(list(R["work"]) + list(out) + [restate_solve(L, I, out)])


@pytest.mark.parametrize("form", ["limit", "limiter"])
@pytest.mark.parametrize("variant", ["plain", "lts", "rho_sp_su", "lts_rho_su", "sp"])
def test_restatement_equals_the_literal_loops_on_the_box(pkg, variant, form):
    L = _skewed(pkg)
    _literal_equals_restatement(L, make_inputs(pkg.synthetic, L, 700, **VARIANTS[variant]), form)
    Lc = dict(skewed_rc(pkg.synthetic), wedge=None)             # with its coupled patches
    _literal_equals_restatement(Lc, make_inputs(pkg.synthetic, Lc, 701, **VARIANTS[variant]), form)


@pytest.mark.parametrize("form", ["limit", "limiter"])
@pytest.mark.parametrize("variant", ["plain", "lts_rho_su"])
def test_restatement_equals_the_literal_loops_on_a_degenerate_graph(pkg, variant, form):
    L = _graph(pkg, "isolated")
    assert faceless_cells(L).shape[0] > 0
    _literal_equals_restatement(L, make_inputs(pkg.synthetic, L, 710, **VARIANTS[variant]), form)


def test_the_limited_fluxes_telescope_in_exact_arithmetic(pkg):
    """Fractions, no tolerance: surfaceIntegrate of the limited flux summed over all cells is the boundary sum (every internal face is added
    once and subtracted once) -- a sign slip on the losort side breaks it; the limiter is really at work on the way"""
    F = Fraction
    L = _skewed(pkg)
    I = make_inputs(pkg.synthetic, L, 700)
    R = literal_limit(L, I, 3, False, conv=F)
    out, bout = R["out"]
    assert sum(literal_integrate(L, (out, bout), F(0)), F(0)) == sum(bout, F(0))
    lam = R["lam"][0]
    assert any(x == 0 for x in lam) and any(x == 1 for x in lam) and any(0 < x < 1 for x in lam)


def test_lambda_zero_is_the_upwind_update_in_exact_arithmetic(pkg):
    F = Fraction
    L = _skewed(pkg, wedge=False)
    I = make_inputs(pkg.synthetic, L, 700, rho=True, su=True)
    R = literal_limit(L, I, 3, False, conv=F, force_lambda=0.0)
    got = literal_solve(L, I, R["out"], conv=F)
    fr = lambda a: [F(x) for x in np.asarray(a).tolist()]
    psi, bpsi, V, rho, rho0, Su = fr(I["psi"]), fr(I["bpsi"]), fr(I["V"]), fr(I["rho"]), fr(I["rho0"]), fr(I["Su"])
    (phi, bphi) = [fr(x) for x in I["phi"]]
    net = [F(0)] * L["n"]                                       # the upwind flux out of each cell
    for f, (o, u) in enumerate(zip(L["lo"].tolist(), L["up"].tolist())):
        flux = phi[f] * (psi[o] if phi[f] >= 0 else psi[u])
        net[o] += flux; net[u] -= flux
    for i, c in enumerate(boundary_cells(L).tolist()):
        net[c] += bphi[i] * bpsi[i]
    rdt = F(I["rdt"])
    want = [(rho0[c] * psi[c] * rdt + Su[c] - net[c] / V[c]) / (rho[c] * rdt) for c in range(L["n"])]
    assert got == want


def test_the_inputs_exercise_the_limiter(pkg):
    """what a GPU comparison on these inputs cannot pass vacuously: asserted on the restatement alone"""
    L = _skewed(pkg)
    nf = L["lo"].shape[0]
    for seed in (700, 701, 702):                                # the seeds of the GPU tests on the box
        I = make_inputs(pkg.synthetic, L, seed)
        R = restate_limit(L, I, 3, False)
        assert all_finite(list(R["work"]) + list(R["out"]) + [x for s in R["steps"] for x in (s[0], s[1], s[2][0], s[2][1])])
        lam = R["lam"][0]
        for count in (np.sum(lam == 1.0), np.sum(lam == 0.0), np.sum((lam > 0.0) & (lam < 1.0))):
            assert count >= 0.1 * nf, (seed, count, nf)
        for j in (1, 2):                                        # iterations 2 and 3 still change a face
            assert np.any(R["steps"][j][2][0] != R["steps"][j - 1][2][0]) or np.any(R["steps"][j][2][1] != R["steps"][j - 1][2][1]), (seed, j)
        corr = R["phiCorr"][0]
        assert np.any((corr == 0.0) & ~np.signbit(corr)) and np.any((corr == 0.0) & np.signbit(corr))
        kind, (bbd, bcorr) = face_kinds(L), (R["phiBD"][1], R["phiCorr"][1])
        free = kind == OTHER
        outlet = (bbd + bcorr) > SMALL * SMALL
        assert np.any(free & outlet & (R["lam"][1] < 1.0)) and np.any(free & ~outlet) and np.all(R["lam"][1][free & ~outlet] == 1.0)
        assert np.all(R["lam"][1][kind == WEDGE] == 0.0) and np.any(kind == WEDGE)           # the wedge patch
    I = make_inputs(pkg.synthetic, L, 700, **VARIANTS["narrow"])
    ev = Events(L)
    seen = ev.per_side(I["psi"][L["up"]], I["psi"][L["lo"]], I["bpsi"])
    hi = ev.fold(np.full(L["n"], 0.2), seen, np.maximum)
    low = ev.fold(np.full(L["n"], 0.8), seen, np.minimum)
    assert np.any(hi > 0.8) and np.any(low < 0.2)              # clamped on each side


def test_channel_mules_stays_bounded_where_the_unlimited_update_does_not():
    """24 x 1 x 1, psi = 0 at the inlet, an outflow patch, Courant number 0.4, a step advanced 30 time steps with the central flux.  The
    unlimited update leaves [0, 1]; MULES stays within [-tol, 1 + tol].  Only rounding can take MULES out of the bounds: the largest
    excursion measured on the restatement is 0.0 below 0 and 8.882e-16 (4 ulp of 1) above 1; the bar is 4 x that, 3.553e-15"""
    free = np.array(channel_run(30, limited=False))
    assert free.min() < -1e-3 and free.max() > 1.0 + 1e-3
    lim = np.array(channel_run(30, limited=True))
    excursion = max(0.0, float(-lim.min()), float(lim.max() - 1.0))
    print("largest excursion", excursion)
    tol = max(4 * 8.881784197001252e-16, 4 * 2.220446049250313e-16)   # 4 x the measured excursion, with a floor of 4 ulp of 1
    assert excursion <= tol
    assert lim[-1].max() > 0.5                                  # the step is still there


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
class Device:
    """one mesh under one addressing on the device: the boundary (or none), the handle, an Assembly, the inputs and the flux arrays"""

    def __init__(self, env, L, addr, boundary=True):
        self.eng, self.ctx, self.dev, self.host, self.E = env
        eng = self.eng
        self.L, self.addr = L, addr
        self.nf, self.nb = L["lo"].shape[0], boundary_cells(L).shape[0]
        self.A = eng.Assembly(addr)
        self.B = eng.GradBoundary(addr, L["fcs"], L["kinds"]) if boundary else None
        self.mu = eng.Mules(addr, self.B, L.get("wedge"))

    def fields(self, I):
        d = lambda a: None if a is None else self.dev(a)
        return self.eng.mules_fields(d(I["V"]), d(I["psi"]), d(I["psi0"]), r_delta_t=d(I["rdt"]) if isinstance(I["rdt"], np.ndarray) else I["rdt"],
                                     b_psi=d(I["bpsi"]) if self.B is not None else None, psi_max=I["psiMax"], psi_min=I["psiMin"], rho=d(I["rho"]),
                                     rho_old=d(I["rho0"]), sp=d(I["Sp"]), su=d(I["Su"]))

    def flux(self, I, given=None):
        """the flux arrays of one run: the limit form's inputs and empty outputs, or (given) phiBD / phiCorr / lambda as the limiter takes them"""
        E, dev, b = self.E, self.dev, self.B is not None
        pair = lambda p: (dev(p[0]), dev(p[1]) if b else None)
        new = lambda: (E(self.nf), E(self.nb) if b else None)
        t = dict(out=new())
        if given is None:
            t.update(phi=pair(I["phi"]), phi_psi=pair(I["phiPsi"]), phi_bd=new(), phi_corr=new(), lambda_=new())
        else:
            t.update(phi_bd=pair(given[0]), phi_corr=pair(given[1]), lambda_=pair(given[2]))
        return t, self.eng.mules_flux(**{k: v[0] for k, v in t.items()}, **{"b_" + k: v[1] for k, v in t.items()})

    def work(self):
        out = [self.E(self.L["n"]) for _ in range(6)]
        self.mu.work(out)
        return [self.host(x) for x in out]

    def pair(self, p):
        return self.host(p[0]), (self.host(p[1]) if p[1] is not None else np.zeros(0))

    def solve(self, f, flux):
        out = self.E(self.L["n"])
        self.A.mules_explicit_solve(self.mu, f, flux[0], out, b_phi_psi=flux[1])
        return self.host(out)

    def close(self):
        self.mu.close()
        if self.B is not None:
            self.B.close()


def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


def _staged(D, I, R, tag, form="limit", return_corr=False, given=None, sync=None):
    """begin, three times iterate(1), apply and the solve, every stage's outputs against the restatement R"""
    f = D.fields(I)
    t, x = D.flux(I, given)
    D.A.mules_begin(D.mu, form, f, x)
    for k, name in enumerate(("phiBD", "phiCorr")):
        got = D.pair(t[("phi_bd", "phi_corr")[k]])
        _eq(got[0], R[name][0], (tag, name)); _eq(got[1], R[name][1], (tag, "b" + name))
    w = D.work()
    for k in range(4):
        _eq(w[k], R["work"][k], (tag, "work", k))
    for j in range(3):
        D.A.mules_iterate(D.mu, 1, f, x)
        if sync is not None:
            sync(t["lambda_"][1])
        w = D.work()
        lp, lm, (l, bl) = R["steps"][j]
        _eq(w[4], lp, (tag, "lambdap", j)); _eq(w[5], lm, (tag, "lambdam", j))
        got = D.pair(t["lambda_"])
        _eq(got[0], l, (tag, "lambda", j)); _eq(got[1], bl, (tag, "blambda", j))
    D.A.mules_apply(D.mu, return_corr, f, x)
    out = D.pair(t["out"])
    _eq(out[0], R["out"][0], (tag, "out")); _eq(out[1], R["out"][1], (tag, "bout"))
    psi = D.solve(f, t["out"])
    _eq(psi, restate_solve(D.L, I, R["out"]), (tag, "solve"))
    return out, psi


def _given(L, I):
    """the limiter form's arguments: the upwind split of the same inputs, lambda not all ones"""
    bd, corr, lam = restate_form(L, I)
    lam = (np.where(np.arange(lam[0].shape[0]) % 5 == 0, 0.5, 1.0), np.where(np.arange(lam[1].shape[0]) % 4 == 0, 0.75, 1.0))
    return bd, corr, lam


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_stage_on_the_skewed_box(pkg, variant):
    """the four work arrays after begin, lambdap / lambdam / lambda after each of three iterations, the applied flux and the solved psi: both
    begin forms, returnCorr on and off, one wedge patch, in the caller's numbering and under ordered addressing; the conveniences give the
    bits of the staged calls"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    L = _skewed(pkg)
    I = make_inputs(pkg.synthetic, L, 700, **VARIANTS[variant])
    ev = Events(L)
    given = _given(L, I)
    refs = {("limit", rc): restate_limit(L, I, 3, rc, ev=ev) for rc in (False, True)}
    refs.update({("limiter", rc): restate_limit(L, I, 3, rc, given=given, ev=ev) for rc in (False, True)})
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        for (form, rc), R in refs.items():
            out, psi = _staged(D, I, R, (variant, tag, form, rc), form, rc, given if form == "limiter" else None)
            f = D.fields(I)
            t, x = D.flux(I, given if form == "limiter" else None)
            if form == "limit":
                D.A.mules_limit(D.mu, f, x, 3, rc)
                got = D.pair(t["out"])
                assert same(got[0], out[0]) and same(got[1], out[1]), (variant, tag, form, rc)
            else:
                D.A.mules_limiter(D.mu, f, x, 3)
                got = D.pair(t["lambda_"])
                assert same(got[0], R["lam"][0]) and same(got[1], R["lam"][1]), (variant, tag, form, rc)
        D.close()


@pytest.mark.gpu
def test_coupled_patches_staged_on_the_skewed_box(pkg):
    """the box with its two coupled patches as they are (no partner: no sync), staged one iteration at a time: the coupled rule of begin's
    phiBD and of the face pass"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    L = dict(skewed_rc(pkg.synthetic), wedge=None)
    assert COUPLED in face_kinds(L)
    I = make_inputs(pkg.synthetic, L, 701, rho=True, sp=True, su=True)
    R = restate_limit(L, I, 3, False)
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _staged(D, I, R, ("coupled", tag))
        D.close()


@pytest.mark.gpu
def test_cyclic_pair_on_one_rank(pkg):
    """begin, then three times iterate(1) followed by mi_vec_min over the two patch slices, against the restatement with syncFaceList
    restated; iterate(n > 1) and the conveniences are refused on a boundary with coupled patches, and launch nothing"""
    import torch
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx, dev, host, E = env
    L, sl, _ = cyclic_pair(skewed_rc(pkg.synthetic))
    I = pair_inputs(L, make_inputs(pkg.synthetic, L, 702), sl)
    R = restate_limit(L, I, 3, False, pairs=[sl])
    plain = restate_limit(L, I, 3, False)
    assert not same(R["lam"][1], plain["lam"][1])              # the sync changes something
    addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    D = Device(env, L, addr)

    def sync(bl):
        a, b = bl[sl[0]], bl[sl[1]]
        other = E(a.numel())
        D.A.vec_min(b, a, other)                                # minOp(mine, theirs) for side b
        D.A.vec_min(a, b, a)
        b.copy_(other)

    _staged(D, I, R, "cyclic", sync=sync)
    f = D.fields(I)
    t, x = D.flux(I)
    D.A.mules_begin(D.mu, "limit", f, x)
    before = [y.clone() for p in t.values() for y in p]
    for call in (lambda: D.A.mules_iterate(D.mu, 2, f, x), lambda: D.A.mules_limit(D.mu, f, x, 3, False), lambda: D.A.mules_limiter(D.mu, f, x, 3),
                 lambda: D.A.mules_limit(D.mu, f, x, 1, False)):
        with pytest.raises(eng.MiError, match="coupled patches"):
            call()
    torch.cuda.synchronize()
    assert all(bool(torch.equal(a, b)) for a, b in zip(before, [y for p in t.values() for y in p]))
    D.close()


def _limit_and_solve(D, I):
    f = D.fields(I)
    t, x = D.flux(I)
    D.A.mules_limit(D.mu, f, x, 3, False)
    return D.pair(t["out"]), D.pair(t["lambda_"]), D.work(), D.solve(f, t["out"])


def _check_limit_and_solve(D, I, R, tag):
    out, lam, w, psi = _limit_and_solve(D, I)
    for k in range(4):
        _eq(w[k], R["work"][k], (tag, "work", k))
    _eq(w[4], R["steps"][-1][0], (tag, "lambdap")); _eq(w[5], R["steps"][-1][1], (tag, "lambdam"))
    for k in range(2):
        _eq(lam[k], R["lam"][k], (tag, "lambda", k)); _eq(out[k], R["out"][k], (tag, "out", k))
    _eq(psi, restate_solve(D.L, I, R["out"]), (tag, "solve"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_degenerate_meshes(pkg, name):
    """cells and meshes without faces, hubs of 3 000 faces, cell counts 255 ... 1025: the restatement is finite on every cell, the faceless ones
    included (they start from VSMALL), and no cell is skipped"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    L = plain_patches(_graph(pkg, name))
    I = make_inputs(pkg.synthetic, L, 730, lts=True, rho=True, su=True)
    R = restate_limit(L, I, 3, False)
    assert all_finite(list(R["work"]) + list(R["steps"][-1][:2]) + list(R["out"]) + [restate_solve(L, I, R["out"])])
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _check_limit_and_solve(D, I, R, (name, tag))
        D.close()


_SHAPE_REFS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("tables, mode", [("default", m) for m in ROW_MODES] + OTHER_TABLES)
def test_every_row_pass_shape(pkg, monkeypatch, tables, mode):
    """gradient-plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, the unstaged fall-back (MI_ROW_CAP=64), the 32-bit
    row tables and the plain block mapping: limit and the solve equal the restatement, hence each other across the shapes"""
    set_row_tables(monkeypatch, tables)
    set_row_blocks(monkeypatch, mode, grad=True)
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    for name in ("box", "graph"):
        case, addr = shaped_addressing(eng, ctx, syn, shape_case(pkg, name, symmetric=True), mode)
        cache = _SHAPE_REFS.setdefault((name, mode.startswith("tiles")), {})
        if not cache:
            L = plain_patches(seeded_rc(syn, case.n_cells, case.lower_addr, case.upper_addr, 500))
            I = make_inputs(syn, L, 750, rho=True, sp=True)
            cache.update(L=L, I=I, R=restate_limit(L, I, 3, False))
        L = cache["L"]
        assert np.array_equal(L["lo"], case.lower_addr) and np.array_equal(L["up"], case.upper_addr)
        D = Device(env, L, addr)
        _check_limit_and_solve(D, cache["I"], cache["R"], (name, tables, mode))
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3, 8, 11])
def test_face_grids(pkg, monkeypatch, blocks):
    """the two face passes walking their loops: MI_FACE_GRID at 1, 3, 8 and 11 workgroups on a mesh whose face count and boundary face count are no
    multiples of 256"""
    set_face_grid(monkeypatch, blocks)
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    case = pkg.synthetic.box_case(9, 8, 10)
    L = plain_patches(seeded_rc(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, 520))
    nf, nb = L["lo"].shape[0], boundary_cells(L).shape[0]
    assert nf % 256 and nb % 256 and nf > 256 * 3
    cache = _SHAPE_REFS.setdefault("grid", {})
    if not cache:
        I = make_inputs(pkg.synthetic, L, 760)
        cache.update(I=I, R=restate_limit(L, I, 3, False))
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    _check_limit_and_solve(D, cache["I"], cache["R"], ("grid", blocks))
    D.close()


@pytest.mark.gpu
def test_no_boundary(pkg):
    """boundary NULL on a mesh given no patches"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    L = skewed_rc(pkg.synthetic)
    bare = dict(n=L["n"], lo=L["lo"], up=L["up"], fcs=[], kinds=[], wedge=None)
    I = make_inputs(pkg.synthetic, bare, 770, su=True)
    R = restate_limit(bare, I, 3, False)
    D = Device(env, bare, eng.Addressing(ctx, bare["n"], bare["lo"], bare["up"]), boundary=False)
    _check_limit_and_solve(D, I, R, "bare")
    D.close()


@pytest.mark.gpu
def test_channel_every_step(pkg):
    """the 30-step channel of the CPU demonstration: psi of every step equals the restatement's"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    L = channel()
    want = channel_run(30)
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    psi = channel_step_field()
    for step in range(30):
        I = channel_inputs(L, psi)
        psi = _limit_and_solve(D, I)[3]
        _eq(psi, want[step], ("channel", step))
    D.close()


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
    env = gpu_env(pkg, fill=fill)
    eng, ctx, dev, host, E = env
    L = _skewed(pkg)
    I = make_inputs(pkg.synthetic, L, 780, rho=True, sp=True, su=True)
    n, nf, nb = L["n"], L["lo"].shape[0], boundary_cells(L).shape[0]
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    other = eng.Addressing(ctx, n, L["lo"], L["up"])
    D = Device(env, L, addr)
    Bo = eng.GradBoundary(other, L["fcs"], L["kinds"])
    for kw in (dict(addr=other, boundary=D.B), dict(addr=addr, boundary=Bo)):
        with pytest.raises(eng.MiError, match="another addressing"):
            eng.Mules(kw["addr"], kw["boundary"], None)
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.Assembly(other).mules_begin(D.mu, "limit", None, None)
    cells = dict(vol=dev(I["V"]), psi=dev(I["psi"]), psi_old=dev(I["psi0"]), b_psi=dev(I["bpsi"]), rho=dev(I["rho"]), rho_old=dev(I["rho0"]),
                 sp=dev(I["Sp"]), su=dev(I["Su"]))
    fields = lambda **kw: eng.mules_fields(**dict(cells, **kw))
    f = fields()
    t, x = D.flux(I)
    arrays = {k: v[0] for k, v in t.items()}
    arrays.update({"b_" + k: v[1] for k, v in t.items()})
    flux = lambda **kw: eng.mules_flux(**dict(arrays, **kw))
    outputs = [arrays[k] for k in ("phi_bd", "b_phi_bd", "phi_corr", "b_phi_corr", "lambda_", "b_lambda_", "out", "b_out")]
    sentinel = lambda: all(bool(torch.all(y == fill)) for y in outputs)
    A, mu = D.A, D.mu
    spare_f, spare_b, spare_c = E(nf + 1), E(nb + 1), E(n + 1)
    # before begin
    for call in (lambda: A.mules_iterate(mu, 1, f, x), lambda: A.mules_apply(mu, False, f, x)):
        with pytest.raises(eng.MiError, match="before mi_mules_begin"):
            call()
    bad = [(fields(vol=None), x, "missing"), (fields(psi_old=None), x, "missing"), (fields(b_psi=None), x, "boundary has faces"),
           (fields(rho_old=None), x, "rho"), (fields(rho=None), x, "rho"), (None, x, "missing"), (f, None, "missing"),
           (f, flux(phi=None), "missing"), (f, flux(b_phi_psi=None), "boundary has faces"), (f, flux(phi_corr=None), "missing"),
           (f, flux(b_lambda_=None), "boundary has faces"),
           (fields(su=Misaligned(spare_c)), x, "aligned"), (f, flux(phi_psi=Misaligned(spare_f)), "aligned"), (f, flux(b_phi_bd=Misaligned(spare_b)), "aligned"),
           (f, flux(phi_bd=arrays["phi"]), "alias"), (f, flux(phi_corr=arrays["phi_psi"]), "alias"), (f, flux(b_lambda_=arrays["b_phi"]), "alias"),
           (f, flux(lambda_=arrays["phi_bd"]), "outputs must differ"), (fields(r_delta_t=arrays["phi_corr"]), x, "alias")]
    for ff, xx, why in bad:
        for call in (lambda: A.mules_begin(mu, "limit", ff, xx), lambda: A.mules_limit(mu, ff, xx, 3, False)):
            with pytest.raises(eng.MiError, match=why):
                call()
    with pytest.raises(eng.MiError, match="form"):
        A.mules_begin(mu, 2, f, x)
    for call in (lambda: A.mules_limit(mu, f, x, -1, False), lambda: A.mules_limiter(mu, f, x, -1)):
        with pytest.raises(eng.MiError, match="negative"):
            call()
    for xx, why in ((flux(out=None), "missing"), (flux(b_out=None), "boundary has faces"), (flux(out=arrays["phi_corr"]), "alias"),
                    (flux(out=Misaligned(spare_f)), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_limit(mu, f, xx, 3, False)
    psi_out = E(n)
    for args, why in (((f, None, psi_out), "missing"), ((f, arrays["phi_psi"], None), "missing"), ((f, arrays["phi_psi"], psi_out, None), "boundary has faces"),
                      ((f, arrays["phi_psi"], cells["vol"]), "alias"), ((f, arrays["phi_psi"], Misaligned(spare_c)), "aligned"),
                      ((fields(rho=None), arrays["phi_psi"], psi_out), "rho")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_explicit_solve(mu, *args[:3], b_phi_psi=args[3] if len(args) > 3 else arrays["b_phi_psi"])
    torch.cuda.synchronize()
    assert sentinel() and bool(torch.all(psi_out == fill)) and all(bool(torch.all(y == fill)) for y in (spare_f, spare_b, spare_c))
    assert all(same(host(cells[k]), I[q]) for k, q in (("vol", "V"), ("psi", "psi"), ("psi_old", "psi0"), ("b_psi", "bpsi"), ("rho", "rho"), ("su", "Su")))
    assert same(host(arrays["phi"]), I["phi"][0]) and same(host(arrays["b_phi_psi"]), I["phiPsi"][1])
    # begin, then the refusals of iterate and apply
    A.mules_begin(mu, "limit", f, x)
    with pytest.raises(eng.MiError, match="negative"):
        A.mules_iterate(mu, -1, f, x)
    lam = [arrays["lambda_"].clone(), arrays["b_lambda_"].clone()]
    for xx, why in ((flux(lambda_=None), "missing"), (flux(lambda_=arrays["phi_corr"]), "alias"), (flux(b_phi_corr=None), "boundary has faces")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_iterate(mu, 1, f, xx)
    for xx, why in ((flux(out=None), "missing"), (flux(out=arrays["lambda_"]), "alias"), (flux(b_out=arrays["out"]), "outputs must differ")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_apply(mu, False, f, xx)
    torch.cuda.synchronize()
    assert bool(torch.equal(lam[0], arrays["lambda_"])) and bool(torch.equal(lam[1], arrays["b_lambda_"]))
    assert bool(torch.all(arrays["out"] == fill)) and bool(torch.all(arrays["b_out"] == fill))
    A.mules_limit(mu, f, x, 3, False)                           # the valid call after them writes every value
    A.mules_explicit_solve(mu, f, arrays["out"], psi_out, b_phi_psi=arrays["b_out"])
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == fill)) for y in outputs + [psi_out])
    # mi_vec_min
    a, b, o = dev(I["phi"][0]), dev(I["phiPsi"][0]), E(nf)
    for args, why in (((a, None, o), "bad argument"), ((a, b, None), "bad argument"), ((a, Misaligned(spare_f), o), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.vec_min(*args)
    torch.cuda.synchronize()
    assert bool(torch.all(o == fill))
    A.vec_min(a, b, o)
    assert same(host(o), np.where(I["phi"][0] < I["phiPsi"][0], I["phi"][0], I["phiPsi"][0]))
    D.close(); Bo.close()
