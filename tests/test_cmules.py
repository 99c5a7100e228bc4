"""Semi-implicit MULES (finiteVolume/fvMatrices/solvers/MULES/CMULESTemplates.C): limiterCorr, limitCorr and correct on the device
(mi_mules_begin_corr, mi_mules_limiter_corr, mi_mules_limit_corr, mi_mules_correct), bit for bit against the restatement of
tests/cmules_support.py -- restated from the reference's text, not pinned by a compiled reference."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from assembly_support import (DEGENERATE_MESHES, OTHER_TABLES, ROW_MODES, bits, gpu_env, same, set_face_grid, set_row_blocks, set_row_tables, shape_case,
                              shaped_addressing)
from least_squares_support import all_finite
from reconstruct_support import seeded_rc, skewed_rc
from mules_support import (COUPLED, OTHER, SMALL, WEDGE, Events, boundary_cells, channel, cyclic_pair, face_kinds, make_inputs, pair_inputs, plain_patches,
                           restate_form, restate_limit)
from cmules_support import (SCALAR_RDT, VARIANTS, RestatedOps, channel_walk, given_lambda, literal_corr_bounds, literal_corr_iterate, literal_correct,
                            literal_limit_corr, make_corr_inputs, negative_zero_cell, restate_correct, restate_corr_bounds, restate_limit_corr)

EXPORTS = ("mi_mules_begin_corr", "mi_mules_limiter_corr", "mi_mules_limit_corr", "mi_mules_correct")
WEDGE_PATCH = 4                                                 # of the skewed box's six patches, in the plain form
NAN = float("nan")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    assert "enum { MI_MULES_CORR_LIMITER, MI_MULES_CORR_LIMIT };" in header
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert " T Foam::MULES::limiterCorr(" in syms and " T Foam::MULES::limitCorr(" in syms
    assert syms.count(" T Foam::MULES::correct(") == 2          # correct alone, and limitCorr + correct


def _skewed(pkg, wedge=True):
    return plain_patches(skewed_rc(pkg.synthetic), WEDGE_PATCH if wedge else None)


def _graph(pkg, name="edge_257", seed=400):
    case = shape_case(pkg, name)
    return seeded_rc(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, seed)


def _cols(x):
    return np.array(x, dtype=np.float64)


def _inputs(pkg, L, seed, variant):
    kw, ec = VARIANTS[variant]
    return make_corr_inputs(pkg.synthetic, L, seed, **kw), ec


def _literal_equals_restatement(L, I, ec, form):
    lam = given_lambda(I) if form == "limiter" else None
    R = restate_limit_corr(L, I, 3, ec, lam=lam)
    tl = lambda pair: tuple(a.tolist() for a in pair)
    phiCorr, bphi = tl(I["phiCorr"]), I["phi"][1].tolist()
    work = literal_corr_bounds(L, I, phiCorr, ec)
    for got, want in zip(work, R["work"]):
        assert same(_cols(got), want)
    llam = tl(lam) if lam is not None else ([1.0] * len(phiCorr[0]), [1.0] * len(phiCorr[1]))
    for j in range(3):
        lp, lm, llam = literal_corr_iterate(L, work, bphi, phiCorr, llam)
        wp, wm, wl = R["steps"][j]
        assert same(_cols(lp), wp) and same(_cols(lm), wm) and same(_cols(llam[0]), wl[0]) and same(_cols(llam[1]), wl[1]), j
    whole = literal_limit_corr(L, I, 3, ec, lam=lam)
    assert same(_cols(whole["out"][0]), R["out"][0]) and same(_cols(whole["out"][1]), R["out"][1])
    assert same(_cols(literal_correct(L, I, whole["out"])), restate_correct(L, I, R["out"]))
    assert all_finite(list(R["work"]) + list(R["out"]) + [restate_correct(L, I, R["out"])])


@pytest.mark.parametrize("form", ["limit", "limiter"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_equals_the_literal_loops(pkg, variant, form):
    """the skewed 5 x 4 x 3 box (one wedge patch; and with its coupled patches) and the 257-cell graph"""
    L = _skewed(pkg)
    _literal_equals_restatement(L, *_inputs(pkg, L, 700, variant), form)
    Lc = dict(skewed_rc(pkg.synthetic), wedge=None)
    _literal_equals_restatement(Lc, *_inputs(pkg, Lc, 701, variant), form)
    Lg = plain_patches(_graph(pkg))
    _literal_equals_restatement(Lg, *_inputs(pkg, Lg, 710, variant), form)


def test_the_limited_corrections_telescope_in_exact_arithmetic(pkg):
    """Fractions, no tolerance, no sources: the sum over cells of V*(rho*rDeltaT)*(psi_new - psi) is minus the boundary sum of the limited
    phiCorr -- every internal face is added once and subtracted once; the limiter is really at work on the way"""
    F = Fraction
    L = _skewed(pkg)
    I = make_corr_inputs(pkg.synthetic, L, 700, rho=True)
    R = literal_limit_corr(L, I, 3, 0.0, conv=F)
    new = literal_correct(L, I, R["out"], conv=F)
    fr = lambda a: [F(x) for x in np.asarray(a).tolist()]
    psi, V, rho = fr(I["psi"]), fr(I["V"]), fr(I["rho"])
    rdt = F(I["rdt"])
    assert sum((V[c] * (rho[c] * rdt) * (new[c] - psi[c]) for c in range(L["n"])), F(0)) == -sum(R["out"][1], F(0))
    lam = R["lam"][0]
    assert any(x == 0 for x in lam) and any(x == 1 for x in lam) and any(0 < x < 1 for x in lam)


def test_lambda_zero_leaves_psi_unchanged_in_exact_arithmetic(pkg):
    F = Fraction
    L = _skewed(pkg, wedge=False)
    I = make_corr_inputs(pkg.synthetic, L, 700, rho=True)
    R = literal_limit_corr(L, I, 3, 0.0, conv=F, force_lambda=0.0)
    assert literal_correct(L, I, R["out"], conv=F) == [F(x) for x in I["psi"].tolist()]


BOX_SEEDS = (700, 702, 703)                                     # 700: the seed of the GPU tests on the box with its wedge patch


def test_the_inputs_exercise_the_limiter(pkg):
    """what a GPU comparison on these inputs cannot pass vacuously: asserted on the restatement alone"""
    L = _skewed(pkg)
    nf = L["lo"].shape[0]
    ev = Events(L)
    for seed in BOX_SEEDS:
        I = make_corr_inputs(pkg.synthetic, L, seed)
        R = restate_limit_corr(L, I, 3, 0.0, ev=ev)
        assert all_finite(list(R["work"]) + list(R["out"]) + [x for s in R["steps"] for x in (s[0], s[1], s[2][0], s[2][1])])
        lam = R["lam"][0]
        for count in (np.sum(lam == 1.0), np.sum(lam == 0.0), np.sum((lam > 0.0) & (lam < 1.0))):
            assert count >= 0.1 * nf, (seed, count, nf)
        for j in (1, 2):                                        # iterations 2 and 3 still change a face
            assert np.any(R["steps"][j][2][0] != R["steps"][j - 1][2][0]) or np.any(R["steps"][j][2][1] != R["steps"][j - 1][2][1]), (seed, j)
        corr = I["phiCorr"][0]
        assert np.any((corr == 0.0) & ~np.signbit(corr)) and np.any((corr == 0.0) & np.signbit(corr))
        kind, bphi, blam = face_kinds(L), I["phi"][1], R["lam"][1]
        free = kind == OTHER
        outlet = bphi > SMALL * SMALL
        assert np.any(free & outlet & (blam < 1.0)) and np.any(free & ~outlet) and np.all(blam[free & ~outlet] == 1.0)
        assert np.all(blam[kind == WEDGE] == 0.0) and np.any(kind == WEDGE)
        # explicit MULES' rule, phiBD + phiCorr with phiBD as MULES::limit forms it, decides a face differently: a reused explicit kernel fails
        explicit_outlet = (I["phiBD"][1] + I["phiCorr"][1]) > SMALL * SMALL
        assert np.any(free & (outlet != explicit_outlet)), seed
        X = restate_limit_corr(L, I, 3, 0.0, ev=ev, explicit_rule_bd=I["phiBD"][1])
        assert not same(X["lam"][1], blam), seed
        # the cell whose psiMaxn is -0.0 before the clamp; the clamp's addition makes it +0.0, explicit MULES' clamp would keep -0.0
        c = negative_zero_cell(L)
        seen = ev.per_side(I["psi"][L["up"]], I["psi"][L["lo"]], I["bpsi"])
        hi = ev.fold(np.full(L["n"], 0.0), seen, lambda a, b: np.where(a > b, a, b))
        assert hi[c] == 0.0 and np.signbit(hi[c]) and I["psi"][c] == 0.0 and not np.signbit(I["psi"][c])
    I = make_corr_inputs(pkg.synthetic, L, 700)
    plain, wide = restate_corr_bounds(L, I, I["phiCorr"], 0.0, ev), restate_corr_bounds(L, I, I["phiCorr"], 0.1, ev)
    assert np.any(plain[0] != wide[0]) and np.any(plain[1] != wide[1])       # the extremaCoeff variant moves a bound on each side


def test_the_inputs_tell_the_clamp_and_the_old_value_term_from_explicit_mules(pkg):
    """Two places where a reused piece of explicit MULES would go unnoticed unless the inputs are made for them; asserted on the restatement
    alone, on the very inputs of the GPU cases (the box at seed 700 in its variants, the 13 x 11 x 9 box at 760).
    The clamp: the cell negative_zero_cell sees -0.0 across every face and holds psi = 0.0 itself, so psiMaxn is -0.0 before the clamp; the
    addition `psiMaxn + 0.0` makes it +0.0 and, in every variant without Su, V*(coef*(+0.0) - 0.0) = +0.0 where the explicit clamp, which has
    no addition, would give V*(coef*(-0.0) - 0.0) = -0.0: dropping the addition changes a bit of the transformed psiMaxn of that cell.
    (With Su the subtraction loses the sign; with extremaCoeff > 0 the addition is not of zero.)
    The old-value term: with rho and a scalar rDeltaT of 1.3, (rho*psi)*rDeltaT and explicit MULES' (rho*rDeltaT)*psi round apart"""
    syn = pkg.synthetic
    L = _skewed(pkg)
    case = syn.box_case(13, 11, 9)
    G = plain_patches(seeded_rc(syn, case.n_cells, case.lower_addr, case.upper_addr, 520))
    without_su = [(L, 700, v) for v in ("plain", "lts", "sp")] + [(G, 760, "plain")]
    for mesh, seed, variant in without_su:
        I, ec = _inputs(pkg, mesh, seed, variant)
        assert ec == 0.0 and I["Su"] is None
        c = negative_zero_cell(mesh)
        ev = Events(mesh)
        real = restate_corr_bounds(mesh, I, I["phiCorr"], 0.0, ev)
        dropped = restate_corr_bounds(mesh, I, I["phiCorr"], 0.0, ev, explicit_clamp=True)
        assert real[0][c] == 0.0 and not np.signbit(real[0][c]) and np.signbit(dropped[0][c]), (seed, variant)
        assert bits(real[0])[c] != bits(dropped[0])[c]
        for k in (1, 2, 3):
            assert same(real[k], dropped[k])
    for variant in ("rho_sp_su", "lts_rho_su"):
        I, ec = _inputs(pkg, L, 700, variant)
        assert isinstance(I["rdt"], np.ndarray) or I["rdt"] == SCALAR_RDT != 1.0
        real = restate_corr_bounds(L, I, I["phiCorr"], ec)
        regrouped = restate_corr_bounds(L, I, I["phiCorr"], ec, explicit_old=True)
        assert not same(real[0], regrouped[0]) and not same(real[1], regrouped[1]), variant


def test_channel_compression_sharpens_and_stays_bounded():
    """24 x 1 x 1, Courant number 0.4, a step of alpha advanced 30 time steps by the statements of alphaEqn.H: MULESCorr yes, nAlphaCorr 2 (so the
    0.5*alpha1 + 0.5*alpha10 branch runs), cAlpha 1, central div(phi,alpha), the implicit upwind predictor by forward substitution.  alpha stays
    in [0, 1] to within rounding: the largest excursion measured on the restatement is 0.0 on either side, so the bar is the floor, 4 ulp
    of 1 = 8.882e-16.  After 30 steps 10 cells lie in (0.01, 0.99); the upwind predictor alone leaves 17"""
    L = channel()
    walk = np.array(channel_walk(RestatedOps(L), 30))
    upwind = np.array(channel_walk(RestatedOps(L), 30, compress=False))
    excursion = max(0.0, float(-walk.min()), float(walk.max() - 1.0))
    smeared = lambda a: int(np.sum((a > 0.01) & (a < 0.99)))
    print("largest excursion", excursion, "cells in (0.01, 0.99):", smeared(walk[-1]), "upwind alone:", smeared(upwind[-1]))
    tol = max(4 * 0.0, 4 * 2.220446049250313e-16)               # 4 x the measured excursion, with a floor of 4 ulp of 1
    assert excursion <= tol
    assert smeared(walk[-1]) < smeared(upwind[-1])
    assert walk[-1].max() > 0.9                                 # the step is still there


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
class Device:
    """one mesh under one addressing on the device: the boundary (or none), the handle, an Assembly"""

    def __init__(self, env, L, addr, boundary=True):
        self.eng, self.ctx, self.dev, self.host, self.E = env
        eng = self.eng
        self.L, self.addr = L, addr
        self.nf, self.nb = L["lo"].shape[0], boundary_cells(L).shape[0]
        self.A = eng.Assembly(addr)
        self.B = eng.GradBoundary(addr, L["fcs"], L["kinds"]) if boundary else None
        self.mu = eng.Mules(addr, self.B, L.get("wedge"))

    def fields(self, I, explicit=False):
        """the corr calls get no psi_old and no rho_old"""
        d = lambda a: None if a is None else self.dev(a)
        return self.eng.mules_fields(d(I["V"]), d(I["psi"]), d(I["psi0"]) if explicit else None,
                                     r_delta_t=d(I["rdt"]) if isinstance(I["rdt"], np.ndarray) else I["rdt"],
                                     b_psi=d(I["bpsi"]) if self.B is not None else None, psi_max=I["psiMax"], psi_min=I["psiMin"], rho=d(I["rho"]),
                                     rho_old=d(I["rho0"]) if explicit else None, sp=d(I["Sp"]), su=d(I["Su"]))

    def flux(self, I, lam=None):
        """phi_corr, b_phi and lambda (given, or NaN to be written); the internal phi is not given: no corr call reads it"""
        E, dev, b = self.E, self.dev, self.B is not None
        pair = lambda p: (dev(p[0]), dev(p[1]) if b else None)
        t = dict(phi_corr=pair(I["phiCorr"]), lambda_=pair(lam) if lam is not None else (E(self.nf), E(self.nb) if b else None))
        arrays = {k: v[0] for k, v in t.items()}
        arrays.update({"b_" + k: v[1] for k, v in t.items()})
        arrays["b_phi"] = dev(I["phi"][1]) if b else None
        self.arrays = arrays
        return t, self.eng.mules_flux(**arrays)

    def in_place(self):
        return self.eng.mules_flux(**dict(self.arrays, out=self.arrays["phi_corr"], b_out=self.arrays["b_phi_corr"]))

    def work(self):
        out = [self.E(self.L["n"]) for _ in range(6)]
        self.mu.work(out)
        return [self.host(x) for x in out]

    def pair(self, p):
        return self.host(p[0]), (self.host(p[1]) if p[1] is not None else np.zeros(0))

    def correct(self, f, I, flux):
        psi = self.dev(I["psi"])
        self.A.mules_correct(self.mu, f, flux[0], psi, b_phi_corr=flux[1])
        return self.host(psi)

    def close(self):
        self.mu.close()
        if self.B is not None:
            self.B.close()


def _addressings(eng, ctx, L):
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


def _staged(D, I, ec, R, tag, form="limit", lam=None, sync=None):
    """begin_corr, three times iterate(1), the in-place apply and correct, every stage's outputs against the restatement R"""
    f = D.fields(I)
    t, x = D.flux(I, lam)
    D.A.mules_begin_corr(D.mu, form, f, x, ec)
    w = D.work()
    for k in range(4):
        _eq(w[k], R["work"][k], (tag, "work", k))
    got = D.pair(t["lambda_"])
    start = lam if lam is not None else (np.ones(D.nf), np.ones(D.nb))
    _eq(got[0], start[0], (tag, "lambda after begin")); _eq(got[1], start[1], (tag, "blambda after begin"))
    for j in range(3):
        D.A.mules_iterate(D.mu, 1, f, x)
        if sync is not None:
            sync(t["lambda_"][1])
        w = D.work()
        lp, lm, (l, bl) = R["steps"][j]
        _eq(w[4], lp, (tag, "lambdap", j)); _eq(w[5], lm, (tag, "lambdam", j))
        got = D.pair(t["lambda_"])
        _eq(got[0], l, (tag, "lambda", j)); _eq(got[1], bl, (tag, "blambda", j))
    D.A.mules_apply(D.mu, True, f, D.in_place())
    out = D.pair(t["phi_corr"])
    _eq(out[0], R["out"][0], (tag, "out")); _eq(out[1], R["out"][1], (tag, "bout"))
    psi = D.correct(f, I, t["phi_corr"])
    _eq(psi, restate_correct(D.L, I, R["out"]), (tag, "correct"))
    return out, psi


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_stage_on_the_skewed_box(pkg, variant):
    """the four work arrays (and lambda) after begin_corr, lambdap / lambdam / lambda after each of three iterations, the in-place product and
    the corrected psi: both forms, one wedge patch, in the caller's numbering and under ordered addressing; the conveniences give the bits
    of the staged calls"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    L = _skewed(pkg)
    I, ec = _inputs(pkg, L, 700, variant)
    ev = Events(L)
    lam = given_lambda(I)
    refs = {"limit": restate_limit_corr(L, I, 3, ec, ev=ev), "limiter": restate_limit_corr(L, I, 3, ec, lam=lam, ev=ev)}
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        for form, R in refs.items():
            given = lam if form == "limiter" else None
            out, _ = _staged(D, I, ec, R, (variant, tag, form), form, given)
            f = D.fields(I)
            t, x = D.flux(I, given)
            if form == "limit":
                D.A.mules_limit_corr(D.mu, f, x, 3, ec)
                got = D.pair(t["phi_corr"])
                assert same(got[0], out[0]) and same(got[1], out[1]), (variant, tag, form)
                got = D.pair(t["lambda_"])
            else:
                D.A.mules_limiter_corr(D.mu, f, x, 3, ec)
                got = D.pair(t["lambda_"])
                assert same(D.pair(t["phi_corr"])[0], I["phiCorr"][0])      # limiterCorr leaves phiCorr alone
            assert same(got[0], R["lam"][0]) and same(got[1], R["lam"][1]), (variant, tag, form)
        D.close()


@pytest.mark.gpu
def test_coupled_patches_staged_on_the_skewed_box(pkg):
    """the box with its two coupled patches as they are (no partner: no sync), staged one iteration at a time"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    L = dict(skewed_rc(pkg.synthetic), wedge=None)
    assert COUPLED in face_kinds(L)
    I = make_corr_inputs(pkg.synthetic, L, 701, rho=True, sp=True, su=True)
    R = restate_limit_corr(L, I, 3, 0.0)
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _staged(D, I, 0.0, R, ("coupled", tag))
        D.close()


@pytest.mark.gpu
def test_cyclic_pair_on_one_rank(pkg):
    """begin_corr, then three times iterate(1) followed by mi_vec_min over the two patch slices, against the restatement with syncFaceList
    restated; iterate(n > 1) and the conveniences are refused on a boundary with coupled patches, and launch nothing"""
    import torch
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    L, sl, _ = cyclic_pair(skewed_rc(pkg.synthetic))
    I = pair_inputs(L, make_corr_inputs(pkg.synthetic, L, 702), sl)
    bd, corr, _ = restate_form(L, I)                            # the correction flux of the paired inputs
    I = dict(I, phiBD=bd, phiCorr=corr)
    R = restate_limit_corr(L, I, 3, 0.0, pairs=[sl])
    assert not same(R["lam"][1], restate_limit_corr(L, I, 3, 0.0)["lam"][1])    # the sync changes something
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))

    def sync(bl):
        a, b = bl[sl[0]], bl[sl[1]]
        other = torch.empty_like(a)
        D.A.vec_min(b, a, other)                                # minOp(mine, theirs) for side b
        D.A.vec_min(a, b, a)
        b.copy_(other)

    _staged(D, I, 0.0, R, "cyclic", sync=sync)
    f = D.fields(I)
    t, x = D.flux(I)
    D.A.mules_begin_corr(D.mu, "limit", f, x)
    before = [y.clone() for p in t.values() for y in p]
    for call in (lambda: D.A.mules_iterate(D.mu, 2, f, x), lambda: D.A.mules_limit_corr(D.mu, f, x, 3), lambda: D.A.mules_limiter_corr(D.mu, f, x, 3),
                 lambda: D.A.mules_limit_corr(D.mu, f, x, 1)):
        with pytest.raises(eng.MiError, match="coupled patches"):
            call()
    torch.cuda.synchronize()
    assert all(same(host(a), host(b)) for a, b in zip(before, [y for p in t.values() for y in p]))
    D.close()


def _limit_and_correct(D, I, ec=0.0):
    f = D.fields(I)
    t, x = D.flux(I)
    D.A.mules_limit_corr(D.mu, f, x, 3, ec)
    return D.pair(t["phi_corr"]), D.pair(t["lambda_"]), D.work(), D.correct(f, I, t["phi_corr"])


def _check_limit_and_correct(D, I, R, tag, ec=0.0):
    out, lam, w, psi = _limit_and_correct(D, I, ec)
    for k in range(4):
        _eq(w[k], R["work"][k], (tag, "work", k))
    _eq(w[4], R["steps"][-1][0], (tag, "lambdap")); _eq(w[5], R["steps"][-1][1], (tag, "lambdam"))
    for k in range(2):
        _eq(lam[k], R["lam"][k], (tag, "lambda", k)); _eq(out[k], R["out"][k], (tag, "out", k))
    _eq(psi, restate_correct(D.L, I, R["out"]), (tag, "correct"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_degenerate_meshes(pkg, name):
    """cells and meshes without faces, hubs of 3 000 faces, cell counts 255 ... 1025: finite on every cell, and no cell is skipped"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    L = plain_patches(_graph(pkg, name))
    I = make_corr_inputs(pkg.synthetic, L, 730, lts=True, rho=True, su=True)
    R = restate_limit_corr(L, I, 3, 0.0)
    assert all_finite(list(R["work"]) + list(R["steps"][-1][:2]) + list(R["out"]) + [restate_correct(L, I, R["out"])])
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _check_limit_and_correct(D, I, R, (name, tag))
        D.close()


_SHAPE_REFS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("tables, mode", [("default", m) for m in ROW_MODES] + OTHER_TABLES)
def test_every_row_pass_shape(pkg, monkeypatch, tables, mode):
    """gradient-plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, the unstaged fall-back, the 32-bit row tables
    and the plain block mapping: the opening pass of limitCorr and correct equal the restatement, hence each other across the shapes"""
    set_row_tables(monkeypatch, tables)
    set_row_blocks(monkeypatch, mode, grad=True)
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    for name in ("box", "graph"):
        case, addr = shaped_addressing(eng, ctx, syn, shape_case(pkg, name, symmetric=True), mode)
        cache = _SHAPE_REFS.setdefault((name, mode.startswith("tiles")), {})
        if not cache:
            L = plain_patches(seeded_rc(syn, case.n_cells, case.lower_addr, case.upper_addr, 500))
            I = make_corr_inputs(syn, L, 750, rho=True, sp=True)
            cache.update(L=L, I=I, R=restate_limit_corr(L, I, 3, 0.1))
        L = cache["L"]
        assert np.array_equal(L["lo"], case.lower_addr) and np.array_equal(L["up"], case.upper_addr)
        D = Device(env, L, addr)
        _check_limit_and_correct(D, cache["I"], cache["R"], (name, tables, mode), 0.1)
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3, 8, 11])
def test_face_grids(pkg, monkeypatch, blocks):
    """the corr-form lambda pass and the in-place product walking their loops: MI_FACE_GRID at 1, 3, 8 and 11 workgroups on the 13 x 11 x 9
    box, whose face count and boundary face count are no multiples of 256"""
    set_face_grid(monkeypatch, blocks)
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    case = pkg.synthetic.box_case(13, 11, 9)
    L = plain_patches(seeded_rc(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, 520))
    nf, nb = L["lo"].shape[0], boundary_cells(L).shape[0]
    assert nf % 256 and nb % 256 and nf > 256 * 11
    cache = _SHAPE_REFS.setdefault("grid", {})
    if not cache:
        I = make_corr_inputs(pkg.synthetic, L, 760)
        cache.update(I=I, R=restate_limit_corr(L, I, 3, 0.0))
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    _check_limit_and_correct(D, cache["I"], cache["R"], ("grid", blocks))
    D.close()


@pytest.mark.gpu
def test_no_boundary(pkg):
    """boundary NULL on a mesh given no patches"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx = env[0], env[1]
    L = skewed_rc(pkg.synthetic)
    bare = dict(n=L["n"], lo=L["lo"], up=L["up"], fcs=[], kinds=[], wedge=None)
    I = make_corr_inputs(pkg.synthetic, bare, 770, su=True)
    R = restate_limit_corr(bare, I, 3, 0.0)
    D = Device(env, bare, eng.Addressing(ctx, bare["n"], bare["lo"], bare["up"]), boundary=False)
    _check_limit_and_correct(D, I, R, "bare")
    D.close()


@pytest.mark.gpu
def test_a_handle_takes_the_patch_rule_of_its_last_begin(pkg):
    """begin, then begin_corr, then begin again on one handle: one iteration after each decides the other patches by the rule of the begin
    that opened it -- the inputs hold faces the two rules decide differently"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    L = _skewed(pkg)
    I = make_corr_inputs(pkg.synthetic, L, 700)
    ev = Events(L)
    explicit = restate_limit(L, I, 1, False, ev=ev)
    corr = restate_limit_corr(L, I, 1, 0.0, ev=ev)
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    fe, fc = D.fields(I, explicit=True), D.fields(I)

    def run_explicit(tag):
        new = lambda: (E(D.nf), E(D.nb))
        t = dict(phi=(dev(I["phi"][0]), dev(I["phi"][1])), phi_psi=(dev(I["phiPsi"][0]), dev(I["phiPsi"][1])), phi_bd=new(), phi_corr=new(), lambda_=new())
        x = eng.mules_flux(**{k: v[0] for k, v in t.items()}, **{"b_" + k: v[1] for k, v in t.items()})
        D.A.mules_begin(D.mu, "limit", fe, x)
        D.A.mules_iterate(D.mu, 1, fe, x)
        got = D.pair(t["lambda_"])
        _eq(got[0], explicit["lam"][0], (tag, "lambda")); _eq(got[1], explicit["lam"][1], (tag, "blambda"))
        return t

    run_explicit("first begin")
    t, x = D.flux(I)
    D.A.mules_begin_corr(D.mu, "limit", fc, x)
    D.A.mules_iterate(D.mu, 1, fc, x)
    got = D.pair(t["lambda_"])
    _eq(got[0], corr["lam"][0], ("begin_corr", "lambda")); _eq(got[1], corr["lam"][1], ("begin_corr", "blambda"))
    with pytest.raises(eng.MiError, match="return_corr"):
        D.A.mules_apply(D.mu, False, fc, D.in_place())
    t = run_explicit("begin again")
    arrays = {k: v[0] for k, v in t.items()}
    arrays.update({"b_" + k: v[1] for k, v in t.items()})
    with pytest.raises(eng.MiError, match="alias"):              # the in-place product is the corr state's alone
        D.A.mules_apply(D.mu, True, fe, eng.mules_flux(**dict(arrays, out=arrays["phi_corr"], b_out=arrays["b_phi_corr"])))
    D.close()


@pytest.mark.gpu
def test_channel_every_step(pkg):
    """the 30-step channel of the CPU demonstration with the compression flux, limitCorr and correct on the device: alpha of every step
    equals the restatement's"""
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    L = channel()
    want = channel_walk(RestatedOps(L), 30)
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))

    class DeviceOps:
        def compression_flux(self, cdw, phir, alpha1):
            out = E(D.nf)
            D.A.alpha_compression_flux(dev(cdw), dev(phir), dev(alpha1), out)
            return host(out)

        def limit_corr(self, I):
            self.f = D.fields(I)
            self.t, x = D.flux(I)
            D.A.mules_limit_corr(D.mu, self.f, x, 3, 0.0)
            return D.pair(self.t["phi_corr"])

        def correct(self, I, flux):
            return D.correct(self.f, I, self.t["phi_corr"])

    got = channel_walk(DeviceOps(), 30)
    for step in range(30):
        _eq(got[step], want[step], ("channel", step))
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
    I = make_corr_inputs(pkg.synthetic, L, 780, rho=True, sp=True, su=True)
    n, nf, nb = L["n"], L["lo"].shape[0], boundary_cells(L).shape[0]
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    other = eng.Addressing(ctx, n, L["lo"], L["up"])
    D = Device(env, L, addr)
    with pytest.raises(eng.MiError, match="another addressing"):
        eng.Assembly(other).mules_begin_corr(D.mu, "limit", None, None)
    cells = dict(vol=dev(I["V"]), psi=dev(I["psi"]), psi_old=None, b_psi=dev(I["bpsi"]), rho=dev(I["rho"]), rho_old=None, sp=dev(I["Sp"]), su=dev(I["Su"]),
                 r_delta_t=I["rdt"])
    fields = lambda **kw: eng.mules_fields(**dict(cells, **kw))
    f = fields()
    t, x = D.flux(I)
    arrays = dict(D.arrays)
    flux = lambda **kw: eng.mules_flux(**dict(arrays, **kw))
    kept = {k: arrays[k].clone() for k in ("phi_corr", "b_phi_corr", "b_phi")}
    outputs = [arrays["lambda_"], arrays["b_lambda_"]]
    untouched = lambda: (all(bool(torch.all(y == fill)) for y in outputs) and all(bool(torch.equal(arrays[k], v)) for k, v in kept.items()))
    A, mu = D.A, D.mu
    spare_f, spare_b, spare_c = E(nf + 1), E(nb + 1), E(n + 1)
    for call in (lambda: A.mules_iterate(mu, 1, f, x), lambda: A.mules_apply(mu, True, f, D.in_place())):
        with pytest.raises(eng.MiError, match="before mi_mules_begin"):
            call()
    bad = [(fields(vol=None), x, "missing"), (fields(psi=None), x, "missing"), (fields(b_psi=None), x, "boundary has faces"), (None, x, "missing"),
           (f, None, "missing"), (f, flux(phi_corr=None), "missing"), (f, flux(b_phi_corr=None), "boundary has faces"),
           (f, flux(b_phi=None), "neither coupled nor wedge"), (f, flux(b_lambda_=None), "boundary has faces"),
           (fields(su=Misaligned(spare_c)), x, "aligned"), (f, flux(phi_corr=Misaligned(spare_f)), "aligned"), (f, flux(b_phi=Misaligned(spare_b)), "aligned"),
           (f, flux(lambda_=arrays["phi_corr"]), "alias"), (f, flux(b_lambda_=arrays["b_phi"]), "alias"), (fields(r_delta_t=arrays["lambda_"]), x, "alias"),
           (f, flux(lambda_=spare_f[:nf], b_lambda_=spare_f[:nb]), "outputs must differ")]
    for ff, xx, why in bad:
        for call in (lambda: A.mules_begin_corr(mu, "limit", ff, xx), lambda: A.mules_limit_corr(mu, ff, xx, 3)):
            with pytest.raises(eng.MiError, match=why):
                call()
    for form in (2, -1):
        with pytest.raises(eng.MiError, match="form"):
            A.mules_begin_corr(mu, form, f, x)
    for ec in (-0.1, float("inf"), float("nan")):
        for call in (lambda: A.mules_begin_corr(mu, "limit", f, x, ec), lambda: A.mules_limit_corr(mu, f, x, 3, ec),
                     lambda: A.mules_limiter_corr(mu, f, x, 3, ec)):
            with pytest.raises(eng.MiError, match="extrema_coeff"):
                call()
    for call in (lambda: A.mules_limit_corr(mu, f, x, -1), lambda: A.mules_limiter_corr(mu, f, x, -1)):
        with pytest.raises(eng.MiError, match="negative"):
            call()
    psi = dev(I["psi"])
    for args, why in (((f, None, psi), "missing"), ((f, arrays["phi_corr"], None), "missing"), ((f, arrays["phi_corr"], psi, None), "boundary has faces"),
                      ((f, arrays["phi_corr"], cells["vol"]), "alias"), ((f, arrays["phi_corr"], Misaligned(spare_c)), "aligned"),
                      ((fields(vol=None), arrays["phi_corr"], psi), "missing")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_correct(mu, *args[:3], b_phi_corr=args[3] if len(args) > 3 else arrays["b_phi_corr"])
    torch.cuda.synchronize()
    assert untouched() and same(host(psi), I["psi"]) and all(bool(torch.all(y == fill)) for y in (spare_f, spare_b, spare_c))
    assert all(same(host(cells[k]), I[q]) for k, q in (("vol", "V"), ("psi", "psi"), ("b_psi", "bpsi"), ("rho", "rho"), ("su", "Su")))
    # begin_corr, then the refusals of iterate and apply
    A.mules_begin_corr(mu, "limit", f, x)
    with pytest.raises(eng.MiError, match="negative"):
        A.mules_iterate(mu, -1, f, x)
    lam = [arrays["lambda_"].clone(), arrays["b_lambda_"].clone()]
    out, b_out = E(nf), E(nb)
    for xx, why in ((flux(lambda_=None), "missing"), (flux(lambda_=arrays["phi_corr"]), "alias"), (flux(b_phi_corr=None), "boundary has faces"),
                    (flux(b_phi=None), "neither coupled nor wedge")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_iterate(mu, 1, f, xx)
    for rc, xx, why in ((True, flux(out=None, b_out=b_out), "missing"), (True, flux(out=arrays["lambda_"], b_out=b_out), "alias"),
                        (True, flux(out=out, b_out=arrays["b_lambda_"]), "alias"), (True, flux(out=out, b_out=out), "outputs must differ"),
                        (False, flux(out=out, b_out=b_out), "return_corr"), (True, flux(out=Misaligned(spare_f), b_out=b_out), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.mules_apply(mu, rc, f, xx)
    torch.cuda.synchronize()
    assert bool(torch.equal(lam[0], arrays["lambda_"])) and bool(torch.equal(lam[1], arrays["b_lambda_"]))
    assert bool(torch.all(out == fill)) and bool(torch.all(b_out == fill)) and all(bool(torch.equal(arrays[k], v)) for k, v in kept.items())
    A.mules_iterate(mu, 3, f, x)
    A.mules_apply(mu, True, f, flux(out=out, b_out=b_out))     # out of place is legal too, and gives the in-place bits
    A.mules_apply(mu, True, f, D.in_place())
    torch.cuda.synchronize()
    assert bool(torch.equal(out, arrays["phi_corr"])) and bool(torch.equal(b_out, arrays["b_phi_corr"])) and not bool(torch.any(out == fill))
    R = restate_limit_corr(L, I, 3, 0.0)
    assert same(host(out), R["out"][0]) and same(host(b_out), R["out"][1])
    psi = dev(I["psi"])                                         # correct looks at neither psi_dev nor b_psi_dev: both may be NULL
    A.mules_correct(mu, fields(psi=None, b_psi=None), out, psi, b_phi_corr=b_out)
    assert same(host(psi), restate_correct(L, I, R["out"]))
    D.close()
