"""Semi-implicit MULES and the interfaceCompression scheme restated (tests/test_cmules.py, tests/test_interface_compression.py): limiterCorr,
limitCorr and correct written out loop by loop, generic over their number type (float, or fractions.Fraction), and the same vectorised; the
interfaceCompression limiter, its weights and alphaEqn.H's compression flux; the inputs the tests run on; the channel walk.

The pin is this restatement, not a compiled reference, taken from the reference's text:
  limiterCorr    CMULESTemplates.C:375-703.  limiterCMULESFunctor / patchMinMaxCMULESFunctor (:160-343): psiMaxn starts at the global psiMin,
                 psiMinn at the global psiMax; max / min over the NEIGHBOUR cells' psi (the cell's own value is not in the loops) and the patches'
                 psiPf; sumPhip / mSumPhim from VSMALL, `phiCorr > 0.0` picks the branch, the losort side with the signs of :246-254; no phiBD.
                 The clamp (:496-497) ADDS extremaCoeff*(psiMax - psiMin) before it takes min / max, also when that is 0.0.  The transform
                 (:503-517) has the old-value term rho*psi*rDeltaT = (rho*psi)*rDeltaT of the CURRENT fields.  The iteration (:522-702) is
                 explicit MULES' but for patchLambdaPfCMULESFunctor (:345-371): a patch that is neither wedge nor coupled limits a face where
                 the boundary value of phi is > SMALL*SMALL.
  limitCorr      :706-758: lambda = 1, limiterCorr, phiCorr *= lambda.
  correct        :35-74: psi = (rho*psi*rDeltaT + Su - surfaceIntegrate(phiCorr))/(rho*rDeltaT - Sp).
  interfaceCompression   interfaceCompression.H:58-77 in PhiScheme.C:52-197; the device-functor rounding of DESIGN 3.5a / 3.5b:
                 1 - 4*x*(1 - x) = fma(-(4*x), 1 - x, 1), sqr a product, weights fma(lim, cdw, (1 - lim)*pos(flux)).
Absent fields, max / min, the order of a cell's faces, meshes and flux pairs: as tests/mules_support.py."""
from fractions import Fraction

import numpy as np

from mules_support import (COUPLED, SMALL, VSMALL, WEDGE, Events, _cell_fields, _cells, _max, _min, _rdt, add, boundary_cells, channel,
                           channel_step_field, face_kinds, literal_integrate, make_inputs, restate_form, rmax, rmin, sync_min)


# ---- literal: loop by loop, generic over the number type --------------------------------------------------------------------------------
def literal_corr_bounds(L, I, phiCorr, extrema=0.0, conv=float):
    """-> psiMaxn, psiMinn (transformed), sumPhip, mSumPhim; phiCorr a pair of lists in the number type"""
    own, nei, bnd = _cells(L)
    lo, up = L["lo"].tolist(), L["up"].tolist()
    rdt, rho, _, Sp, Su, V, psi, _, bpsi = _cell_fields(I, conv)
    gMax, gMin, vsmall = conv(I["psiMax"]), conv(I["psiMin"]), conv(VSMALL)
    ec = conv(extrema) * (gMax - gMin)                         # a scalar of the host
    corr, bcorr = phiCorr
    out = [[], [], [], []]
    for c in range(L["n"]):
        hi, low, sp, sm = gMin, gMax, vsmall, vsmall
        for f in own[c]:
            hi = _max(hi, psi[up[f]]); low = _min(low, psi[up[f]])
            if corr[f] > 0:
                sp = sp + corr[f]
            else:
                sm = sm - corr[f]
        for f in nei[c]:
            hi = _max(hi, psi[lo[f]]); low = _min(low, psi[lo[f]])
            if corr[f] > 0:
                sm = sm + corr[f]
            else:
                sp = sp - corr[f]
        for i in bnd[c]:
            hi = _max(hi, bpsi[i]); low = _min(low, bpsi[i])
            if bcorr[i] > 0:
                sp = sp + bcorr[i]
            else:
                sm = sm - bcorr[i]
        hi = _min(hi + ec, gMax); low = _max(low - ec, gMin)
        coef = rdt[c] if rho is None else rho[c] * rdt[c]
        if Sp is not None:
            coef = coef - Sp[c]
        old = (psi[c] if rho is None else rho[c] * psi[c]) * rdt[c]
        top = coef * hi
        if Su is not None:
            top = top - Su[c]
        top = V[c] * (top - old)
        bot = coef * low
        bot = -bot if Su is None else Su[c] - bot
        bot = V[c] * (bot + old)
        for k, v in enumerate((top, bot, sp, sm)):
            out[k].append(v)
    return out


def literal_corr_iterate(L, work, bphi, phiCorr, lam, conv=float):
    """one limiterCorr iteration -> lambdap, lambdam, (lambda, blambda) new lists; bphi the boundary values of phi"""
    own, nei, bnd = _cells(L)
    lo, up, bc, kind = L["lo"].tolist(), L["up"].tolist(), boundary_cells(L).tolist(), face_kinds(L).tolist()
    maxn, minn, sumPhip, mSumPhim = work
    (corr, bcorr), (l, bl) = phiCorr, lam
    one, small = conv(1.0), conv(SMALL)
    zero = one - one
    lambdap, lambdam = [], []
    for c in range(L["n"]):
        slp, mslm = zero, zero
        for f in own[c]:
            p = l[f] * corr[f]
            if p > 0:
                slp = slp + p
            else:
                mslm = mslm - p
        for f in nei[c]:
            p = l[f] * corr[f]
            if p > 0:
                mslm = mslm + p
            else:
                slp = slp - p
        for i in bnd[c]:
            p = bl[i] * bcorr[i]
            if p > 0:
                slp = slp + p
            else:
                mslm = mslm - p
        lambdam.append(_max(_min((slp + maxn[c]) / (mSumPhim[c] - small), one), zero))
        lambdap.append(_max(_min((mslm + minn[c]) / (sumPhip[c] + small), one), zero))
    nl = [_min(l[f], _min(lambdap[lo[f]], lambdam[up[f]])) if corr[f] > 0 else _min(l[f], _min(lambdam[lo[f]], lambdap[up[f]]))
          for f in range(len(lo))]
    nbl = []
    for i in range(len(bc)):
        v = bl[i]
        if kind[i] == WEDGE:
            v = zero
        elif kind[i] == COUPLED or bphi[i] > small * small:
            v = _min(v, lambdap[bc[i]] if bcorr[i] > 0 else lambdam[bc[i]])
        nbl.append(v)
    return lambdap, lambdam, (nl, nbl)


def literal_correct(L, I, flux, conv=float):
    """MULES::correct: the new psi from the current one"""
    rdt, rho, _, Sp, Su, V, psi, _, _ = _cell_fields(I, conv)
    s = literal_integrate(L, flux, conv(0.0))
    out = []
    for c in range(L["n"]):
        num = (psi[c] if rho is None else rho[c] * psi[c]) * rdt[c]
        if Su is not None:
            num = num + Su[c]
        num = num - s[c] / V[c]
        den = rdt[c] if rho is None else rho[c] * rdt[c]
        if Sp is not None:
            den = den - Sp[c]
        out.append(num / den)
    return out


def literal_limit_corr(L, I, n_iter=3, extrema=0.0, conv=float, lam=None, force_lambda=None):
    """limitCorr (lam None) or limiterCorr with lambda as given, then the product -> dict(work, steps, lam, out)"""
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    phiCorr = tuple(col(a) for a in I["phiCorr"])
    bphi = col(I["phi"][1])
    lam = tuple(col(a) for a in lam) if lam is not None else tuple([conv(1.0)] * len(x) for x in phiCorr)
    work = literal_corr_bounds(L, I, phiCorr, extrema, conv)
    steps = []
    for _ in range(n_iter):
        lp, lm, lam = literal_corr_iterate(L, work, bphi, phiCorr, lam, conv)
        steps.append((lp, lm, lam))
    if force_lambda is not None:
        lam = tuple([conv(force_lambda)] * len(x) for x in lam)
    return dict(work=work, steps=steps, lam=lam, out=tuple([c * l for c, l in zip(cc, ll)] for cc, ll in zip(phiCorr, lam)))


# ---- the same, vectorised ---------------------------------------------------------------------------------------------------------------
def restate_corr_bounds(L, I, phiCorr, extrema=0.0, ev=None, explicit_clamp=False, explicit_old=False):
    """explicit_clamp / explicit_old: what a reused piece of explicit MULES would compute instead -- the clamp without its addition when that
    is 0.0, the old-value term grouped (rho*rDeltaT)*psi; only to show that the inputs tell the two apart"""
    ev = ev or Events(L)
    n, psi = L["n"], I["psi"]
    corr, bcorr = phiCorr
    gMax, gMin = float(I["psiMax"]), float(I["psiMin"])
    ec = float(extrema) * (gMax - gMin)
    seen = ev.per_side(psi[L["up"]], psi[L["lo"]], I["bpsi"])
    hi = ev.fold(np.full(n, gMin), seen, rmax)
    low = ev.fold(np.full(n, gMax), seen, rmin)
    c = ev.per_side(corr, corr, bcorr)
    pos, nbr = c > 0.0, ev.side == 1
    sp = ev.fold(np.full(n, VSMALL), np.where(nbr, -c, c), add, mask=np.where(nbr, ~pos, pos))
    sm = ev.fold(np.full(n, VSMALL), np.where(nbr, c, -c), add, mask=np.where(nbr, pos, ~pos))
    if explicit_clamp and ec == 0.0:
        hi, low = rmin(hi, gMax), rmax(low, gMin)
    else:
        hi, low = rmin(hi + ec, gMax), rmax(low - ec, gMin)
    rdt = _rdt(I, n)
    coef = rdt if I["rho"] is None else I["rho"] * rdt
    if I["Sp"] is not None:
        coef = coef - I["Sp"]
    old = (psi if I["rho"] is None else I["rho"] * psi) * rdt
    if explicit_old:
        old = (rdt if I["rho"] is None else I["rho"] * rdt) * psi
    top = coef * hi
    if I["Su"] is not None:
        top = top - I["Su"]
    top = I["V"] * (top - old)
    bot = coef * low
    bot = -bot if I["Su"] is None else I["Su"] - bot
    bot = I["V"] * (bot + old)
    return [top, bot, sp, sm]


def restate_corr_iterate(L, work, bphi, phiCorr, lam, ev=None, explicit_rule_bd=None):
    """explicit_rule_bd: decide the other patches by explicit MULES' rule with this boundary phiBD instead (what a reused explicit kernel
    would compute; only to show that the inputs tell the two apart)"""
    ev = ev or Events(L)
    n = L["n"]
    maxn, minn, sumPhip, mSumPhim = work
    (corr, bcorr), (l, bl) = phiCorr, lam
    p = ev.per_side(l * corr, l * corr, bl * bcorr)
    pos, nbr = p > 0.0, ev.side == 1
    slp = ev.fold(np.zeros(n), np.where(nbr, -p, p), add, mask=np.where(nbr, ~pos, pos))
    mslm = ev.fold(np.zeros(n), np.where(nbr, p, -p), add, mask=np.where(nbr, pos, ~pos))
    with np.errstate(all="ignore"):
        lambdam = rmax(rmin((slp + maxn) / (mSumPhim - SMALL), 1.0), 0.0)
        lambdap = rmax(rmin((mslm + minn) / (sumPhip + SMALL), 1.0), 0.0)
    lo, up, bc, kind = L["lo"], L["up"], boundary_cells(L), face_kinds(L)
    nl = np.where(corr > 0.0, rmin(l, rmin(lambdap[lo], lambdam[up])), rmin(l, rmin(lambdam[lo], lambdap[up])))
    cut = rmin(bl, np.where(bcorr > 0.0, lambdap[bc], lambdam[bc]))
    outlet = (bphi > SMALL * SMALL) if explicit_rule_bd is None else ((explicit_rule_bd + bcorr) > SMALL * SMALL)
    nbl = np.where(kind == WEDGE, 0.0, np.where((kind == COUPLED) | outlet, cut, bl))
    return lambdap, lambdam, (nl, nbl)


def restate_correct(L, I, flux, ev=None):
    ev = ev or Events(L)
    n = L["n"]
    v, bv = flux
    s = ev.fold(np.zeros(n), ev.per_side(v, -v, bv), add)
    rdt = _rdt(I, n)
    num = (I["psi"] if I["rho"] is None else I["rho"] * I["psi"]) * rdt
    if I["Su"] is not None:
        num = num + I["Su"]
    num = num - s / I["V"]
    den = rdt if I["rho"] is None else I["rho"] * rdt
    if I["Sp"] is not None:
        den = den - I["Sp"]
    return num / den


def restate_limit_corr(L, I, n_iter=3, extrema=0.0, lam=None, pairs=(), ev=None, explicit_rule_bd=None):
    """limitCorr (lam None: lambda = 1) or limiterCorr on the given lambda pair, then phiCorr*lambda
    -> dict(work, steps=[(lambdap, lambdam, (lambda, blambda))], lam, out)"""
    ev = ev or Events(L)
    phiCorr = I["phiCorr"]
    lam = lam if lam is not None else (np.ones(phiCorr[0].shape[0]), np.ones(phiCorr[1].shape[0]))
    work = restate_corr_bounds(L, I, phiCorr, extrema, ev)
    steps = []
    for _ in range(n_iter):
        lp, lm, lam = restate_corr_iterate(L, work, I["phi"][1], phiCorr, lam, ev, explicit_rule_bd)
        lam = (lam[0], sync_min(lam[1], pairs))
        steps.append((lp, lm, lam))
    return dict(work=work, steps=steps, lam=lam, out=(lam[0] * phiCorr[0], lam[1] * phiCorr[1]))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
SCALAR_RDT = 1.3


def negative_zero_cell(L):
    """a cell with at least one neighbour, the middle one if it has"""
    deg = np.bincount(L["lo"], minlength=L["n"]) + np.bincount(L["up"], minlength=L["n"])
    c = L["n"] // 2
    return c if deg[c] > 0 else int(np.argmax(deg))


def make_corr_inputs(syn, L, seed, **kw):
    """mules_support.make_inputs with phiCorr = phiPsi - phiBD, phiBD formed as MULES::limit forms it, so explicit MULES' patch rule
    (phiBD + phiCorr) can be evaluated on the same numbers.  The noise of the high-order flux is large enough that on some boundary faces the
    sign of phiBD + phiCorr is not that of phi.  Every value that one cell (negative_zero_cell) sees across its faces is -0.0: its psiMaxn is
    -0.0 before the clamp, whose addition turns it into +0.0; the cell's own psi is 0.0, so without Su that sign reaches the transformed
    psiMaxn (V*(coef*(+-0.0) - 0.0)).  A scalar rDeltaT is SCALAR_RDT, not 1: (rho*psi)*rDeltaT and (rho*rDeltaT)*psi then round apart"""
    I = make_inputs(syn, L, seed, **kw)
    if not isinstance(I["rdt"], np.ndarray):
        I = dict(I, rdt=SCALAR_RDT)
    if L["lo"].shape[0]:
        c = negative_zero_cell(L)
        psi, bpsi = I["psi"].copy(), I["bpsi"].copy()
        psi[L["up"][L["lo"] == c]] = -0.0
        psi[L["lo"][L["up"] == c]] = -0.0
        bpsi[boundary_cells(L) == c] = -0.0
        psi[c] = 0.0
        I = dict(I, psi=psi, psi0=psi.copy(), bpsi=bpsi)
    bd, corr, _ = restate_form(L, I)
    return dict(I, phiBD=bd, phiCorr=corr)


# name -> (make_inputs keywords, extremaCoeff)
VARIANTS = {
    "plain": (dict(), 0.0),
    "lts": (dict(lts=True), 0.0),
    "rho_sp_su": (dict(rho=True, sp=True, su=True), 0.0),
    "lts_rho_su": (dict(lts=True, rho=True, su=True), 0.0),
    "sp": (dict(sp=True), 0.0),
    "extrema": (dict(), 0.1),
}


def given_lambda(I):
    """the limiter form's lambda: not all ones"""
    nf, nb = I["phiCorr"][0].shape[0], I["phiCorr"][1].shape[0]
    return np.where(np.arange(nf) % 5 == 0, 0.5, 1.0), np.where(np.arange(nb) % 4 == 0, 0.75, 1.0)


# ---- interfaceCompression ------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """one rounding, signed zeros as the hardware gives them: an exactly zero result takes the sign of the rounded a*b + c, which is then
    exact too"""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else a * b + c


def ic_limiter(P, N):
    """interfaceCompression.H:73-76 on two floats"""
    a, b = fma(-(4.0 * P), 1.0 - P, 1.0), fma(-(4.0 * N), 1.0 - N, 1.0)
    return _min(_max(1.0 - _max(a * a, b * b), 0.0), 1.0)


def ic_weight(lim, cdw, flux):
    return fma(lim, cdw, (1.0 - lim) * (1.0 if flux >= 0 else 0.0))


def literal_ic_weights(cdw, flux, aP, aN):
    """face by face -> weights, limiter; aP / aN the two cell values of every face"""
    lim = [ic_limiter(p, q) for p, q in zip(aP.tolist(), aN.tolist())]
    return np.array([ic_weight(l, w, f) for l, w, f in zip(lim, cdw.tolist(), flux.tolist())]), np.array(lim)


def fma_v(a, b, c):
    return np.array([fma(x, y, z) for x, y, z in zip(np.broadcast_to(a, c.shape).tolist(), b.tolist(), c.tolist())]).reshape(c.shape)


def restate_ic_weights(cdw, flux, aP, aN):
    one = np.ones_like(aP)
    a, b = fma_v(-(4.0 * aP), 1.0 - aP, one), fma_v(-(4.0 * aN), 1.0 - aN, one)
    lim = rmin(rmax(1.0 - rmax(a * a, b * b), 0.0), 1.0)
    return fma_v(lim, cdw, (1.0 - lim) * np.where(flux >= 0, 1.0, 0.0)), lim


def interpolate(w, P, N, patch=False):
    """surfaceInterpolationScheme.C:273-279 as mi_face_interpolate fixes it (one fma); a coupled patch :361-366, every operator rounded"""
    return w * P + (1.0 - w) * N if patch else fma_v(w, P - N, N)


def restate_compression_flux_unfused(cdw, phir, a1P, a1N, patch=False):
    """fvc::flux(-fvc::flux(-phir, alpha2, interfaceCompression), alpha1, interfaceCompression) field operation by field operation"""
    a2P, a2N = 1.0 - a1P, 1.0 - a1N                             # the solver's alpha2 = 1.0 - alpha1, gathered
    n = -phir
    w2, _ = restate_ic_weights(cdw, n, a2P, a2N)
    g = n * interpolate(w2, a2P, a2N, patch)
    m = -g
    w1, _ = restate_ic_weights(cdw, m, a1P, a1N)
    return m * interpolate(w1, a1P, a1N, patch)


def literal_compression_flux(cdw, phir, a1P, a1N, patch=False):
    """the same as one expression per face, as the fused kernel writes it"""
    out = []
    for w, ph, P, N in zip(cdw.tolist(), phir.tolist(), a1P.tolist(), a1N.tolist()):
        ip = (lambda wt, p, q: wt * p + (1.0 - wt) * q) if patch else (lambda wt, p, q: fma(wt, p - q, q))
        P2, N2 = 1.0 - P, 1.0 - N
        n = -ph
        m = -(n * ip(ic_weight(ic_limiter(P2, N2), w, n), P2, N2))
        out.append(m * ip(ic_weight(ic_limiter(P, N), w, m), P, N))
    return np.array(out)


def ic_inputs(syn, n, nf, seed):
    """alpha per cell: a fifth exactly 0, a fifth exactly 1, a fifth exactly 0.5, a tenth slightly outside [0, 1] on either side, the rest
    uniform; cdw in (0.3, 0.7); a flux of both signs with exact zeros of both signs"""
    u = syn.splitmix_uniform
    alpha, pick = u(seed, n), u(seed + 1, n)
    alpha[pick < 0.2] = 0.0
    alpha[(pick >= 0.2) & (pick < 0.4)] = 1.0
    alpha[(pick >= 0.4) & (pick < 0.6)] = 0.5
    alpha[(pick >= 0.6) & (pick < 0.65)] = -1e-9 * (1 + u(seed + 2, n)[(pick >= 0.6) & (pick < 0.65)])
    alpha[(pick >= 0.65) & (pick < 0.7)] = 1.0 + 1e-9 * (1 + u(seed + 3, n)[(pick >= 0.65) & (pick < 0.7)])
    flux = u(seed + 4, nf) - 0.5
    flux[::5] = 0.0
    flux[2::7] = -0.0
    return alpha, 0.3 + 0.4 * u(seed + 5, nf), flux


# ---- the channel walk: alphaEqn.H with MULESCorr yes, nAlphaCorr 2, cAlpha 1, central div(phi,alpha) -------------------------------------
class RestatedOps:
    """the three device entries of the walk, restated"""

    def __init__(self, L):
        self.L, self.ev = L, Events(L)

    def compression_flux(self, cdw, phir, alpha1):
        return restate_compression_flux_unfused(cdw, phir, alpha1[self.L["lo"]], alpha1[self.L["up"]])

    def limit_corr(self, I):
        return restate_limit_corr(self.L, I, 3, 0.0, ev=self.ev)["out"]

    def correct(self, I, flux):
        return restate_correct(self.L, I, flux, self.ev)


def channel_fields(psi, phi_pair, corr_pair):
    return dict(psi=psi, psi0=psi, V=np.ones(psi.shape[0]), rdt=1.0, rho=None, rho0=None, Sp=None, Su=None, bpsi=np.array([0.0, psi[-1]]),
                psiMax=1.0, psiMin=0.0, phi=phi_pair, phiCorr=corr_pair)


def upwind_predictor(alpha, courant):
    """fvm::ddt + fvm::div(phi, upwind) on unit cells with rDeltaT = 1, solved by forward substitution (the inlet value is 0); its flux()"""
    new = np.empty_like(alpha)
    prev = 0.0
    for c in range(alpha.shape[0]):
        new[c] = (alpha[c] + courant * prev) / (1.0 + courant)
        prev = new[c]
    return new, (courant * new[:-1], np.array([-courant * 0.0, courant * new[-1]]))


def n_hat_f(alpha):
    """interfaceProperties' nHatf on the unit channel by numpy glue: the Gauss linear cell gradient, interpolated, /(|.| + deltaN), & Sf = +x"""
    face = np.concatenate([[0.0], 0.5 * (alpha[:-1] + alpha[1:]), [alpha[-1]]])
    g = face[1:] - face[:-1]
    gf = 0.5 * (g[:-1] + g[1:])
    return gf / (np.abs(gf) + 1e-8)


def channel_walk(ops, steps=30, nx=24, courant=0.4, compress=True):
    """-> [alpha1 after each time step].  compress False: the upwind predictor alone"""
    L = channel(nx)
    lo, up = L["lo"], L["up"]
    nf = lo.shape[0]
    phi, bphi = np.full(nf, courant), np.array([-courant, courant])
    cdw = np.full(nf, 0.5)
    phic = 1.0 * np.abs(phi / 1.0)                              # cAlpha*mag(phi/magSf); zero on the (non-coupled) patches
    alpha1, out = channel_step_field(nx), []
    for _ in range(steps):
        alpha1, phiAlpha = upwind_predictor(alpha1, courant)
        for a_corr in range(2 if compress else 0):
            phir = phic * n_hat_f(alpha1)
            bpsi = np.array([0.0, alpha1[-1]])
            un = (phi * (0.5 * (alpha1[lo] + alpha1[up])) + ops.compression_flux(cdw, phir, alpha1), bphi * bpsi + 0.0)
            corr = (un[0] - phiAlpha[0], un[1] - phiAlpha[1])
            alpha10 = alpha1
            I = channel_fields(alpha1, un, corr)                # MULES::correct passes phiAlphaUn as phi
            corr = ops.limit_corr(I)
            alpha1 = ops.correct(I, corr)
            if a_corr == 0:
                phiAlpha = (phiAlpha[0] + corr[0], phiAlpha[1] + corr[1])
            else:
                alpha1 = 0.5 * alpha1 + 0.5 * alpha10
                phiAlpha = (phiAlpha[0] + 0.5 * corr[0], phiAlpha[1] + 0.5 * corr[1])
        out.append(alpha1)
    return out
