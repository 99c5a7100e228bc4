"""hePsiThermo / heRhoThermo ::calculate() restated twice (hePsiThermo.C:31-171, heRhoThermo.C:31-177, heThermo.C:131-145, thermoI.H:42-90,
hConstThermoI.H, eConstThermoI.H, janafThermoI.H:58-71, :119-141, :188-241, perfectGasI.H:80-106, constTransportI.H:98-128,
sutherlandTransportI.H:133-164): literal loops over Python floats that follow the reference's statements, and vectorised numpy.
The kernels of csrc/thermo.inc are compared with the vectorised form bit for bit; a CPU test shows that the two forms agree and that the
inputs reach every branch.

Rounding: every operator on its own; fma in janaf's Horner chains of cp, ha and hc, in hs = ha - hc, in janaf's cv = cp - cpMcv where Cv meets it
(not in gamma), and in es = hs - (p*W)/rho for hConst and eConst (the header comment of include/mi_ldu.h lists them).  max(a, b) = (a > b) ? a : b, min(a, b) = (a < b) ? a : b, mag = fabs.  A model here
is the dict host_model() returns: the given numbers and the ones mi_thermo_model_init derives, under the struct's names."""
import itertools
import math

import numpy as np

from interface_support import div, fma, fma_v

RR = 8314.4621
TSTD = 298.15
NAN = float("nan")
ENERGY, THERMO, TRANSPORT = ("h", "e"), ("hConst", "eConst", "janaf"), ("const", "sutherland")
MODELS = tuple(itertools.product(ENERGY, THERMO, TRANSPORT))          # all twelve
FULL_GRID = (("h", "hConst", "sutherland"), ("e", "janaf", "sutherland"))   # the two models that run every launch form
PROPERTIES = ("Cp", "Cv", "gamma", "Cpv", "CpByCpv", "kappa")
# air (the engine's defaults, typed in again so that a changed default shows) and carbon dioxide: one second set of numbers per part
AIR = dict(W=28.9, Cp=1007.0, Cv=719.3, Hf=0.0, mu=1.84e-05, Pr=0.7, As=1.4792e-06, Ts=116.0, Tlow=200.0, Thigh=6000.0, Tcommon=1000.0,
           highCpCoeffs=(3.08792717, 0.00124597184, -4.23718945e-07, 6.74774789e-11, -3.97076972e-15, -995.262755, 5.9596093),
           lowCpCoeffs=(3.5683962, -0.000678729429, 1.55371476e-06, -3.2993706e-12, -4.66395387e-13, -1062.34659, 3.71582965))
CO2 = dict(W=44.01, Cp=846.0, Cv=657.0, Hf=-8941478.5, mu=1.47e-05, Pr=0.76, As=1.572e-06, Ts=240.0, Tlow=250.0, Thigh=5000.0, Tcommon=1100.0,
           highCpCoeffs=(4.45362, 0.00314017, -1.27841e-06, 2.394e-10, -1.66903e-14, -48967.0, -0.955396),
           lowCpCoeffs=(2.27572, 0.00992207, -1.04091e-05, 6.86669e-09, -2.11728e-12, -48373.1, 10.1885))
SETS = {"air": AIR, "co2": CO2}
N_BASE, N_ALL = 257, (0, 1, 2, 257, 1537)


def rmax(a, b):
    return a if a > b else b


def rmin(a, b):
    return a if a < b else b


def same_bits(a, b):
    """bit for bit where both are numbers, NaN exactly where the other has NaN (a NaN's sign and payload are the arithmetic unit's own)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def host_model(energy="h", thermo="hConst", transport="const", numbers=AIR):
    """the literal host formulas of mi_thermo_model_init; members of the parts not chosen are 0"""
    g = dict(numbers)
    W = g["W"]
    M = dict(energy=ENERGY.index(energy), thermo=THERMO.index(thermo), transport=TRANSPORT.index(transport), W=W, R=RR / W, cpMcv=RR,
             Cp=0.0, Cv=0.0, Hf=0.0, CpW=0.0, CvW=0.0, HfW=0.0, cpE=0.0, Tlow=0.0, Thigh=0.0, Tcommon=0.0, highCpCoeffs=(0.0,) * 7,
             lowCpCoeffs=(0.0,) * 7, highH=(0.0,) * 4, lowH=(0.0,) * 4, hc=0.0, mu=0.0, Pr=0.0, rPr=0.0, As=0.0, Ts=0.0)
    if thermo == "hConst":
        M.update(Cp=g["Cp"], Hf=g["Hf"], CpW=g["Cp"] * W, HfW=g["Hf"] * W)
    elif thermo == "eConst":
        M.update(Cv=g["Cv"], Hf=g["Hf"], CvW=g["Cv"] * W, HfW=g["Hf"] * W)
        M["cpE"] = M["CvW"] + RR
    else:
        hi, lo = tuple(g["highCpCoeffs"]), tuple(g["lowCpCoeffs"])
        M.update(Tlow=g["Tlow"], Thigh=g["Thigh"], Tcommon=g["Tcommon"], highCpCoeffs=hi, lowCpCoeffs=lo,
                 highH=(hi[1] / 2.0, hi[2] / 3.0, hi[3] / 4.0, hi[4] / 5.0), lowH=(lo[1] / 2.0, lo[2] / 3.0, lo[3] / 4.0, lo[4] / 5.0))
        a = lo
        M["hc"] = RR * fma(fma(fma(fma(fma(a[4] / 5.0, TSTD, a[3] / 4.0), TSTD, a[2] / 3.0), TSTD, a[1] / 2.0), TSTD, a[0]), TSTD, a[5])
    if transport == "const":
        M.update(mu=g["mu"], Pr=g["Pr"], rPr=1.0 / g["Pr"])
    else:
        M.update(As=g["As"], Ts=g["Ts"])
    return M


def engine_model(eng, energy, thermo, transport, numbers=AIR):
    return eng.thermo_model(energy=energy, thermo=thermo, transport=transport, **numbers)


# ---- literal: one element at a time, the reference's statements -----------------------------------------------------------------------------------
def _coeffs(M, T):
    return M["lowCpCoeffs"] if T < M["Tcommon"] else M["highCpCoeffs"]


def lit_cp(M, T):
    if M["thermo"] == 0:
        return M["CpW"]                                            # hConstThermoI.H:110
    if M["thermo"] == 1:
        return M["CvW"] + M["cpMcv"]                               # eConstThermoI.H:111
    a = _coeffs(M, T)                                              # janafThermoI.H:194-195
    return RR * fma(fma(fma(fma(a[4], T, a[3]), T, a[2]), T, a[1]), T, a[0])


def lit_hc(M):
    a = M["lowCpCoeffs"]                                           # janafThermoI.H:230-241
    return RR * fma(fma(fma(fma(fma(a[4] / 5.0, TSTD, a[3] / 4.0), TSTD, a[2] / 3.0), TSTD, a[1] / 2.0), TSTD, a[0]), TSTD, a[5])


def lit_rho(M, p, T):
    return div(p, (RR / M["W"]) * T)                               # perfectGasI.H:82, specieI.H:97-100


def lit_hs(M, T):
    """hs alone, as the enthalpy form meets it"""
    if M["thermo"] == 2:
        a = _coeffs(M, T)                                          # ha - hc (janafThermoI.H:207-225)
        inner = fma(fma(fma(fma(fma(a[4] / 5.0, T, a[3] / 4.0), T, a[2] / 3.0), T, a[1] / 2.0), T, a[0]), T, a[5])
        return fma(RR, inner, -lit_hc(M))
    return lit_cp(M, T) * T                                        # hConstThermoI.H:132, eConstThermoI.H:135


def lit_es(M, p, T):
    q = div(p * M["W"], lit_rho(M, p, T))                          # thermoI.H:171: hs - p*W/rho
    if M["thermo"] == 2:
        return lit_hs(M, T) - q
    return fma(lit_cp(M, T), T, -q)


def lit_he(M, p, T):
    return div(lit_hs(M, T), M["W"]) if M["energy"] == 0 else div(lit_es(M, p, T), M["W"])


def lit_cv(M, T):
    """cv = cp - cpMcv (thermoI.H:128-131) as Cv meets it: janaf's product 8314.4621*chain has this one use and contracts with the subtraction"""
    if M["thermo"] == 2:
        a = _coeffs(M, T)
        return fma(RR, fma(fma(fma(fma(a[4], T, a[3]), T, a[2]), T, a[1]), T, a[0]), -M["cpMcv"])
    return lit_cp(M, T) - M["cpMcv"]


def lit_cpv(M, T, energy=None):
    e = M["energy"] if energy is None else energy
    return div(lit_cp(M, T), M["W"]) if e == 0 else div(lit_cv(M, T), M["W"])


def lit_limit(M, T):
    if M["thermo"] == 2 and (T < M["Tlow"] or T > M["Thigh"]):     # janafThermoI.H:124-135
        return rmin(rmax(T, M["Tlow"]), M["Thigh"])
    return T


def lit_the(M, f, p, T0):
    """thermo::T (thermoI.H:42-90) -> (T, evaluations, the iterates)"""
    Test, Tnew, Ttol, it, path = T0, T0, T0 * 1.0e-4, 0, [T0]
    while True:
        Test = Tnew
        Tnew = lit_limit(M, Test - div(lit_he(M, p, Test) - f, lit_cpv(M, Test)))
        path.append(Tnew)
        it += 1
        if it - 1 > 100:
            return NAN, it, path
        if not (abs(Tnew - Test) > Ttol):
            return Tnew, it, path


def lit_sqrt(x):
    return math.sqrt(x) if x >= 0 else NAN


def lit_mu(M, T):
    return M["mu"] if M["transport"] == 0 else div(M["As"] * lit_sqrt(T), 1.0 + div(M["Ts"], T))


def lit_kappa(M, T):
    if M["transport"] == 0:
        return (lit_cpv(M, T) * M["mu"]) * M["rPr"]                # constTransportI.H:116
    Cv_ = lit_cpv(M, T, 1)                                         # sutherlandTransportI.H:150-151
    return (lit_mu(M, T) * Cv_) * (1.32 + div(1.77 * (RR / M["W"]), Cv_))


def lit_alphah(M, T):
    return M["mu"] * M["rPr"] if M["transport"] == 0 else div(lit_kappa(M, T), lit_cpv(M, T))


def lit_props(M, p, T, rho_form):
    psi = div(1.0, (RR / M["W"]) * T)
    rho = NAN if rho_form == 0 else lit_rho(M, p, T) if rho_form == 1 else psi * p
    return psi, lit_mu(M, T), lit_alphah(M, T), rho


def literal_calculate(M, he, p, t0, rho_form=0):
    n = he.shape[0]
    out = [np.full(n, NAN) for _ in range(5)]
    iters = np.zeros(n, dtype=np.int32)
    for i in range(n):
        T, iters[i], _ = lit_the(M, float(he[i]), float(p[i]), float(t0[i]))
        out[0][i] = T
        out[1][i], out[2][i], out[3][i], out[4][i] = lit_props(M, float(p[i]), T, rho_form)
    return dict(T=out[0], psi=out[1], mu=out[2], alpha=out[3], rho=out[4], iters=iters)


def literal_property(M, kind, p, T):
    out = np.empty(T.shape[0])
    for i, t in enumerate(T.tolist()):
        cp = lit_cp(M, t)
        gamma = div(cp, cp - M["cpMcv"])
        out[i] = {"Cp": lit_cpv(M, t, 0), "Cv": lit_cpv(M, t, 1), "gamma": gamma, "Cpv": lit_cpv(M, t),
                  "CpByCpv": 1.0 if M["energy"] == 0 else gamma, "kappa": lit_kappa(M, t)}[kind]
    return out


def literal_boundary(M, kinds, sizes, B, rho_form=0, t_into_he=False):
    """the patch loop of hePsiThermo.C:109-171 face by face on copies of B's arrays"""
    R = {k: B[k].copy() for k in ("he", "p", "T", "psi", "mu", "alpha", "rho")}
    off = 0
    for kind, size in zip(kinds, sizes):
        for f in range(off, off + size):
            p = float(R["p"][f])
            if kind == 1:
                T = float(R["T"][f])
                R["he"][f] = lit_he(M, p, T)
            elif kind == 2:
                T = lit_the(M, float(R["he"][f]), p, float(R["T"][f]))[0]
                R["he" if t_into_he else "T"][f] = T
            else:
                continue
            R["psi"][f], R["mu"][f], R["alpha"][f], rho = lit_props(M, p, T, rho_form)
            if rho_form:
                R["rho"][f] = rho
        off += size
    return R


# ---- the same, vectorised; alt names ONE rounding to form differently (tests/test_thermo.py shows that each changes a compared bit) -----------------
def _fma_or(alt, name, a, b, c):
    if name in alt:
        with np.errstate(all="ignore"):
            return a * b + c
    return fma_v(a, b, c)


def _sel(M, T, key, k):
    return np.where(T < M["Tcommon"], M["low" + key][k], M["high" + key][k])


def _cp_chain(M, T, alt=()):
    a = [_sel(M, T, "CpCoeffs", k) for k in range(5)]
    x = a[4]
    for k in (3, 2, 1, 0):
        x = _fma_or(alt, "cp_chain", x, T, a[k])
    return x


def v_cp(M, T, alt=()):
    if M["thermo"] == 0:
        return np.full(T.shape, M["CpW"])
    if M["thermo"] == 1:
        return np.full(T.shape, M["cpE"])
    return RR * _cp_chain(M, T, alt)


def v_cv(M, T, alt=()):
    """cp - cpMcv as Cv meets it; alt "cv": janaf's product rounded first.  gamma keeps the product rounded: v_gamma"""
    with np.errstate(all="ignore"):
        if M["thermo"] == 2 and "cv" not in alt:
            return fma_v(np.full(T.shape, RR), _cp_chain(M, T, alt), np.full(T.shape, -M["cpMcv"]))
        return v_cp(M, T, alt) - M["cpMcv"]


def v_gamma(M, T, alt=()):
    """cp/(cp - cpMcv) with cp rounded (thermoI.H:148-149: the product has two uses); alt "gamma": the subtraction contracted as in Cv"""
    with np.errstate(all="ignore"):
        cp = v_cp(M, T)
        return cp / (v_cv(M, T) if "gamma" in alt else cp - M["cpMcv"])


def v_hs_minus(M, T, q, es, alt=()):
    with np.errstate(all="ignore"):
        if M["thermo"] == 2:
            lo = T < M["Tcommon"]
            x = np.where(lo, M["lowCpCoeffs"][4] * 0.2, M["highCpCoeffs"][4] * 0.2) if "fifth" in alt else _sel(M, T, "H", 3)
            third = np.where(lo, M["lowCpCoeffs"][2] * (1.0 / 3.0), M["highCpCoeffs"][2] * (1.0 / 3.0)) if "third" in alt else _sel(M, T, "H", 1)
            for c in (_sel(M, T, "H", 2), third, _sel(M, T, "H", 0), _sel(M, T, "CpCoeffs", 0), _sel(M, T, "CpCoeffs", 5)):
                x = _fma_or(alt, "ha_chain", x, T, c)
            hs = _fma_or(alt, "ha_hc", np.full(T.shape, RR), x, np.full(T.shape, -M["hc"]))
            return hs - q if es else hs
        cp = v_cp(M, T)
        return _fma_or(alt, "es", cp, T, -q) if es else cp * T


def v_he(M, p, T, alt=()):
    with np.errstate(all="ignore"):
        if M["energy"] == 0:
            if "per_mass" in alt and M["thermo"] == 0:             # Cp*T without the round trip through W
                return M["Cp"] * T
            return v_hs_minus(M, T, 0.0, False, alt) / M["W"]
        rho = p / (M["R"] * T)
        q = p * (M["W"] / rho) if "q_regroup" in alt else (p * M["W"]) / rho
        return v_hs_minus(M, T, q, True, alt) / M["W"]


def v_cpv(M, T, energy=None, alt=()):
    e = M["energy"] if energy is None else energy
    return v_cp(M, T, alt) / M["W"] if e == 0 else v_cv(M, T, alt) / M["W"]


def v_limit(M, T):
    if M["thermo"] != 2:
        return T
    with np.errstate(all="ignore"):
        a = np.where(T > M["Tlow"], T, M["Tlow"])
        c = np.where(a < M["Thigh"], a, M["Thigh"])
        return np.where((T < M["Tlow"]) | (T > M["Thigh"]), c, T)


def v_the(M, f, p, T0, alt=()):
    """-> (T, evaluations, crossed: consecutive iterates on different sides of Tcommon, clamped_low, clamped_high)"""
    n = T0.shape[0]
    Tnew, Ttol, it = T0.copy(), T0 * 1.0e-4, np.zeros(n, dtype=np.int32)
    crossed, lo_hit, hi_hit = (np.zeros(n, dtype=bool) for _ in range(3))
    active = np.arange(n)
    with np.errstate(all="ignore"):
        while active.size:
            Test = Tnew[active]
            raw = Test - (v_he(M, p[active], Test, alt) - f[active]) / v_cpv(M, Test, alt=alt)
            new = v_limit(M, raw)
            if M["thermo"] == 2:
                crossed[active] |= (Test < M["Tcommon"]) != (new < M["Tcommon"])
                lo_hit[active] |= (raw < M["Tlow"]) & (new == M["Tlow"])
                hi_hit[active] |= (raw > M["Thigh"]) & (new == M["Thigh"])
            it[active] += 1
            over = it[active] - 1 > 100
            new = np.where(over, NAN, new)
            Tnew[active] = new
            active = active[~over & (np.abs(new - Test) > Ttol[active])]
    return Tnew, it, crossed, lo_hit, hi_hit


def v_mu(M, T):
    with np.errstate(all="ignore"):
        return np.full(T.shape, M["mu"]) if M["transport"] == 0 else (M["As"] * np.sqrt(T)) / (1.0 + M["Ts"] / T)


def v_kappa(M, T, alt=()):
    with np.errstate(all="ignore"):
        if M["transport"] == 0:
            return (v_cpv(M, T, alt=alt) * M["mu"]) * M["rPr"]
        Cv_ = v_cpv(M, T, 1, alt)
        return (v_mu(M, T) * Cv_) * (1.32 + (1.77 * M["R"]) / Cv_)


def v_props(M, p, T, rho_form, alt=()):
    with np.errstate(all="ignore"):
        psi = M["W"] / (RR * T) if "psi_regroup" in alt else 1.0 / (M["R"] * T)
        if M["transport"] == 0:
            alpha = np.full(T.shape, M["mu"] / M["Pr"] if "rpr_regroup" in alt else M["mu"] * M["rPr"])
        else:
            alpha = v_kappa(M, T, alt) / v_cpv(M, T, alt=alt)
        rho = np.full(T.shape, NAN) if rho_form == 0 else p / (M["R"] * T) if rho_form == 1 else psi * p
    return psi, v_mu(M, T), alpha, rho


def restate_calculate(M, he, p, t0, rho_form=0, alt=()):
    T, it, crossed, lo_hit, hi_hit = v_the(M, he, p, t0, alt)
    psi, mu, alpha, rho = v_props(M, p, T, rho_form, alt)
    return dict(T=T, psi=psi, mu=mu, alpha=alpha, rho=rho, iters=it, crossed=crossed, lo_hit=lo_hit, hi_hit=hi_hit)


def restate_property(M, kind, p, T, alt=()):
    with np.errstate(all="ignore"):
        gamma = v_gamma(M, T, alt)
        return {"Cp": lambda: v_cpv(M, T, 0, alt), "Cv": lambda: v_cpv(M, T, 1, alt), "gamma": lambda: gamma, "Cpv": lambda: v_cpv(M, T, alt=alt),
                "CpByCpv": lambda: np.ones(T.shape) if M["energy"] == 0 else gamma, "kappa": lambda: v_kappa(M, T, alt)}[kind]()


def restate_boundary(M, kinds, sizes, B, rho_form=0, t_into_he=False):
    R = {k: B[k].copy() for k in ("he", "p", "T", "psi", "mu", "alpha", "rho")}
    kind = np.concatenate([np.full(s, k) for k, s in zip(kinds, sizes)]) if len(sizes) else np.zeros(0, dtype=int)
    f1, f2 = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    T = R["T"].copy()
    R["he"][f1] = v_he(M, R["p"][f1], T[f1])
    T[f2] = v_the(M, B["he"][f2], R["p"][f2], T[f2])[0]
    R["he" if t_into_he else "T"][f2] = T[f2]
    on = np.flatnonzero(kind != 0)
    psi, mu, alpha, rho = v_props(M, R["p"][on], T[on], rho_form)
    R["psi"][on], R["mu"][on], R["alpha"][on] = psi, mu, alpha
    if rho_form:
        R["rho"][on] = rho
    return R


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def inputs(syn, M, n, seed):
    """he, p, t0 for n elements (a prefix of the same 1537): true temperatures over both janaf ranges, start temperatures within the
    tolerance (one evaluation), 1 % off and up to 50 % off, and from index 3 on every second element one special: a negative start (102
    evaluations, NaN), he = NaN (1 evaluation, NaN), he of a temperature below Tlow and of one above Thigh (janaf's clamp), a pair of
    iterates across Tcommon, a far start (three or more evaluations)"""
    N = 1537
    u = [syn.splitmix_uniform(seed + k, N) for k in range(4)]
    Tc = M["Tcommon"] if M["thermo"] == 2 else 1000.0
    Tt = 260.0 + u[0] * 2300.0
    p = 5.0e4 + u[1] * 1.5e5
    third = np.arange(N) % 3
    f = np.where(third == 0, 1.0 + 5.0e-5 * (u[2] - 0.5), np.where(third == 1, 1.0 + 0.02 * (u[2] - 0.5), 0.5 + u[2]))
    t0 = Tt * f
    Thigh = M["Thigh"] if M["thermo"] == 2 else 6000.0
    Tt[7], Tt[9], Tt[11], Tt[13], Tt[15] = 100.0, Thigh * 1.2, Tc * 1.2, 2500.0, Tc * 0.8
    t0[7], t0[9], t0[11], t0[13], t0[15] = 300.0, Thigh * 0.9, Tc * 0.8, 300.0, Tc * 1.3
    he = v_he(M, p, Tt)
    t0[3] = -300.0
    he[5] = NAN
    return dict(he=he[:n].copy(), p=p[:n].copy(), t0=t0[:n].copy(), Tt=Tt[:n].copy())


def patch_kinds(L):
    """a kind-1 (fixesValue) patch between kind-2 patches and a kind-0 (empty) patch, in the mesh's patch order"""
    return list((2, 1, 2, 0, 2, 1)[:len(L["patches"])])


def boundary_inputs(syn, M, L, seed):
    """patch-ordered boundary arrays: he of a true temperature, T 1 % or 20 % off it, the outputs seeded with NaN"""
    sizes = [fc.shape[0] for fc, _ in L["patches"]]
    nb = int(sum(sizes))
    u = [syn.splitmix_uniform(seed + k, max(nb, 1))[:nb] for k in range(3)]
    Tt = 280.0 + u[0] * 1900.0
    p = 6.0e4 + u[1] * 1.2e5
    T = Tt * np.where(np.arange(nb) % 2 == 0, 1.0 + 0.02 * (u[2] - 0.5), 0.8 + 0.4 * u[2])
    B = dict(he=v_he(M, p, Tt), p=p, T=T)
    for k in ("psi", "mu", "alpha", "rho"):
        B[k] = np.full(nb, NAN)
    return sizes, B


# ---- the walk of the driver (foam/thermoBox.C): the constructor and three correct() ------------------------------------------------------------
def walk_rule(step, he, p):
    """what the driver does to he and p between two correct() calls: a fixed rule in exactly rounded operations"""
    with np.errstate(all="ignore"):
        return he * (1.0 + 0.03125 * step), p * (1.0 - 0.015625 * step)


def restate_walk(M, kinds, sizes, T, p, bT, bp, rho_form=2, steps=3):
    """heThermo::init (he = HE(p, T) on the cells and on every patch that is not skipped) and calculate(), then `steps` times the rule and
    correct() -> the list of states (dicts of cell and boundary arrays) after each calculate()"""
    kind = np.concatenate([np.full(s, k) for k, s in zip(kinds, sizes)])
    on = kind != 0
    he = v_he(M, p, T)
    bhe = np.where(on, v_he(M, bp, bT), NAN)
    B = dict(he=bhe, p=bp.copy(), T=bT.copy())
    for k in ("psi", "mu", "alpha", "rho"):
        B[k] = np.full(bT.shape[0], NAN)
    states, Tc, pc = [], T.copy(), p.copy()
    for step in range(steps + 1):
        if step:
            he, pc = walk_rule(step, he, pc)
            B["he"], B["p"] = walk_rule(step, B["he"], B["p"])
        C = restate_calculate(M, he, pc, Tc, rho_form)
        Tc = C["T"]
        B = restate_boundary(M, kinds, sizes, B, rho_form)
        states.append(dict(T=C["T"].copy(), psi=C["psi"], mu=C["mu"], alpha=C["alpha"], rho=C["rho"], he=he.copy(), p=pc.copy(),
                           **{"b" + k: v.copy() for k, v in B.items()}))
    return states
