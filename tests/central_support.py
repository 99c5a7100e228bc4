"""rhoCentralFoam's Kurganov and Tadmor face fluxes restated twice (rhoCentralFoam.C:60-185, compressibleCourantNo.H:35-47):
literal loops over Python floats with an explicit fma, and vectorised numpy with the element-wise fma of interface_support (fma_v).  The
kernels of csrc/central.inc are compared with the vectorised form bit for bit; a CPU test shows that the two forms agree and that the
inputs reach every branch.

The limiter of the literal form is limiter_face of tests/test_limited_schemes.py, the restatement the engine's lim_face is held to.  The
vectorised form restates the three limiters of the ratio r that the GPU cases use (vanLeer, vanAlbada, Minmod; scalar, V and bounded) in
numpy; the kinds that read more than r (QUICK, limitedCubic, ...) take limiter_face face by face there too.

A mesh here is interface_support.mesh's dict with cell centres, magSf and linear weights added.  Fields of one side of a face travel as a
dict F: rho, rhoU[3], rPsi, e, c, gRho[3], gRhoU[9], gRPsi[3], gE[3], gC[3], limU, gLimU[3]; face values as V: name -> (pos, neg)."""
import math

import numpy as np

from assembly_support import rmax, rmin
from interface_support import div, dot3, dot3_v, fma, fma_v
from interface_support import mesh as _mesh
from test_limited_schemes import Hits, limiter_face, weight

MESHES = ("box", "edge_257", "isolated")
FLUX_SCHEMES = ("Kurganov", "Tadmor")
# reconstruct(rho), reconstruct(U), reconstruct(T).  "cubic" adds the arms of the switch that gather more than the upwind cell's gradient
LIMITER_SETS = {"vanLeer": ("vanLeer", "vanLeerV", "vanLeer"),
                "mixed": ("vanAlbada", "Minmod", "limitedVanLeer 0 260000"),
                "cubic": ("limitedCubic 1", "QUICKV", "QUICK")}
SCALARS = ("rho", "rPsi", "e", "c")
GRAD_OF = {"rho": "gRho", "rPsi": "gRPsi", "e": "gE", "c": "gC"}
SLOT_OF = {"rho": 0, "rPsi": 2, "e": 2, "c": 2}
OUT = ("phi", "phiUp0", "phiUp1", "phiUp2", "phiEp", "amaxSf")
OPT = ("a_pos", "aU0", "aU1", "aU2")
_KINDS = ("limitedLinear", "vanLeer", "MUSCL", "Minmod", "SuperBee", "UMIST", "vanAlbada", "OSPRE", "QUICK", "limitedCubic", "Gamma", "SFCD")
_BOUNDED = {"limitedLimitedLinear": "limitedLinear", "limitedVanLeer": "vanLeer", "limitedMUSCL": "MUSCL", "limitedLimitedCubic": "limitedCubic",
            "limitedGamma": "Gamma"}
_VECTOR_R = ("vanLeer", "vanAlbada", "Minmod")


def slot(text):
    """a reconstruct(...) entry -> dict(kind, vec, bounds, k) as limiter_face takes them"""
    tok = text.split()
    name, nums = tok[0], [float(x) for x in tok[1:]]
    vec, bounds, k = False, None, 0.0
    if name in _BOUNDED:
        name = _BOUNDED[name]
        bounds = (nums[-2], nums[-1])
        nums = nums[:-2]
    elif name.endswith("V") and name[:-1] in _KINDS:
        name, vec = name[:-1], True
    assert name in _KINDS, text
    if nums:
        k = nums[0]
    return dict(kind=name, vec=vec, bounds=bounds, k=k, text=text)


def slots(names):
    return [slot(t) for t in names]


# ---- meshes and inputs ---------------------------------------------------------------------------------------------------------------------
def mesh(pkg, name):
    """interface_support.mesh with seeded cell centres C, magSf = |Sf| and linear weights cdw in (0.3, 0.7)"""
    L = dict(_mesh(pkg, name))
    u = pkg.synthetic.splitmix_uniform
    nf = L["lo"].shape[0]
    L["C"] = [u(900 + d, L["n"]) for d in range(3)]
    L["magSf"] = np.sqrt(L["Sf"][0] * L["Sf"][0] + L["Sf"][1] * L["Sf"][1] + L["Sf"][2] * L["Sf"][2])
    L["cdw"] = 0.3 + 0.4 * u(903, nf)
    return L


def inputs(syn, n, seed):
    """the fields of n cells (or patch faces) in four runs of consecutive cells, so that most faces join cells of one kind: a quarter at rest
    with every field uniform (U exactly zero; equal neighbours: the limiter's 1000* guard), a quarter supersonic along (1, 0.8, 0.6), a
    quarter supersonic against it, a quarter subsonic.  rho about 1, c about 340, rPsi about 8e4, e between 2e5 and 3e5 (the bounded
    limiter of the "mixed" set clips above 2.6e5).  The gradients are seeded numbers of the fields' order, not gradients of them"""
    u = lambda k: syn.splitmix_uniform(seed + k, max(n, 1))[:n]
    kind = (4 * np.arange(n)) // max(n, 1)
    rho = 0.6 + 0.8 * u(0)
    speed = np.where(kind == 1, 900.0 + 600.0 * u(1), np.where(kind == 2, -(900.0 + 600.0 * u(1)), 0.0))
    U = [speed * a + np.where(kind == 3, 200.0 * (u(2 + d) - 0.5), 0.0) for d, a in enumerate((1.0, 0.8, 0.6))]
    rPsi = 7.0e4 + 2.0e4 * u(5)
    e = 2.0e5 + 1.0e5 * u(6)
    c = 300.0 + 80.0 * u(7)
    rest = kind == 0
    rho[rest], rPsi[rest], e[rest], c[rest] = 1.0, 8.0e4, 2.5e5, 340.0
    rhoU = [rho * x for x in U]
    F = dict(rho=rho, rhoU=rhoU, rPsi=rPsi, e=e, c=c)
    F["gRho"] = [2.0 * (u(10 + d) - 0.5) for d in range(3)]
    F["gRhoU"] = [2000.0 * (u(13 + d) - 0.5) for d in range(9)]
    F["gRPsi"] = [4.0e4 * (u(22 + d) - 0.5) for d in range(3)]
    F["gE"] = [2.0e5 * (u(25 + d) - 0.5) for d in range(3)]
    F["gC"] = [100.0 * (u(28 + d) - 0.5) for d in range(3)]
    F["limU"] = dot3_v(rhoU, rhoU)
    F["gLimU"] = [2.0e6 * (u(31 + d) - 0.5) for d in range(3)]
    for key in ("gRho", "gRPsi", "gE", "gC", "gLimU", "gRhoU"):
        for g in F[key]:
            g[rest] = 0.0
    return F


def gather(F, idx):
    """the fields of one side of every face: F at the cells idx"""
    return {k: ([a[idx] for a in v] if isinstance(v, list) else v[idx]) for k, v in F.items()}


# ---- literal loops ----------------------------------------------------------------------------------------------------------------------------
def lit_weights(s, cdw, pP, pN, gP, gN, d, hit):
    """the limited weights towards pos (faceFlux +1.0) and towards neg (-1.0)"""
    out = []
    for fl in (1.0, -1.0):
        lim = limiter_face(s["kind"], s["vec"], s["bounds"], s["k"], cdw, fl, pP, pN, gP, gN, d, hit)
        out.append(weight(lim, cdw, fl))
    return out


def lit_interp(w, vP, vN, coupled):
    """surfaceInterpolationScheme.C:274-279 on an internal face, :361-366 on a coupled patch"""
    return w * vP + (1.0 - w) * vN if coupled else fma(w, vP - vN, vN)


def lit_flux(v, s, magSf, tadmor, hit=lambda key: None):
    """rhoCentralFoam.C:107-185 on one face.  v: name -> [pos, neg] (rhoU: [[3], [3]]); s the face area vector"""
    U = [[div(v["rhoU"][d][k], v["rho"][d]) for k in range(3)] for d in range(2)]
    p = [v["rho"][d] * v["rPsi"][d] for d in range(2)]
    phiv = [dot3(U[d], s) for d in range(2)]
    cSf = [v["c"][d] * magSf for d in range(2)]
    in_p, in_m = rmax(phiv[0] + cSf[0], phiv[1] + cSf[1]), rmin(phiv[0] - cSf[0], phiv[1] - cSf[1])
    ap, am = rmax(in_p, 0.0), rmin(in_m, 0.0)
    if (in_p == 0 and math.copysign(1.0, in_p) < 0) or (in_m == 0 and math.copysign(1.0, in_m) < 0):
        hit("minus_zero")
    a_pos = div(ap, ap - am)
    amaxSf = rmax(abs(am), abs(ap))
    aSf = am * a_pos
    if am == 0 and ap > 0:
        assert a_pos == 1.0 and aSf == 0.0
        hit("supersonic_pos")
    elif ap == 0 and am < 0:
        assert a_pos == 0.0
        hit("supersonic_neg")
    elif am < 0 < ap:
        hit("subsonic")
    if all(x == 0 for d in range(2) for x in U[d]):
        hit("at_rest")
    if tadmor:
        aSf = -0.5 * amaxSf
        a_pos = 0.5
    a_neg = 1.0 - a_pos
    phiv = [phiv[0] * a_pos, phiv[1] * a_neg]
    fp, fn = phiv[0] - aSf, phiv[1] + aSf
    out = dict(amaxSf=rmax(abs(fp), abs(fn)), a_pos=a_pos)
    out["phi"] = fp * v["rho"][0] + fn * v["rho"][1]
    pf = a_pos * p[0] + a_neg * p[1]
    for k in range(3):
        out["phiUp%d" % k] = (fp * v["rhoU"][0][k] + fn * v["rhoU"][1][k]) + pf * s[k]
        out["aU%d" % k] = a_pos * U[0][k] + a_neg * U[1][k]
    h = [v["rho"][d] * (v["e"][d] + 0.5 * dot3(U[d], U[d])) + p[d] for d in range(2)]
    out["phiEp"] = ((fp * h[0] + fn * h[1]) + aSf * p[0]) - aSf * p[1]
    return out


def literal_faces(S, cdw, A, B, d, Sf, magSf, tadmor, coupled=False, hit=lambda key: None):
    """the face pass over per-face sides A (owner) and B (neighbour), d the three delta arrays -> name -> array"""
    rows = []
    for f in range(cdw.shape[0]):
        at = lambda X, key, j=None: float(X[key][f]) if j is None else float(X[key][j][f])
        dd = [float(d[k][f]) for k in range(3)]
        w = float(cdw[f])
        v = {}
        for name in SCALARS:
            g = GRAD_OF[name]
            vP, vN = at(A, name), at(B, name)
            ws = lit_weights(S[SLOT_OF[name]], w, vP, vN, [at(A, g, k) for k in range(3)], [at(B, g, k) for k in range(3)], dd, hit)
            v[name] = [lit_interp(x, vP, vN, coupled) for x in ws]
        uP, uN = [at(A, "rhoU", k) for k in range(3)], [at(B, "rhoU", k) for k in range(3)]
        if S[1]["vec"]:
            ws = lit_weights(S[1], w, uP, uN, [at(A, "gRhoU", k) for k in range(9)], [at(B, "gRhoU", k) for k in range(9)], dd, hit)
        else:
            ws = lit_weights(S[1], w, at(A, "limU"), at(B, "limU"), [at(A, "gLimU", k) for k in range(3)], [at(B, "gLimU", k) for k in range(3)], dd, hit)
        v["rhoU"] = [[lit_interp(x, uP[k], uN[k], coupled) for k in range(3)] for x in ws]
        rows.append(lit_flux(v, [float(Sf[k][f]) for k in range(3)], float(magSf[f]), tadmor, hit))
    return {k: np.array([r[k] for r in rows]) for k in OUT + OPT}


def literal_sound_speed(Cp, Cv, psi):
    rPsi = [div(1.0, x) for x in psi.tolist()]
    c = []
    for a, b, r in zip(Cp.tolist(), Cv.tolist(), rPsi):
        x = div(a, b) * r
        c.append(math.sqrt(x) if x >= 0 else float("nan"))
    return np.array(rPsi), np.array(c)


# ---- the same, vectorised ------------------------------------------------------------------------------------------------------------------------
def _sign_v(x):
    return np.where(x >= 0, 1.0, -1.0)


def v_limiter(s, cdw, fl, pP, pN, gP, gN, d):
    """the limiter at a uniform faceFlux fl: numpy for the limiters of the ratio r, limiter_face face by face for the others"""
    kind, vec, bounds = s["kind"], s["vec"], s["bounds"]
    if kind not in _VECTOR_R:
        m = cdw.shape[0]
        col = lambda X, f: [float(x[f]) for x in X] if isinstance(X, list) else float(X[f])
        return np.array([limiter_face(kind, vec, bounds, s["k"], float(cdw[f]), fl, col(pP, f), col(pN, f), col(gP, f), col(gN, f),
                                      [float(d[k][f]) for k in range(3)]) for f in range(m)])
    g = gP if fl > 0 else gN                                                # NVDTVD.H:110: the upwind cell's gradient
    with np.errstate(all="ignore"):
        if vec:
            gfV = [pN[j] - pP[j] for j in range(3)]
            gradf = dot3_v(gfV, gfV)
            gradcf = dot3_v(gfV, [dot3_v(d, g[3 * j:3 * j + 3]) for j in range(3)])
        else:
            gradf = pN - pP
            gradcf = dot3_v(d, g)
        guard = np.abs(gradcf) >= 1000 * np.abs(gradf)
        safe = np.where(guard, 1.0, gradf)
        r = np.where(guard, 2 * 1000 * _sign_v(gradcf) * _sign_v(gradf) - 1, fma_v(2.0, gradcf / safe, -1.0))
        if kind == "vanLeer":
            lim = (r + np.abs(r)) / (1 + np.abs(r))
        elif kind == "vanAlbada":
            lim = r * (r + 1) / fma_v(r, r, 1.0)
        else:
            lim = np.where(np.where(r < 1.0, r, 1.0) > 0.0, np.where(r < 1.0, r, 1.0), 0.0)
        if bounds is not None:
            lo, hi = bounds
            out = (pP < lo) | (pN > hi) if fl > 0 else (pN < lo) | (pP > hi)
            lim = np.where(out, 0.0, lim)
    return lim


def v_weights(s, cdw, pP, pN, gP, gN, d):
    lp, ln = v_limiter(s, cdw, 1.0, pP, pN, gP, gN, d), v_limiter(s, cdw, -1.0, pP, pN, gP, gN, d)
    return fma_v(lp, cdw, (1.0 - lp) * 1.0), fma_v(ln, cdw, (1.0 - ln) * 0.0)


def v_interp(w, vP, vN, coupled):
    return w * vP + (1.0 - w) * vN if coupled else fma_v(w, vP - vN, vN)


def restate_reconstruct(S, cdw, A, B, d, coupled=False):
    """the ten interpolations -> V: name -> (pos, neg); rhoU -> ([3], [3])"""
    V = {}
    for name in SCALARS:
        g = GRAD_OF[name]
        ws = v_weights(S[SLOT_OF[name]], cdw, A[name], B[name], A[g], B[g], d)
        V[name] = tuple(v_interp(w, A[name], B[name], coupled) for w in ws)
    if S[1]["vec"]:
        ws = v_weights(S[1], cdw, A["rhoU"], B["rhoU"], A["gRhoU"], B["gRhoU"], d)
    else:
        ws = v_weights(S[1], cdw, A["limU"], B["limU"], A["gLimU"], B["gLimU"], d)
    V["rhoU"] = tuple([v_interp(w, A["rhoU"][k], B["rhoU"][k], coupled) for k in range(3)] for w in ws)
    return V


def boundary_values(F):
    """any patch that is not coupled: the boundary value is the face value of both directions"""
    return {k: (F[k], F[k]) for k in SCALARS + ("rhoU",)}


def restate_flux(V, Sf, magSf, tadmor, alt=()):
    """rhoCentralFoam.C:107-185 over face arrays.  alt: the roundings the CPU test shows to be visible -- "magsqr_plain" (no contraction),
    "reciprocal" (U = rhoU*(1/rho)), "asf_factored" (aSf*(p_pos - p_neg))"""
    with np.errstate(all="ignore"):
        if "reciprocal" in alt:
            U = [[V["rhoU"][d][k] * (1.0 / V["rho"][d]) for k in range(3)] for d in range(2)]
        else:
            U = [[V["rhoU"][d][k] / V["rho"][d] for k in range(3)] for d in range(2)]
        p = [V["rho"][d] * V["rPsi"][d] for d in range(2)]
        phiv = [dot3_v(U[d], Sf) for d in range(2)]
        cSf = [V["c"][d] * magSf for d in range(2)]
        vmax = lambda a, b: np.where(a > b, a, b)
        vmin = lambda a, b: np.where(a < b, a, b)
        ap = vmax(vmax(phiv[0] + cSf[0], phiv[1] + cSf[1]), 0.0)
        am = vmin(vmin(phiv[0] - cSf[0], phiv[1] - cSf[1]), 0.0)
        a_pos = ap / (ap - am)
        amaxSf = vmax(np.abs(am), np.abs(ap))
        aSf = am * a_pos
        if tadmor:
            aSf = -0.5 * amaxSf
            a_pos = np.full(ap.shape, 0.5)
        a_neg = 1.0 - a_pos
        phiv = [phiv[0] * a_pos, phiv[1] * a_neg]
        fp, fn = phiv[0] - aSf, phiv[1] + aSf
        out = dict(amaxSf=vmax(np.abs(fp), np.abs(fn)), a_pos=a_pos)
        out["phi"] = fp * V["rho"][0] + fn * V["rho"][1]
        pf = a_pos * p[0] + a_neg * p[1]
        for k in range(3):
            out["phiUp%d" % k] = (fp * V["rhoU"][0][k] + fn * V["rhoU"][1][k]) + pf * Sf[k]
            out["aU%d" % k] = a_pos * U[0][k] + a_neg * U[1][k]
        if "magsqr_plain" in alt:
            msq = [U[d][0] * U[d][0] + U[d][1] * U[d][1] + U[d][2] * U[d][2] for d in range(2)]
        else:
            msq = [dot3_v(U[d], U[d]) for d in range(2)]
        h = [V["rho"][d] * (V["e"][d] + 0.5 * msq[d]) + p[d] for d in range(2)]
        if "asf_factored" in alt:
            out["phiEp"] = (fp * h[0] + fn * h[1]) + aSf * (p[0] - p[1])
        else:
            out["phiEp"] = ((fp * h[0] + fn * h[1]) + aSf * p[0]) - aSf * p[1]
    return out


def restate_internal(L, S, F, tadmor, alt=(), coupled_rule=False):
    """mi_central_flux on the mesh L; coupled_rule: the two-product interpolate in the internal-face rule's place (an alternative)"""
    lo, up = L["lo"], L["up"]
    d = [c[up] - c[lo] for c in L["C"]]
    V = restate_reconstruct(S, L["cdw"], gather(F, lo), gather(F, up), d, coupled_rule)
    return restate_flux(V, L["Sf"], L["magSf"], tadmor, alt), V


def restate_sound_speed(Cp, Cv, psi, regroup=False):
    """regroup: Cp/(Cv*psi), the alternative"""
    with np.errstate(all="ignore"):
        rPsi = 1.0 / psi
        return rPsi, np.sqrt(Cp / (Cv * psi) if regroup else (Cp / Cv) * rPsi)


def courant_products(dc, magSf, amaxSf):
    """-> deltaCoeffs*amaxSf and (deltaCoeffs*amaxSf)/magSf, the stored products mi_sum and mi_min_max are run over"""
    with np.errstate(all="ignore"):
        p = dc * amaxSf
        return p, p / magSf


# ---- patches ---------------------------------------------------------------------------------------------------------------------------------------
def patch_case(syn):
    """the 429-face patch of interface_support.patch_case: cell fields, their patchNeighbourFields, the patch's weights, delta, Sf and magSf,
    and the seven boundary-value arrays of the plain form (the patchNeighbourField's values)"""
    u = syn.splitmix_uniform
    n = 13 * 11 * 9
    fc = np.arange(0, n, 3, dtype=np.int32)
    m = fc.shape[0]
    Sf = [u(940 + d, m) - 0.5 for d in range(3)]
    return dict(n=n, fc=fc, m=m, cells=inputs(syn, n, 4100), nbr=inputs(syn, m, 4200), w=0.3 + 0.4 * u(943, m), pd=[u(944 + d, m) - 0.5 for d in range(3)],
                Sf=Sf, magSf=np.sqrt(Sf[0] * Sf[0] + Sf[1] * Sf[1] + Sf[2] * Sf[2]))


def restate_patch(P, S, tadmor, coupled=True, values=None):
    """coupled: the limiter and the two-product interpolate between the cells behind the patch and the patchNeighbourField; otherwise the
    plain form over `values` (default: the patchNeighbourField's seven value arrays)"""
    if coupled:
        V = restate_reconstruct(S, P["w"], gather(P["cells"], P["fc"]), P["nbr"], P["pd"], True)
    else:
        V = boundary_values(P["nbr"] if values is None else values)
    return restate_flux(V, P["Sf"], P["magSf"], tadmor)


# ---- the shock tube walk (foam/shockTube.C) --------------------------------------------------------------------------------------------------------
TUBE = dict(n=120, length=10.0, dt=1.0e-5, pL=1.0e5, TL=348.4, pR=1.0e4, TR=278.2, steps=3)
TUBE_AIR = dict(W=28.96, Cv=717.5, Hf=0.0, mu=1.8e-05, Pr=0.7, Cp=0.0, As=0.0, Ts=0.0)


def tube_mesh(n=TUBE["n"], length=TUBE["length"]):
    """n x 1 x 1 cells of unit cross-section along x; two plain end patches of one face each, the empty side patches left out"""
    h = length / n
    lo, up = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    one, zero = np.ones(n - 1), np.zeros(n - 1)
    x = (np.arange(n) + 0.5) * h - 0.5 * length
    return dict(n=n, lo=lo, up=up, Sf=[one, zero.copy(), zero.copy()], magSf=one.copy(), cdw=np.full(n - 1, 0.5), dc=np.full(n - 1, 1.0 / h),
                C=[x, np.zeros(n), np.zeros(n)], vol=np.full(n, h), fcs=[np.array([0], dtype=np.int32), np.array([n - 1], dtype=np.int32)],
                bSf=[np.array([-1.0, 1.0]), np.zeros(2), np.zeros(2)], bMagSf=np.ones(2), bdc=np.full(2, 2.0 / h), bcells=np.array([0, n - 1]))


def tube_start(L):
    left = L["C"][0] < 0
    return np.where(left, TUBE["pL"], TUBE["pR"]), np.where(left, TUBE["TL"], TUBE["TR"])


def gauss_grad(L, w, x, bx):
    """fvc::grad, Gauss linear, as mi_face_interpolate, mi_gauss_grad, mi_patch_add_product and mi_vec_div form it: the linear face value, per cell
    fma(Sf, ssf, .) over its own faces, fma(-Sf, ssf, .) over its neighbour-side faces, fma(Sf_b, x_b, .) per boundary face (mi_patch_add_product), /V"""
    lo, up = L["lo"], L["up"]
    ssf = fma_v(w, x[lo] - x[up], x[up])
    out = []
    for k in range(3):
        g = np.zeros(L["n"])
        own, nei = fma_v(L["Sf"][k], ssf, np.zeros(ssf.shape)), None
        g[lo] = own                                                          # a tube cell owns at most one face
        nei = fma_v(-L["Sf"][k], ssf, g[up])
        g[up] = nei
        g[L["bcells"]] = fma_v(L["bSf"][k], bx, g[L["bcells"]])          # one boundary face a cell
        out.append(g / L["vol"])
    return out


def explicit_solve(L, r_delta_t, old, flux, bflux):
    """solve(fvm::ddt(x) + fvc::div(flux)) as mi_fvm_ddt_euler, mi_surface_integrate, mi_patch_add, mi_vec_div and mi_vec_submul form it:
    diag = rDeltaT*V, source = (rDeltaT*old)*V, div = (sum own - sum nei + boundary)/V, source -= V*div, x = source/diag"""
    diag, source = r_delta_t * L["vol"], (r_delta_t * old) * L["vol"]
    s = np.zeros(L["n"])
    np.add.at(s, L["lo"], flux)
    np.subtract.at(s, L["up"], flux)
    np.add.at(s, L["bcells"], bflux)
    dv = s / L["vol"]
    source = source - L["vol"] * dv
    return source / diag


def restate_walk(M, L, S, tadmor, steps=TUBE["steps"]):
    """the inviscid statements of rhoCentralFoam.C on the tube -> the list of states after each step.  The boundary fields of the two
    zeroGradient end patches follow the reference: rho_b = psi_b*p_b, rhoU_b = rho_b*U_b, the others the cell's value"""
    from thermo_support import restate_boundary, restate_calculate, restate_property, v_he
    n, bc = L["n"], L["bcells"]
    p, T = tube_start(L)
    U = [np.zeros(n) for _ in range(3)]
    e = v_he(M, p, T)
    C = restate_calculate(M, e, p, T, 0)
    T, psi = C["T"], C["psi"]
    rho = psi * p
    rhoU = [rho * u for u in U]
    rhoE = rho * (e + 0.5 * dot3_v(U, U))
    b = dict(p=p[bc], T=T[bc], e=e[bc], psi=psi[bc], U=[u[bc] for u in U])
    b["rho"] = b["psi"] * b["p"]
    b["rhoU"] = [b["rho"] * u for u in b["U"]]
    rdt = 1.0 / TUBE["dt"]
    states = []
    for _ in range(steps):
        rPsi, c = restate_sound_speed(restate_property(M, "Cp", p, T), restate_property(M, "Cv", p, T), psi)
        brPsi, bcs = restate_sound_speed(restate_property(M, "Cp", b["p"], b["T"]), restate_property(M, "Cv", b["p"], b["T"]), b["psi"])
        F = dict(rho=rho, rhoU=rhoU, rPsi=rPsi, e=e, c=c)
        Fb = dict(rho=b["rho"], rhoU=b["rhoU"], rPsi=brPsi, e=b["e"], c=bcs)
        for name in SCALARS:
            F[GRAD_OF[name]] = gauss_grad(L, L["cdw"], F[name], Fb[name])
        F["gRhoU"] = [g for k in range(3) for g in gauss_grad(L, L["cdw"], rhoU[k], Fb["rhoU"][k])]
        F["limU"], F["gLimU"] = None, None
        R, _ = restate_internal(L, S, {k: v for k, v in F.items() if v is not None}, tadmor)
        Rb = restate_flux(boundary_values(Fb), L["bSf"], L["bMagSf"], tadmor)
        prod, quot = courant_products(L["dc"], L["magSf"], R["amaxSf"])
        _, bquot = courant_products(L["bdc"], L["bMagSf"], Rb["amaxSf"])
        rho = explicit_solve(L, rdt, rho, R["phi"], Rb["phi"])
        rhoU = [explicit_solve(L, rdt, rhoU[k], R["phiUp%d" % k], Rb["phiUp%d" % k]) for k in range(3)]
        U = [x / rho for x in rhoU]
        b["rho"] = rho[bc]                                                   # solve() ends in correctBoundaryConditions: zeroGradient
        b["U"] = [u[bc] for u in U]
        b["rhoU"] = [b["rho"] * u for u in b["U"]]
        rhoE = explicit_solve(L, rdt, rhoE, R["phiEp"], Rb["phiEp"])
        e = rhoE / rho - 0.5 * (U[0] * U[0] + U[1] * U[1] + U[2] * U[2])     # the tube has U_y = U_z = 0: contracted or not, the same bits
        b["e"] = e[bc]
        C = restate_calculate(M, e, p, T, 0)
        T, psi = C["T"], C["psi"]
        B = restate_boundary(M, [2, 2], [1, 1], dict(he=b["e"], p=b["p"], T=b["T"], psi=b["psi"], mu=np.zeros(2), alpha=np.zeros(2), rho=np.zeros(2)), 0)
        b["T"], b["psi"] = B["T"], B["psi"]
        p = rho / psi
        b["p"] = p[bc]
        b["rho"] = b["psi"] * b["p"]
        states.append(dict(rho=rho.copy(), rhoU0=rhoU[0].copy(), rhoE=rhoE.copy(), e=e.copy(), T=T.copy(), p=p.copy(), psi=psi.copy(),
                           phi=R["phi"], phiEp=R["phiEp"], amaxSf=R["amaxSf"], bphi=Rb["phi"], co_max=float(max(np.max(quot), np.max(bquot))),
                           co_sum_terms=prod, sum_rhoV=float(np.sum(rho * L["vol"])), bflux=float(np.sum(Rb["phi"]))))
    return states
