"""Explicit MULES restated (tests/test_mules.py): MULES::limiter, limit and explicitSolve written out loop by loop, generic over their number
type (float, or fractions.Fraction for exact arithmetic), and the same vectorised over cells and faces; the inputs the tests run on.

The pin is this restatement, not a compiled reference:
  limiter        MULESTemplates.C:381-745 with MULESFunctors.H.  limiterMULESFunctor / patchMinMaxMULESFunctor (:144-348): psiMaxn starts at
                 the global psiMin and psiMinn at the global psiMax; the loop takes max / min over the NEIGHBOUR cells' psi only (the cell's own
                 value is not in it), the patches add psiPf; sumPhiBD is + own, - losort, + boundary; sumPhip / mSumPhim start at VSMALL and
                 `phiCorr > 0.0` picks the branch; both bounds are clamped by the global bounds (:507-508); then the static-mesh expressions
                 (:538-554), one rounding per written operation.  One iteration (:560-744): sumlPhip / mSumlPhim from 0 over lambda*phiCorr,
                 lambdam from (sumlPhip + psiMaxn)/(mSumPhim - SMALL) and lambdap from (mSumlPhim + psiMinn)/(sumPhip + SMALL), each clamped
                 to [0, 1] (the names crossed as :637-638 cross them), the face pass, the three patch branches (wedge, coupled, other).
  limit          :748-813: phiBD = upwind flux = phi*(w*(psiP - psiN) + psiN), w = pos(phi) (surfaceInterpolationScheme.C:273-376); coupled
                 patch faces phi*(w*psiInternal + (1 - w)*psiNeighbour), other patch faces phi*psiPf; phiCorr = phiPsi - phiBD; lambda = 1;
                 the result phiBD + lambda*phiCorr (the product rounded first), or lambda*phiCorr with returnCorr.
  explicitSolve  :36-78, static mesh: surfaceIntegrate (own +, losort -, boundary +, then /V: fvcSurfaceIntegrate.C:40-203), then
                 (rho0*psi0*rDeltaT + Su - that)/(rho*rDeltaT - Sp).
  absent fields  rho None is geometricOneField, Sp / Su None zeroField: the operation is NOT performed (one*x = x, x - zero = x,
                 zero - x = -x: primitives/zero/zeroI.H, one/oneI.H).
  max / min      (a > b) ? a : b and (a < b) ? a : b (label.H:285-297).
A cell meets its own faces ascending, then its neighbour-side faces ascending (losort), then its boundary faces patch after patch.
A mesh is a dict n, lo, up, fcs (the patches' faceCells), kinds (0 other, 1 coupled, 2 fixesValue, as GradBoundary takes them) and wedge (one flag
per patch, optional).  Inputs are a dict (make_inputs); a flux with a boundary is a pair of arrays, the boundary patch-ordered."""
import numpy as np

VSMALL, SMALL = 1e-300, 1e-15                                   # doubleScalar.H:55-57
OTHER, COUPLED, WEDGE = 0, 1, 2                                 # the kind of a boundary face


def face_kinds(L):
    """per boundary face: WEDGE where the patch is flagged, COUPLED where its kind is 1, OTHER elsewhere"""
    wedge = L.get("wedge") or [False] * len(L["fcs"])
    out = [np.full(fc.shape[0], WEDGE if w else (COUPLED if k == 1 else OTHER), dtype=np.int64) for fc, k, w in zip(L["fcs"], L["kinds"], wedge)]
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def boundary_cells(L):
    return np.concatenate(L["fcs"]).astype(np.int64) if L["fcs"] else np.zeros(0, np.int64)


# ---- literal: loop by loop, generic over the number type --------------------------------------------------------------------------------
def _max(a, b):
    return a if a > b else b


def _min(a, b):
    return a if a < b else b


def _cells(L):
    """per cell: own faces ascending, neighbour-side faces ascending, boundary faces patch after patch"""
    n = L["n"]
    own, nei, bnd = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    for f, (o, u) in enumerate(zip(L["lo"].tolist(), L["up"].tolist())):
        own[o].append(f); nei[u].append(f)
    for i, c in enumerate(boundary_cells(L).tolist()):
        bnd[c].append(i)
    return own, nei, bnd


def literal_form(L, I, conv=float):
    """the limit form's opening: (phiBD, bphiBD), (phiCorr, bphiCorr), (lambda, blambda) from phi and phiPsi"""
    one = conv(1.0)
    zero = one - one
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    psi, bpsi = col(I["psi"]), col(I["bpsi"])
    (phi, bphi), (phiPsi, bphiPsi) = [(col(a), col(b)) for a, b in (I["phi"], I["phiPsi"])]
    lo, up, bc, kind = L["lo"].tolist(), L["up"].tolist(), boundary_cells(L).tolist(), face_kinds(L).tolist()
    bd, corr = [], []
    for f in range(len(lo)):
        w = one if phi[f] >= 0 else zero
        P, N = psi[lo[f]], psi[up[f]]
        bd.append(phi[f] * (w * (P - N) + N))
        corr.append(phiPsi[f] - bd[f])
    bbd, bcorr = [], []
    for i in range(len(bc)):
        face = bpsi[i]
        if kind[i] == COUPLED:
            w = one if bphi[i] >= 0 else zero
            face = w * psi[bc[i]] + (one - w) * bpsi[i]
        bbd.append(bphi[i] * face)
        bcorr.append(bphiPsi[i] - bbd[i])
    return (bd, bbd), (corr, bcorr), ([one] * len(lo), [one] * len(bc))


def _cell_fields(I, conv):
    col = lambda a: None if a is None else [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    n = np.asarray(I["psi"]).shape[0]
    rdt = col(I["rdt"]) if isinstance(I["rdt"], np.ndarray) else [conv(I["rdt"])] * n
    return rdt, col(I["rho"]), col(I["rho0"]), col(I["Sp"]), col(I["Su"]), col(I["V"]), col(I["psi"]), col(I["psi0"]), col(I["bpsi"])


def literal_bounds(L, I, phiBD, phiCorr, conv=float):
    """-> psiMaxn, psiMinn (transformed), sumPhip, mSumPhim; phiBD / phiCorr pairs of lists in the number type"""
    own, nei, bnd = _cells(L)
    lo, up = L["lo"].tolist(), L["up"].tolist()
    rdt, rho, rho0, Sp, Su, V, psi, psi0, bpsi = _cell_fields(I, conv)
    gMax, gMin, vsmall = conv(I["psiMax"]), conv(I["psiMin"]), conv(VSMALL)
    (bd, bbd), (corr, bcorr) = phiBD, phiCorr
    out = [[], [], [], []]
    for c in range(L["n"]):
        hi, low, sumBD, sp, sm = gMin, gMax, conv(0.0), vsmall, vsmall
        for f in own[c]:
            hi = _max(hi, psi[up[f]]); low = _min(low, psi[up[f]])
            sumBD = sumBD + bd[f]
            if corr[f] > 0:
                sp = sp + corr[f]
            else:
                sm = sm - corr[f]
        for f in nei[c]:
            hi = _max(hi, psi[lo[f]]); low = _min(low, psi[lo[f]])
            sumBD = sumBD - bd[f]
            if corr[f] > 0:
                sm = sm + corr[f]
            else:
                sp = sp - corr[f]
        for i in bnd[c]:
            hi = _max(hi, bpsi[i]); low = _min(low, bpsi[i])
            sumBD = sumBD + bbd[i]
            if bcorr[i] > 0:
                sp = sp + bcorr[i]
            else:
                sm = sm - bcorr[i]
        hi = _min(hi, gMax); low = _max(low, gMin)
        coef = rdt[c] if rho is None else rho[c] * rdt[c]
        if Sp is not None:
            coef = coef - Sp[c]
        old = (rdt[c] if rho0 is None else rho0[c] * rdt[c]) * psi0[c]
        top = coef * hi
        if Su is not None:
            top = top - Su[c]
        top = V[c] * (top - old)
        bot = coef * low
        bot = -bot if Su is None else Su[c] - bot
        bot = V[c] * (bot + old)
        for k, v in enumerate((top + sumBD, bot - sumBD, sp, sm)):
            out[k].append(v)
    return out


def literal_iterate(L, work, phiBD, phiCorr, lam, conv=float):
    """one limiter iteration -> lambdap, lambdam, (lambda, blambda) new lists"""
    own, nei, bnd = _cells(L)
    lo, up, bc, kind = L["lo"].tolist(), L["up"].tolist(), boundary_cells(L).tolist(), face_kinds(L).tolist()
    maxn, minn, sumPhip, mSumPhim = work
    (bd, bbd), (corr, bcorr), (l, bl) = phiBD, phiCorr, lam
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
        elif kind[i] == COUPLED or (bbd[i] + bcorr[i]) > small * small:
            v = _min(v, lambdap[bc[i]] if bcorr[i] > 0 else lambdam[bc[i]])
        nbl.append(v)
    return lambdap, lambdam, (nl, nbl)


def literal_apply(phiBD, phiCorr, lam, return_corr):
    """-> (out, bout)"""
    return tuple([l * c if return_corr else b + l * c for b, c, l in zip(bd, corr, ll)] for bd, corr, ll in zip(phiBD, phiCorr, lam))


def literal_integrate(L, flux, zero=0.0):
    """surfaceIntegrate before the division by V: own +, losort -, boundary +"""
    own, nei, bnd = _cells(L)
    v, bv = flux
    out = []
    for c in range(L["n"]):
        s = zero
        for f in own[c]:
            s = s + v[f]
        for f in nei[c]:
            s = s - v[f]
        for i in bnd[c]:
            s = s + bv[i]
        out.append(s)
    return out


def literal_solve(L, I, flux, conv=float):
    rdt, rho, rho0, Sp, Su, V, _, psi0, _ = _cell_fields(I, conv)
    s = literal_integrate(L, flux, conv(0.0))
    out = []
    for c in range(L["n"]):
        num = (psi0[c] if rho0 is None else rho0[c] * psi0[c]) * rdt[c]
        if Su is not None:
            num = num + Su[c]
        num = num - s[c] / V[c]
        den = rdt[c] if rho is None else rho[c] * rdt[c]
        if Sp is not None:
            den = den - Sp[c]
        out.append(num / den)
    return out


def literal_limit(L, I, n_iter=3, return_corr=False, conv=float, force_lambda=None):
    """MULES::limit in the loops: -> dict(phiBD, phiCorr, work, steps=[(lambdap, lambdam, lambda)], out)"""
    phiBD, phiCorr, lam = literal_form(L, I, conv)
    work = literal_bounds(L, I, phiBD, phiCorr, conv)
    steps = []
    for _ in range(n_iter):
        lp, lm, lam = literal_iterate(L, work, phiBD, phiCorr, lam, conv)
        steps.append((lp, lm, lam))
    if force_lambda is not None:
        lam = tuple([conv(force_lambda)] * len(x) for x in lam)
    return dict(phiBD=phiBD, phiCorr=phiCorr, work=work, steps=steps, lam=lam, out=literal_apply(phiBD, phiCorr, lam, return_corr))


# ---- the same, vectorised ---------------------------------------------------------------------------------------------------------------
class Events:
    """every (cell, face) meeting of a mesh in the cell's order, grouped into rounds: round r holds each cell's r-th meeting, so one numpy
    statement per round folds a value into every cell in the reference's order"""

    def __init__(self, L):
        nf, bc = L["lo"].shape[0], boundary_cells(L)
        # all owner meetings in face order, all neighbour meetings in face order, the boundary in patch order: per cell that is own faces
        # ascending, losort faces, boundary faces by patch
        self.cell = np.concatenate([L["lo"].astype(np.int64), L["up"].astype(np.int64), bc])
        self.side = np.concatenate([np.zeros(nf, np.int64), np.ones(nf, np.int64), np.full(bc.shape[0], 2, np.int64)])
        self.face = np.concatenate([np.arange(nf), np.arange(nf), np.arange(bc.shape[0])])
        order = np.argsort(self.cell, kind="stable")
        start = np.searchsorted(self.cell[order], np.arange(L["n"]))
        rank = np.empty(order.shape[0], np.int64)
        rank[order] = np.arange(order.shape[0]) - start[self.cell[order]] if order.shape[0] else 0
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2 if rank.shape[0] else 1))
        self.rounds = [by_rank[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def per_side(self, own, nei, bnd):
        """an event array from a face array per side (each already indexed by face / boundary face)"""
        return np.concatenate([own, nei, bnd])

    def fold(self, acc, vals, op, mask=None):
        acc = acc.copy()
        for idx in self.rounds:
            if mask is not None:
                idx = idx[mask[idx]]
            c = self.cell[idx]
            acc[c] = op(acc[c], vals[idx])
        return acc


rmax = lambda a, b: np.where(a > b, a, b)
rmin = lambda a, b: np.where(a < b, a, b)
add = lambda a, b: a + b
sub = lambda a, b: a - b


def restate_form(L, I):
    psi, bpsi = I["psi"], I["bpsi"]
    (phi, bphi), (phiPsi, bphiPsi) = I["phi"], I["phiPsi"]
    P, N = psi[L["lo"]], psi[L["up"]]
    w = np.where(phi >= 0, 1.0, 0.0)
    bd = phi * (w * (P - N) + N)
    bw = np.where(bphi >= 0, 1.0, 0.0)
    face = np.where(face_kinds(L) == COUPLED, bw * psi[boundary_cells(L)] + (1.0 - bw) * bpsi, bpsi)
    bbd = bphi * face
    return (bd, bbd), (phiPsi - bd, bphiPsi - bbd), (np.ones(phi.shape[0]), np.ones(bphi.shape[0]))


def _rdt(I, n):
    return I["rdt"] if isinstance(I["rdt"], np.ndarray) else np.full(n, float(I["rdt"]))


def restate_bounds(L, I, phiBD, phiCorr, ev=None):
    ev = ev or Events(L)
    n, psi = L["n"], I["psi"]
    (bd, bbd), (corr, bcorr) = phiBD, phiCorr
    seen = ev.per_side(psi[L["up"]], psi[L["lo"]], I["bpsi"])          # the value across each meeting
    hi = ev.fold(np.full(n, float(I["psiMin"])), seen, rmax)
    low = ev.fold(np.full(n, float(I["psiMax"])), seen, rmin)
    sumBD = ev.fold(np.zeros(n), ev.per_side(bd, -bd, bbd), add)
    c = ev.per_side(corr, corr, bcorr)
    pos, nbr = c > 0.0, ev.side == 1
    sp = ev.fold(np.full(n, VSMALL), np.where(nbr, -c, c), add, mask=np.where(nbr, ~pos, pos))      # own/boundary: += corr; losort: -= corr
    sm = ev.fold(np.full(n, VSMALL), np.where(nbr, c, -c), add, mask=np.where(nbr, pos, ~pos))      # own/boundary: -= corr; losort: += corr
    hi, low = rmin(hi, float(I["psiMax"])), rmax(low, float(I["psiMin"]))
    rdt = _rdt(I, n)
    coef = rdt if I["rho"] is None else I["rho"] * rdt
    if I["Sp"] is not None:
        coef = coef - I["Sp"]
    old = (rdt if I["rho0"] is None else I["rho0"] * rdt) * I["psi0"]
    top = coef * hi
    if I["Su"] is not None:
        top = top - I["Su"]
    top = I["V"] * (top - old)
    bot = coef * low
    bot = -bot if I["Su"] is None else I["Su"] - bot
    bot = I["V"] * (bot + old)
    return [top + sumBD, bot - sumBD, sp, sm]


def restate_iterate(L, work, phiBD, phiCorr, lam, ev=None):
    ev = ev or Events(L)
    n = L["n"]
    maxn, minn, sumPhip, mSumPhim = work
    (bd, bbd), (corr, bcorr), (l, bl) = phiBD, phiCorr, lam
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
    nbl = np.where(kind == WEDGE, 0.0, np.where((kind == COUPLED) | ((bbd + bcorr) > SMALL * SMALL), cut, bl))
    return lambdap, lambdam, (nl, nbl)


def restate_apply(phiBD, phiCorr, lam, return_corr):
    return tuple(l * c if return_corr else b + l * c for b, c, l in zip(phiBD, phiCorr, lam))


def restate_solve(L, I, flux, ev=None):
    ev = ev or Events(L)
    n = L["n"]
    v, bv = flux
    s = ev.fold(np.zeros(n), ev.per_side(v, -v, bv), add)
    rdt = _rdt(I, n)
    num = (I["psi0"] if I["rho0"] is None else I["rho0"] * I["psi0"]) * rdt
    if I["Su"] is not None:
        num = num + I["Su"]
    num = num - s / I["V"]
    den = rdt if I["rho"] is None else I["rho"] * rdt
    if I["Sp"] is not None:
        den = den - I["Sp"]
    return num / den


def sync_min(blam, pairs):
    """syncFaceList(minOp) on one rank: the two sides of a cyclic pair take minOp(mine, theirs) = (mine < theirs) ? mine : theirs;
    pairs: [(slice a, slice b)] into the boundary array"""
    out = blam.copy()
    for a, b in pairs:
        out[a], out[b] = rmin(blam[a], blam[b]), rmin(blam[b], blam[a])
    return out


def restate_limit(L, I, n_iter=3, return_corr=False, given=None, pairs=(), ev=None):
    """MULES::limit (given None: the limit form from phi and phiPsi) or MULES::limiter followed by the apply (given = (phiBD, phiCorr, lambda),
    each a pair) -> dict(phiBD, phiCorr, work, steps=[(lambdap, lambdam, (lambda, blambda))], lam, out)"""
    ev = ev or Events(L)
    phiBD, phiCorr, lam = given if given is not None else restate_form(L, I)
    work = restate_bounds(L, I, phiBD, phiCorr, ev)
    steps = []
    for _ in range(n_iter):
        lp, lm, lam = restate_iterate(L, work, phiBD, phiCorr, lam, ev)
        lam = (lam[0], sync_min(lam[1], pairs))
        steps.append((lp, lm, lam))
    return dict(phiBD=phiBD, phiCorr=phiCorr, work=work, steps=steps, lam=lam, out=restate_apply(phiBD, phiCorr, lam, return_corr))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def plain_patches(L, wedge_patch=None):
    """the mesh with every coupled patch declared `other` (the conveniences refuse coupled patches) and, optionally, one wedge patch"""
    kinds = [0 if k == 1 else k for k in L["kinds"]]
    wedge = [p == wedge_patch for p in range(len(kinds))]
    return dict(L, kinds=kinds, wedge=wedge)


def make_inputs(syn, L, seed, lts=False, rho=False, sp=False, su=False, bounds=(0.0, 1.0)):
    """psi uniform in [0, 1] with a quarter of the cells exactly 0 and a quarter exactly 1, V in [0.5, 1.5], rDeltaT = 1 (lts: per cell in
    [0.8, 1.2]), phi uniform in +-0.75 with every seventh face exactly 0, the high-order flux the central flux plus noise of +-0.0375.  Where phi
    is 0 the high-order flux is +0.0 and -0.0 in turn, so phiCorr holds both zeros.  A numpy prototype of the limiter found this scale: a third
    of the noise left iteration 3 changing nothing"""
    u = syn.splitmix_uniform
    n, nf, bc = L["n"], L["lo"].shape[0], boundary_cells(L)
    nb = bc.shape[0]
    psi = u(seed, n)
    pick = u(seed + 1, n)
    psi[pick < 0.25] = 0.0
    psi[pick > 0.75] = 1.0
    psi0 = psi.copy()
    phi = 1.5 * (u(seed + 2, nf) - 0.5)
    phi[::7] = 0.0
    phiPsi = phi * (0.5 * (psi[L["lo"]] + psi[L["up"]])) + 0.075 * (u(seed + 3, nf) - 0.5)
    phiPsi[::7] = 0.0
    phiPsi[7::14] = -0.0
    bpsi = u(seed + 4, nb)
    bphi = 1.5 * (u(seed + 5, nb) - 0.5)
    bphi[3::7] = 0.0
    bphiPsi = bphi * bpsi + 0.075 * (u(seed + 6, nb) - 0.5)
    bphiPsi[3::7] = 0.0
    bphiPsi[3::14] = -0.0
    return dict(psi=psi, psi0=psi0, V=0.5 + u(seed + 7, n), rdt=(0.8 + 0.4 * u(seed + 8, n)) if lts else 1.0,
                rho=(0.5 + u(seed + 9, n)) if rho else None, rho0=(0.5 + u(seed + 10, n)) if rho else None,
                Sp=(-0.2 * u(seed + 11, n)) if sp else None, Su=(0.2 * (u(seed + 12, n) - 0.5)) if su else None,
                bpsi=bpsi, psiMax=bounds[1], psiMin=bounds[0], phi=(phi, bphi), phiPsi=(phiPsi, bphiPsi))


VARIANTS = {                                                    # name -> make_inputs keywords
    "plain": dict(),
    "lts": dict(lts=True),
    "rho_sp_su": dict(rho=True, sp=True, su=True),
    "lts_rho_su": dict(lts=True, rho=True, su=True),
    "sp": dict(sp=True),
    "narrow": dict(bounds=(0.2, 0.8)),
}


def cyclic_pair(L):
    """the first two patches of equal size declared a cyclic pair (coupled), every other coupled patch `other` -> (mesh, (slice a, slice b))"""
    sizes = [fc.shape[0] for fc in L["fcs"]]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    a, b = next((p, q) for p in range(len(sizes)) for q in range(p + 1, len(sizes)) if sizes[p] == sizes[q] and sizes[p] > 0)
    kinds = [1 if p in (a, b) else (0 if k == 1 else k) for p, k in enumerate(L["kinds"])]
    return dict(L, kinds=kinds, wedge=None), (slice(offs[a], offs[a + 1]), slice(offs[b], offs[b + 1])), (a, b)


def pair_inputs(L, I, sl):
    """the inputs made consistent across a cyclic pair: psiPf is the other side's cell value, the fluxes are equal and opposite"""
    a, b = sl
    bc = boundary_cells(L)
    I = dict(I, bpsi=I["bpsi"].copy(), phi=(I["phi"][0], I["phi"][1].copy()), phiPsi=(I["phiPsi"][0], I["phiPsi"][1].copy()))
    I["bpsi"][a], I["bpsi"][b] = I["psi"][bc[b]], I["psi"][bc[a]]
    for key in ("phi", "phiPsi"):
        I[key][1][b] = -I[key][1][a]
    return I


# ---- the channel demonstration -----------------------------------------------------------------------------------------------------------
def channel(nx=24):
    """nx x 1 x 1: an inlet patch on cell 0 (fixesValue, psi = 0) and an outflow patch on the last cell (zeroGradient)"""
    lo = np.arange(nx - 1, dtype=np.int32)
    return dict(n=nx, lo=lo, up=lo + 1, fcs=[np.array([0], np.int32), np.array([nx - 1], np.int32)], kinds=[2, 0], wedge=None)


def channel_inputs(L, psi, courant=0.4):
    """unit cells, rDeltaT = 1, uniform phi = courant; the high-order flux is the central one; inlet value 0, outlet value the last cell's"""
    n, nf = L["n"], L["lo"].shape[0]
    phi = np.full(nf, courant)
    bphi = np.array([-courant, courant])
    bpsi = np.array([0.0, psi[-1]])
    return dict(psi=psi, psi0=psi.copy(), V=np.ones(n), rdt=1.0, rho=None, rho0=None, Sp=None, Su=None, bpsi=bpsi, psiMax=1.0, psiMin=0.0,
                phi=(phi, bphi), phiPsi=(phi * (0.5 * (psi[L["lo"]] + psi[L["up"]])), bphi * bpsi))


def channel_step_field(nx=24):
    psi = np.zeros(nx)
    psi[3:11] = 1.0
    return psi


def channel_run(steps=30, nx=24, limited=True):
    """-> [psi after each step]"""
    L = channel(nx)
    ev = Events(L)
    psi, out = channel_step_field(nx), []
    for _ in range(steps):
        I = channel_inputs(L, psi)
        flux = restate_limit(L, I, 3, False, ev=ev)["out"] if limited else I["phiPsi"]
        psi = restate_solve(L, I, flux, ev)
        out.append(psi)
    return out
