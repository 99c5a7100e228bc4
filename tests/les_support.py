"""The LES block restated twice (simpleFilter.C:64-125; cubeRootVolDelta.C:42-76; Smagorinsky.H:119, Smagorinsky.C:47; oneEqEddy.C:48, :104-113;
dynOneEqEddy.C:45-100, :136, :151-152): literal loops over Python floats with an explicit fma, and vectorised numpy.  The kernels of
csrc/les.inc are compared with the vectorised form bit for bit; a CPU test shows that the two forms agree and that the inputs reach every
branch.

Meshes are turbulence_support.mesh's; boundary face fields are patch-ordered; a symmetric tensor is six arrays xx, xy, xz, yy, yz, zz.  Rounding:
every operator on its own; fma in the interpolate of the filter (mi_face_interpolate's rule), in magSqr of a vector (3.5a), in magSqr of a
symmetric tensor (3.5o) and in the double inner product; dev has none.  max(a, b) = (a > b) ? a : b."""
import math

import numpy as np

from interface_support import div, fma, fma_v
from turbulence_support import _rows, bound_cell, boundary_cells, rmax, rmax_v

SMALL, VSMALL = 1e-15, 1e-300
THIRD = 1.0 / 3.0
DEFAULTS = (0.094, 1.048)
U0 = (0.3, 0.7, -0.2)                       # the velocity of the quiet region: no component a dyadic number
G0 = (3.1, -1.7, 0.9, 2.3, -4.1, 0.7, -0.3, 1.9, 1.3)   # the velocity gradient of the flat region


def sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def quiet_region(L, rings=3):
    """a cell with internal faces and every cell within `rings` faces of it -> (the cell, the region as a mask)"""
    c0, _ = bound_cell(L)
    if L["name"] in ("box", "big"):
        c0 = 0                                                      # a corner: the region stays a small part of the box
    lo, up = L["lo"], L["up"]
    m = np.zeros(L["n"], dtype=bool)
    m[c0] = True
    for _ in range(rings):
        grow = m.copy()
        grow[up[m[lo]]] = True; grow[lo[m[up]]] = True
        m = grow
    return c0, m


def flat_region(L, quiet):
    """a second region, apart from the quiet one: a cell and every cell within three faces of it (two where three do not fit) -> (the cell,
    the mask), or (-1, nothing) where neither fits (edge_257: 184 of its 257 cells are quiet)"""
    lo, up = L["lo"], L["up"]
    for rings in (3, 2):
        for c1 in up[::-7].tolist():
            m = np.zeros(L["n"], dtype=bool)
            m[c1] = True
            for _ in range(rings):
                grow = m.copy()
                grow[up[m[lo]]] = True; grow[lo[m[up]]] = True
                m = grow
            if not np.any(m & quiet):
                return c1, m
    return -1, np.zeros(L["n"], dtype=bool)


def inputs(syn, L, seed):
    """everything the entries read.  U and gradU seeded, but constant (U0) and zero in the quiet region, boundary values included: there KK is
    zero up to rounding (clipped by SMALL, and of either sign without the clip), D vanishes, and three filter levels further in, at the region's
    centre, f_mmmm is exactly 0.  In the flat region gradU is the constant G0 (boundary values included), U stays seeded: there
    fMagSqrD - magSqr(fD), a variance everywhere else and hence not negative, is rounding noise of either sign, so that ce_num goes negative.
    The boundary's delta is SMALL (LESdelta.C:53).  lm / mmmm / num / den: the inputs of mi_les_dyn_coeffs alone,
    of either sign."""
    u = syn.splitmix_uniform
    n, nf = L["n"], L["lo"].shape[0]
    bc = boundary_cells(L)
    nb = bc.shape[0]
    c0, quiet = quiet_region(L)
    bquiet = quiet[bc] if nb else np.zeros(0, dtype=bool)
    c1, flat = flat_region(L, quiet)
    bflat = flat[bc] if nb else np.zeros(0, dtype=bool)
    U = [np.where(quiet, U0[d], u(seed + d, n) - 0.5) for d in range(3)]
    bU = [np.where(bquiet, U0[d], u(seed + 3 + d, nb) - 0.5) for d in range(3)]
    grad = [np.where(quiet, 0.0, np.where(flat, G0[i], 20.0 * (u(seed + 6 + i, n) - 0.5))) for i in range(9)]
    bgrad = [np.where(bquiet, 0.0, np.where(bflat, G0[i], 20.0 * (u(seed + 15 + i, nb) - 0.5))) for i in range(9)]
    V = 1e-3 * (0.5 + u(seed + 24, n))
    k = 0.01 + u(seed + 25, n)
    nusgs = 1e-4 + 1e-2 * u(seed + 26, n)
    nu_f = 1e-5 * (0.5 + u(seed + 27, n))
    bnueff = 1e-4 + 1e-2 * u(seed + 28, nb)
    lam = 0.3 + 0.4 * u(seed + 30, nf)
    magSf = 0.5 + u(seed + 31, nf)
    bms = 0.5 + u(seed + 32, nb)
    vf = [u(seed + 40 + i, n) - 0.5 for i in range(9)]
    bvf = [u(seed + 50 + i, nb) - 0.5 for i in range(9)]
    ck_f, ce_f = 0.05 + 0.1 * u(seed + 60, n), 0.5 + u(seed + 61, n)
    lm, mmmm = u(seed + 62, n) - 0.5, u(seed + 63, n)
    num, den = u(seed + 64, n) - 0.4, 0.1 + u(seed + 65, n)
    mmmm[3::11] = 0.0
    lm[3::22] = 0.0
    return dict(c0=c0, quiet=quiet, c1=c1, flat=flat, U=U, bU=bU, grad=grad, bgrad=bgrad, V=V, k=k, nusgs=nusgs, nu=1.3e-5, nu_f=nu_f, bnueff=bnueff, lam=lam, magSf=magSf,
                bms=bms, vf=vf, bvf=bvf, ck_f=ck_f, ce_f=ce_f, lm=lm, mmmm=mmmm, num=num, den=den, delta_coeff=1.0, thickness=0.05)


# ---- literal loops -------------------------------------------------------------------------------------------------------------------------------
def l_symm(g):
    return [g[0], 0.5 * (g[1] + g[3]), 0.5 * (g[2] + g[6]), g[4], 0.5 * (g[5] + g[7]), g[8]]


def l_dev(d):
    t = THIRD * ((d[0] + d[3]) + d[5])
    return [d[0] - t, d[1], d[2], d[3] - t, d[4], d[5] - t]


def l_magsqr_st(d):
    s = fma(d[0], d[0], 2.0 * (d[1] * d[1]))
    s = fma(2.0, d[2] * d[2], s)
    s = fma(d[3], d[3], s)
    s = fma(2.0, d[4] * d[4], s)
    return fma(d[5], d[5], s)


def l_ddot(a, b):
    s = fma(a[0], b[0], (2.0 * a[1]) * b[1])
    s = fma(2.0 * a[2], b[2], s)
    s = fma(a[3], b[3], s)
    s = fma(2.0 * a[4], b[4], s)
    return fma(a[5], b[5], s)


def l_magsqr_v(v):
    return fma(v[2], v[2], fma(v[0], v[0], v[1] * v[1]))


def _cells(*arrays):
    """per cell the tuple of its values: a list of arrays gives one tuple of components"""
    return zip(*[list(zip(*[x.tolist() for x in a])) if isinstance(a, (list, tuple)) else a.tolist() for a in arrays])


def _stack(rows, widths):
    """rows of flat per-cell results -> arrays grouped by widths (1: an array, m: a list of m arrays)"""
    a = np.array(rows, dtype=np.float64).reshape(len(rows), sum(widths))
    out, j = [], 0
    for w in widths:
        out.append(np.ascontiguousarray(a[:, j]) if w == 1 else [np.ascontiguousarray(a[:, j + i]) for i in range(w)])
        j += w
    return out


def literal_filter(L, lam, magSf, bms, vf, bface):
    own, nei, bnd = _rows(L)
    lo, up = L["lo"].tolist(), L["up"].tolist()
    m, b, w = magSf.tolist(), bms.tolist(), lam.tolist()
    out = []
    for x, bx in zip([v.tolist() for v in vf], [v.tolist() for v in bface]):
        col = []
        for c in range(L["n"]):
            s = t = 0.0
            for f in own[c] + nei[c]:
                P, N = x[lo[f]], x[up[f]]
                s = s + m[f] * fma(w[f], P - N, N); t = t + m[f]
            for i in bnd[c]:
                s = s + b[i] * bx[i]; t = t + b[i]
            col.append(div(s, t))
        out.append(np.array(col))
    return out


def literal_delta(coeff, thickness, V, root=None):
    """root: the device's values of pow to continue from"""
    r = [(math.sqrt(v / thickness) if thickness > 0 else math.pow(v, THIRD)) for v in V.tolist()] if root is None else root.tolist()
    return np.array([coeff * p for p in r]), np.array(r)


def literal_smagorinsky(ck, ce, delta, grad):
    c0 = (2.0 * ck) / ce
    rows = []
    for d, g in _cells(delta, grad):
        k = (c0 * (d * d)) * l_magsqr_st(l_dev(l_symm(g)))
        rows.append([(ck * d) * sqrt(k), k])
    return _stack(rows, [1, 1])


def literal_k_terms(ce, nusgs, grad, k, delta, nu):
    n = k.shape[0]
    cev = ce if isinstance(ce, np.ndarray) else np.full(n, ce)
    nuv = nu if isinstance(nu, np.ndarray) else np.full(n, nu)
    rows = []
    for t, g, kk, d, e, v in _cells(nusgs, grad, k, delta, cev, nuv):
        rows.append([(2.0 * t) * l_magsqr_st(l_symm(g)), div(e * sqrt(kk), d), t + v])
    return _stack(rows, [1, 1, 1])


def literal_nusgs(ck, k, delta):
    ckv = ck if isinstance(ck, np.ndarray) else np.full(k.shape[0], ck)
    return np.array([(c * sqrt(kk)) * d for c, kk, d in _cells(ckv, k, delta)])


def literal_moments(U, grad):
    rows = []
    for u, g in _cells(U, grad):
        D = l_symm(g)
        rows.append([u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2], l_magsqr_v(u)] + D + [l_magsqr_st(D)])
    return _stack(rows, [6, 1, 6, 1])


def literal_level1(clip, delta, nueff, fU, fS, fMU, fD, fMD, p15=None):
    """-> KK, LL, MM, ce_num, ce_den, pow(KK, 1.5); p15: the device's values of pow to continue from"""
    rows = []
    pw = [None] * delta.shape[0] if p15 is None else p15.tolist()
    for (d, ne, u, s, mu, D, md), p in zip(_cells(delta, nueff, fU, fS, fMU, fD, fMD), pw):
        KK = 0.5 * (mu - l_magsqr_v(u))
        if clip:
            KK = rmax(KK, SMALL)
        a = [s[0] - u[0] * u[0], s[1] - u[0] * u[1], s[2] - u[0] * u[2], s[3] - u[1] * u[1], s[4] - u[1] * u[2], s[5] - u[2] * u[2]]
        m = (-2.0 * d) * sqrt(KK)
        if p is None:
            p = math.pow(KK, 1.5) if KK >= 0 else math.nan
        rows.append([KK] + l_dev(a) + [m * x for x in D] + [ne * (md - l_magsqr_st(D)), div(p, 2.0 * d), p])
    return _stack(rows, [1, 6, 6, 1, 1, 1])


def literal_level2(fLL, fMM):
    return _stack([[0.5 * l_ddot(a, b), l_magsqr_st(b)] for a, b in _cells(fLL, fMM)], [1, 1])


def literal_coeffs(f_lm, f_mmmm, f_num, f_den):
    rows = []
    for a, b, x, y in _cells(f_lm, f_mmmm, f_num, f_den):
        c, e = div(a, b + VSMALL), div(x, y)
        rows.append([0.5 * (abs(c) + c), 0.5 * (abs(e) + e)])
    return _stack(rows, [1, 1])


# ---- the same, vectorised ------------------------------------------------------------------------------------------------------------------------
def symm(g):
    return [g[0], 0.5 * (g[1] + g[3]), 0.5 * (g[2] + g[6]), g[4], 0.5 * (g[5] + g[7]), g[8]]


def dev(d, contracted=False):
    """contracted: fma(-(1/3), tr, xx) -- the alternative the CPU test looks at"""
    tr = (d[0] + d[3]) + d[5]
    if contracted:
        return [fma_v(-THIRD, tr, d[0]), d[1], d[2], fma_v(-THIRD, tr, d[3]), d[4], fma_v(-THIRD, tr, d[5])]
    t = THIRD * tr
    return [d[0] - t, d[1], d[2], d[3] - t, d[4], d[5] - t]


def magsqr_st(d, contracted=True):
    if not contracted:
        return d[0] * d[0] + 2.0 * (d[1] * d[1]) + 2.0 * (d[2] * d[2]) + d[3] * d[3] + 2.0 * (d[4] * d[4]) + d[5] * d[5]
    s = fma_v(d[0], d[0], 2.0 * (d[1] * d[1]))
    s = fma_v(2.0, d[2] * d[2], s)
    s = fma_v(d[3], d[3], s)
    s = fma_v(2.0, d[4] * d[4], s)
    return fma_v(d[5], d[5], s)


def ddot(a, b, contracted=True):
    if not contracted:
        return a[0] * b[0] + (2.0 * a[1]) * b[1] + (2.0 * a[2]) * b[2] + a[3] * b[3] + (2.0 * a[4]) * b[4] + a[5] * b[5]
    s = fma_v(a[0], b[0], (2.0 * a[1]) * b[1])
    s = fma_v(2.0 * a[2], b[2], s)
    s = fma_v(a[3], b[3], s)
    s = fma_v(2.0 * a[4], b[4], s)
    return fma_v(a[5], b[5], s)


def magsqr_v(v, contracted=True):
    if not contracted:
        return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    return fma_v(v[2], v[2], fma_v(v[0], v[0], v[1] * v[1]))


def surface_sum_magsf(L, magSf, bms):
    t = np.zeros(L["n"])
    np.add.at(t, L["lo"], magSf); np.add.at(t, L["up"], magSf); np.add.at(t, boundary_cells(L), bms)
    return t


def restate_filter(L, lam, magSf, bms, vf, bface, fused=False, reciprocal=False, plain_interpolate=False):
    """ufunc.at is unbuffered and walks its indices in order: own faces ascending, then the neighbour side in face order (losort order), then
    the boundary faces.  fused: magSf*i contracted into the sum; reciprocal: s*(1/sum); plain_interpolate: w*P + (1 - w)*N -- the alternatives
    the CPU test shows to be visible"""
    lo, up, bc = L["lo"], L["up"], boundary_cells(L)
    t = surface_sum_magsf(L, magSf, bms)
    out = []
    for x, bx in zip(vf, bface):
        i = lam * x[lo] + (1.0 - lam) * x[up] if plain_interpolate else fma_v(lam, x[lo] - x[up], x[up])
        if fused:
            s = [0.0] * L["n"]
            for idx, a, b in ((lo, magSf, i), (up, magSf, i), (bc, bms, bx)):
                for c, p, q in zip(idx.tolist(), a.tolist(), b.tolist()):
                    s[c] = fma(p, q, s[c])
            s = np.array(s)
        else:
            s = np.zeros(L["n"])
            np.add.at(s, lo, magSf * i); np.add.at(s, up, magSf * i); np.add.at(s, bc, bms * bx)
        with np.errstate(all="ignore"):
            out.append(s * (1.0 / t) if reciprocal else s / t)
    return out


def restate_delta(coeff, thickness, V, root=None):
    with np.errstate(all="ignore"):
        r = (np.sqrt(V / thickness) if thickness > 0 else np.power(V, THIRD)) if root is None else root
    return coeff * r, r


def restate_smagorinsky(ck, ce, delta, grad, dev_contracted=False):
    c0 = (2.0 * ck) / ce
    with np.errstate(all="ignore"):
        k = (c0 * (delta * delta)) * magsqr_st(dev(symm(grad), contracted=dev_contracted))
        return (ck * delta) * np.sqrt(k), k


def restate_k_terms(ce, nusgs, grad, k, delta, nu):
    with np.errstate(all="ignore"):
        return (2.0 * nusgs) * magsqr_st(symm(grad)), (ce * np.sqrt(k)) / delta, nusgs + nu


def restate_nusgs(ck, k, delta, regroup=False):
    """regroup: ck*(delta*sqrt(k)), the alternative the CPU test shows to be visible"""
    with np.errstate(all="ignore"):
        return ck * (delta * np.sqrt(k)) if regroup else (ck * np.sqrt(k)) * delta


def restate_moments(U, grad, contracted=True):
    D = symm(grad)
    return [U[0] * U[0], U[0] * U[1], U[0] * U[2], U[1] * U[1], U[1] * U[2], U[2] * U[2]], magsqr_v(U, contracted), D, magsqr_st(D)


def restate_level1(clip, delta, nueff, fU, fS, fMU, fD, fMD, p15=None, magsqr_contracted=True, dev_contracted=False, fused_difference=False):
    """fused_difference: fSqrU_ij - fU_i*fU_j as one fma -- what a field algebra with expression templates could give, not the reference's"""
    with np.errstate(all="ignore"):
        KK = 0.5 * (fMU - magsqr_v(fU, magsqr_contracted))
        if clip:
            KK = rmax_v(KK, SMALL)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        if fused_difference:
            a = [fma_v(-fU[i], fU[j], fS[q]) for q, (i, j) in enumerate(pairs)]
        else:
            a = [fS[q] - fU[i] * fU[j] for q, (i, j) in enumerate(pairs)]
        m = (-2.0 * delta) * np.sqrt(KK)
        p = np.power(KK, 1.5) if p15 is None else p15
        return KK, dev(a, contracted=dev_contracted), [m * x for x in fD], nueff * (fMD - magsqr_st(fD)), p / (2.0 * delta), p


def restate_level2(fLL, fMM, contracted=True):
    return 0.5 * ddot(fLL, fMM, contracted), magsqr_st(fMM)


def restate_coeffs(f_lm, f_mmmm, f_num, f_den):
    with np.errstate(all="ignore"):
        c, e = f_lm / (f_mmmm + VSMALL), f_num / f_den
        return 0.5 * (np.abs(c) + c), 0.5 * (np.abs(e) + e)


# ---- the dynamic procedure end to end --------------------------------------------------------------------------------------------------------------
def restate_chain(L, I, delta, nueff, clip, p15=None, bp15=None, flt=restate_filter, maps=None):
    """dynOneEqEddy.C:56-100 with :136 / :151-152 on the cells AND on the patch-ordered boundary arrays (delta_b = SMALL, the per-element maps run
    over the boundary values): three filter levels, four maps -> every intermediate.  p15 / bp15: the device's pow values to continue from.
    flt / maps: the forms to use (the literal ones in the CPU test)"""
    M = maps or dict(moments=restate_moments, level1=restate_level1, level2=restate_level2, coeffs=restate_coeffs)
    nb = I["bms"].shape[0]
    F = lambda vf, bvf: flt(L, I["lam"], I["magSf"], I["bms"], vf, bvf)
    flat = lambda *xs: [a for x in xs for a in (x if isinstance(x, list) else [x])]
    bdelta = np.full(nb, SMALL)
    sq, mu, D, md = M["moments"](I["U"], I["grad"])
    bsq, bmu, bD, bmd = M["moments"](I["bU"], I["bgrad"])
    f1 = F(flat(I["U"], sq, mu, D, md), flat(I["bU"], bsq, bmu, bD, bmd))
    fU, fS, fMU, fD, fMD = f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16]
    bc = boundary_cells(L)
    zg = lambda xs: [x[bc] for x in xs] if isinstance(xs, list) else xs[bc]          # zero-gradient boundary values of a filtered field
    KK, LL, MM, num, den, p = M["level1"](clip, delta, nueff, fU, fS, fMU, fD, fMD, p15=p15)
    bKK, bLL, bMM, bnum, bden, bp = M["level1"](clip, bdelta, I["bnueff"], zg(fU), zg(fS), zg(fMU), zg(fD), zg(fMD), p15=bp15)
    f2 = F(flat(LL, MM, num, den), flat(bLL, bMM, bnum, bden))
    fLL, fMM, fnum, fden = f2[0:6], f2[6:12], f2[12], f2[13]
    lm, mmmm = M["level2"](fLL, fMM)
    blm, bmmmm = M["level2"](zg(fLL), zg(fMM))
    flm, fmmmm = F([lm, mmmm], [blm, bmmmm])
    ck, ce = M["coeffs"](flm, fmmmm, fnum, fden)
    return dict(sq=sq, mu=mu, D=D, md=md, bsq=bsq, bmu=bmu, bD=bD, bmd=bmd, f1=f1, KK=KK, LL=LL, MM=MM, num=num, den=den, p=p, bKK=bKK, bLL=bLL, bMM=bMM,
                bnum=bnum, bden=bden, bp=bp, f2=f2, lm=lm, mmmm=mmmm, blm=blm, bmmmm=bmmmm, flm=flm, fmmmm=fmmmm, ck=ck, ce=ce)


# ---- channel_walk: the constructor and three correct() steps of each model on turbulence_support.channel -------------------------------------------
MODELS = ("Smagorinsky", "oneEqEddy", "dynOneEqEddy")


def channel_flow(M, step):
    """the velocity and its gradient at a step (step -1: the constructor's): the channel's seeded fields scaled by 1 + step/4, so that no two
    steps see the same flow; boundary values: zero on the walls, the cell's elsewhere; the gradient's are the cell's"""
    from turbulence_support import wall_mask
    bc, wall = boundary_cells(M["L"]), wall_mask(M["L"])
    f = 1.0 + 0.25 * (step + 1)
    U = [f * x for x in M["U"]]
    grad = [f * x for x in M["grad"]]
    return dict(U=U, bU=[np.where(wall, 0.0, x[bc]) for x in U], grad=grad, bgrad=[x[bc] for x in grad])


def restate_les_constructor(model, M, S, X):
    """Smagorinsky.C:76, oneEqEddy.C:90-92, dynOneEqEddy.C:134-137 (bound(k, kMin) finds nothing to do on the channel's k) -> the state.
    X: delta (from the device's pow) and, for the dynamic model, the device's pow values of the unclipped chain"""
    bc = boundary_cells(M["L"])
    ck, ce = DEFAULTS
    F = channel_flow(M, -1)
    out = {}
    if model == "Smagorinsky":
        nus, k = restate_smagorinsky(ck, ce, X["delta"], F["grad"])
        S = dict(S, k=k, bk=k[bc])
    elif model == "oneEqEddy":
        nus = restate_nusgs(ck, S["k"], X["delta"])
    else:
        I = dict(F, lam=M["lam"], magSf=M["magSf"], bms=M["bms"], bnueff=np.full(M["nb"], M["nu"]))
        C = restate_chain(M["L"], I, X["delta"], np.full(M["n"], M["nu"]), 0, p15=X["p"], bp15=X["bp"])
        out.update({"dyn_" + key: v for key, v in C.items()})
        nus = restate_nusgs(C["ck"], S["k"], X["delta"])
    out.update(nusgs=nus, bnusgs=nus[bc])
    return out, dict(S, nusgs=nus, bnusgs=nus[bc])


def restate_les_correct(model, orc, M, S, X, step):
    """correct() of the model (Smagorinsky.C:84-89, oneEqEddy.C:100-122, dynOneEqEddy.C:145-172) from the state S (k, bk, nusgs, bnusgs) ->
    (every intermediate, the next state).  X: what the restatement continues from -- delta, the device's pow values of the chain and the
    solution of the engine's solver"""
    from turbulence_support import boundary_values, restate_bound_field, restate_equation
    bc, nu, delta = boundary_cells(M["L"]), M["nu"], X["delta"]
    ck, ce = DEFAULTS
    F = channel_flow(M, step)
    out = {}
    if model == "Smagorinsky":
        nus, k = restate_smagorinsky(ck, ce, delta, F["grad"])
        out.update(k_new=k, nusgs=nus, bnusgs=nus[bc])
        return out, dict(k=k, bk=k[bc], nusgs=nus, bnusgs=nus[bc])
    if model == "dynOneEqEddy":
        I = dict(F, lam=M["lam"], magSf=M["magSf"], bms=M["bms"], bnueff=S["bnusgs"] + nu)
        C = restate_chain(M["L"], I, delta, S["nusgs"] + nu, 1, p15=X["p"], bp15=X["bp"])
        out.update({"dyn_" + key: v for key, v in C.items()})
        ck, ce = C["ck"], C["ce"]
    G, sp, dk = restate_k_terms(ce, S["nusgs"], F["grad"], S["k"], delta, nu)
    out.update(G=G, sp=sp, dk=dk)
    e = restate_equation(orc, M, S["k"], S["k"], G, sp, dk, S["bnusgs"] + nu, M["k_in"], M["alpha_k"])
    out.update({"k_" + key: v for key, v in e.items()})
    k = X["k_solved"]
    k, bk, out["k_bounded"] = restate_bound_field(M, k, boundary_values(M, k, M["k_in"]), SMALL)
    nus = restate_nusgs(ck, k, delta)
    out.update(k_new=k, bk_new=bk, nusgs=nus, bnusgs=nus[bc])
    return out, dict(k=k, bk=bk, nusgs=nus, bnusgs=nus[bc])
