"""interFoam's interfaceProperties restated twice (interfaceProperties.C:58-159, :220-231): literal loops over Python floats with an
explicit fma, and vectorised numpy with the element-wise fma of cmules_support (fma_v).  The kernels of csrc/interface.inc are compared with
the vectorised form bit for bit; a CPU test shows that the two forms agree and that the inputs reach every branch.

A mesh here is a dict(n, lo, up, Sf: three face arrays, fcs: two patches' faceCells); boundary face fields are patch-ordered.  Rounding: every
operator on its own, fma where the kernels write one: the interpolate (mi_face_interpolate's rule), the dot product and the magSqr under mag
(the contraction of DESIGN 3.5a)."""
import math

import numpy as np

from assembly_support import shape_case
from cmules_support import fma as _fma_finite
from reconstruct_support import skewed_rc

TO_RAD = math.pi / 180.0                    # convertToRad as the reference forms it
MESHES = ("box", "edge_257", "isolated")    # the skewed 5 x 4 x 3 box, a 257-cell graph, cells and a whole block of cells without faces
B12_BOUND = 16 * 2.0 ** -52                 # the device's b1 and b2 against numpy, absolute: derived in test_the_contact_angle_form's docstring


def fma(a, b, c):
    """one rounding; a non-finite operand: a*b + c as the hardware gives it (NaN or infinity either way)"""
    if math.isfinite(a) and math.isfinite(b) and math.isfinite(c):
        return _fma_finite(a, b, c)
    return a * b + c


def fma_v(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.array([fma(x, y, z) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())]).reshape(a.shape)


def div(a, b):
    """IEEE division on floats: x/0 is an infinity or NaN, not an exception"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- meshes and inputs ---------------------------------------------------------------------------------------------------------------------
def mesh(pkg, name):
    syn = pkg.synthetic
    if name == "box":
        L = skewed_rc(syn)
        n, lo, up, Sf = L["n"], L["lo"], L["up"], L["Sf"]
    else:
        case = shape_case(pkg, name)
        n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
        Sf = [syn.splitmix_uniform(700 + d, lo.shape[0]) - 0.5 for d in range(3)]
    faced = (np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)) > 0
    p0 = np.arange(0, n, 3, dtype=np.int32)
    p1 = np.arange(1, n, 2, dtype=np.int32)[::-1]              # not sorted; shares cells with the first patch
    return dict(name=name, n=n, lo=lo, up=up, Sf=[np.ascontiguousarray(s) for s in Sf], fcs=[np.ascontiguousarray(p[faced[p]]) for p in (p0, p1)])


def boundary_cells(L):
    return np.concatenate(L["fcs"]).astype(np.int32)


def quiet_cell(L):
    """a cell with internal faces whose faces all carry a zero flux in inputs(): its own and its neighbours' gradients are zero"""
    lo, up = L["lo"], L["up"]
    c0 = int(lo[lo.shape[0] // 2])
    nb = np.unique(np.concatenate([up[lo == c0], lo[up == c0], [c0]]))
    return c0, nb


def inputs(syn, L, seed):
    """grad: three cell arrays, 30 % of the cells exactly zero, 20 % of the order of delta_n, the rest ordinary; lam in (0.3, 0.7); vol; bn: a
    boundary flux (zero on the quiet cell's faces); K of both signs; alpha with cells exactly at 0.01 and 0.99; dc, corr face arrays"""
    u = syn.splitmix_uniform
    n, nf = L["n"], L["lo"].shape[0]
    delta_n = 1e-8 / 0.02 ** (1.0 / 3.0)
    pick = u(seed, n)
    grad = []
    for d in range(3):
        g = 20.0 * (u(seed + 1 + d, n) - 0.5)
        tiny = (pick >= 0.3) & (pick < 0.5)
        g[tiny] = 2.0 * delta_n * (u(seed + 4 + d, n)[tiny] - 0.5)
        g[pick < 0.3] = 0.0
        grad.append(g)
    c0, nb = quiet_cell(L)
    for g in grad:
        g[nb] = 0.0
    bc = boundary_cells(L)
    bn = u(seed + 8, bc.shape[0]) - 0.5
    bn[bc == c0] = 0.0
    alpha = u(seed + 9, n)
    alpha[::7] = 0.01
    alpha[3::7] = 0.99
    alpha[5::11] = 0.0
    alpha[6::11] = 1.0
    return dict(delta_n=delta_n, grad=grad, lam=0.3 + 0.4 * u(seed + 10, nf), vol=0.5 + u(seed + 11, n), bn=bn, K=40.0 * (u(seed + 12, n) - 0.5),
                alpha=alpha, dc=0.5 + u(seed + 13, nf), corr=u(seed + 14, nf) - 0.5, sigma=0.07)


# ---- literal loops ----------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return fma(a[2], b[2], fma(a[0], b[0], a[1] * b[1]))


def mag3(a):
    s = dot3(a, a)
    return math.sqrt(s) if s >= 0 else float("nan")


def unit3(g, delta_n):
    """steps 2-4 -> n, mag(g)"""
    m = mag3(g)
    d = m + delta_n
    return [div(x, d) for x in g], m


def literal_nhatf(lo, up, lam, Sf, grad, delta_n):
    """-> nHatf, [nx, ny, nz] on the internal faces"""
    out, nv = [], []
    G = [g.tolist() for g in grad]
    S = [s.tolist() for s in Sf]
    for f, (P, N, w) in enumerate(zip(lo.tolist(), up.tolist(), lam.tolist())):
        g = [fma(w, G[k][P] - G[k][N], G[k][N]) for k in range(3)]
        n, _ = unit3(g, delta_n)
        nv.append(n)
        out.append(dot3(n, [S[k][f] for k in range(3)]))
    return np.array(out), [np.array([v[k] for v in nv]) for k in range(3)]


def literal_patch_nhatf(g, Sf, delta_n, magSf=None, theta_deg=None, b12=None):
    """one patch from the face gradient g (three arrays) -> nHatf, [nx, ny, nz], gradient, a12, (b1, b2).  theta_deg: correctContactAngle
    :83-111; b12 given: the cos / acos results to continue from (the device's own), otherwise math.cos / math.acos"""
    out, nv, grd, a12s, b1s, b2s = [], [], [], [], [], []
    for i in range(g[0].shape[0]):
        gi, s = [float(g[k][i]) for k in range(3)], [float(Sf[k][i]) for k in range(3)]
        n, m = unit3(gi, delta_n)
        if theta_deg is not None:
            theta = TO_RAD * float(theta_deg[i])
            nf = [div(x, float(magSf[i])) for x in s]
            a12 = dot3(n, nf)
            if b12 is None:
                b1 = math.cos(theta)
                b2 = math.cos(math.acos(a12) - theta) if abs(a12) <= 1 else float("nan")
            else:
                b1, b2 = float(b12[0][i]), float(b12[1][i])
            det = 1.0 - a12 * a12
            a, b = div(b1 - a12 * b2, det), div(b2 - a12 * b1, det)
            n = [a * nf[k] + b * n[k] for k in range(3)]
            d = mag3(n) + delta_n
            n = [div(x, d) for x in n]
            grd.append(dot3(nf, n) * m); a12s.append(a12); b1s.append(b1); b2s.append(b2)
        nv.append(n)
        out.append(dot3(n, s))
    return np.array(out), [np.array([v[k] for v in nv]) for k in range(3)], np.array(grd), np.array(a12s), (np.array(b1s), np.array(b2s))


def literal_curvature(L, nhatf, bn, vol):
    """surfaceIntegrate's order per cell: own faces ascending, losort faces, boundary faces patch by patch; /V; unary minus"""
    n, lo, up = L["n"], L["lo"].tolist(), L["up"].tolist()
    own, nei, bnd = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    for f, (P, N) in enumerate(zip(lo, up)):
        own[P].append(f); nei[N].append(f)
    for i, c in enumerate(boundary_cells(L).tolist()):
        bnd[c].append(i)
    v, b, V = nhatf.tolist(), bn.tolist(), vol.tolist()
    out = []
    for c in range(n):
        s = 0.0
        for f in own[c]:
            s = s + v[f]
        for f in nei[c]:
            s = s - v[f]
        for i in bnd[c]:
            s = s + b[i]
        out.append(-(s / V[c]))
    return np.array(out)


def literal_force(sigma, lam, dc, KP, KN, aP, aN, corr=None, patch=False):
    out = []
    for i, (w, d, kp, kn, p, q) in enumerate(zip(lam.tolist(), dc.tolist(), KP.tolist(), KN.tolist(), aP.tolist(), aN.tolist())):
        sP, sN = sigma * kp, sigma * kn
        ip = w * sP + (1.0 - w) * sN if patch else fma(w, sP - sN, sN)
        sn = d * (q - p)
        if corr is not None:
            sn = sn + float(corr[i])
        out.append(ip * sn)
    return np.array(out)


def literal_near_interface(alpha):
    return np.array([(1.0 if x - 0.01 >= 0 else 0.0) * (1.0 if 0.99 - x >= 0 else 0.0) for x in alpha.tolist()])


# ---- the same, vectorised ------------------------------------------------------------------------------------------------------------------------
def dot3_v(a, b):
    with np.errstate(all="ignore"):
        return fma_v(a[2], b[2], fma_v(a[0], b[0], a[1] * b[1]))


def unit3_v(g, delta_n, contracted=True, reciprocal=False):
    """contracted False / reciprocal True: the alternatives the CPU test shows to be visible"""
    with np.errstate(all="ignore"):
        m = np.sqrt(dot3_v(g, g) if contracted else g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        d = m + delta_n
        if reciprocal:
            r = 1.0 / d
            return [x * r for x in g], m
        return [x / d for x in g], m


def face_gradient(lo, up, lam, grad):
    return [fma_v(lam, g[lo] - g[up], g[up]) for g in grad]


def coupled_gradient(w, gP, gN):
    """surfaceInterpolationScheme.C:361-366 per component, every operator rounded"""
    return [w * p + (1.0 - w) * q for p, q in zip(gP, gN)]


def restate_nhatf(lo, up, lam, Sf, grad, delta_n, contracted=True, reciprocal=False):
    """-> nHatf, [nx, ny, nz], mag(g)"""
    n, m = unit3_v(face_gradient(lo, up, lam, grad), delta_n, contracted, reciprocal)
    return dot3_v(n, Sf), n, m


def restate_patch_nhatf(g, Sf, delta_n, magSf=None, theta_deg=None, b12=None):
    """-> nHatf, [nx, ny, nz], gradient, a12, (b1, b2) as literal_patch_nhatf"""
    n, m = unit3_v(g, delta_n)
    grd = a12 = None
    if theta_deg is not None:
        with np.errstate(all="ignore"):
            theta = TO_RAD * theta_deg
            nf = [s / magSf for s in Sf]
            a12 = dot3_v(n, nf)
            b1, b2 = (np.cos(theta), np.cos(np.arccos(a12) - theta)) if b12 is None else b12
            det = 1.0 - a12 * a12
            a, b = (b1 - a12 * b2) / det, (b2 - a12 * b1) / det
            n = [a * nf[k] + b * n[k] for k in range(3)]
            d = np.sqrt(dot3_v(n, n)) + delta_n
            n = [x / d for x in n]
            grd = dot3_v(nf, n) * m
            b12 = (b1, b2)
    return dot3_v(n, Sf), n, grd, a12, b12


def restate_curvature(L, nhatf, bn, vol):
    """ufunc.at is unbuffered and walks its indices in order: all owner events in face order, all neighbour events in face order, then the
    boundary faces in patch order give every cell its own faces, its losort faces, its boundary faces, from +0.0"""
    s = np.zeros(L["n"])
    np.add.at(s, L["lo"], nhatf)
    np.subtract.at(s, L["up"], nhatf)
    np.add.at(s, boundary_cells(L), bn)
    return -(s / vol)


def restate_force(sigma, lam, dc, KP, KN, aP, aN, corr=None, patch=False, sigma_after=False):
    """sigma_after: sigma*interpolate(K), the alternative the CPU test shows to be visible"""
    if sigma_after:
        ip = sigma * (lam * KP + (1.0 - lam) * KN if patch else fma_v(lam, KP - KN, KN))
    else:
        sP, sN = sigma * KP, sigma * KN
        ip = lam * sP + (1.0 - lam) * sN if patch else fma_v(lam, sP - sN, sN)
    sn = dc * (aN - aP)
    if corr is not None:
        sn = sn + corr
    return ip * sn


def restate_near_interface(alpha):
    return np.where(alpha - 0.01 >= 0, 1.0, 0.0) * np.where(0.99 - alpha >= 0, 1.0, 0.0)


# ---- patches ---------------------------------------------------------------------------------------------------------------------------------------
def patch_case(syn):
    """a patch of 429 faces (more than one workgroup, no multiple of 256) on every third cell of the 13 x 11 x 9 box, the shape of
    test_interface_compression._patch_case: cell fields, their patchNeighbourFields and the patch's own arrays; a third of the faces see a
    zero gradient on both sides"""
    u = syn.splitmix_uniform
    n = 13 * 11 * 9
    fc = np.arange(0, n, 3, dtype=np.int32)
    m = fc.shape[0]
    delta_n = 1e-8 / 0.02 ** (1.0 / 3.0)
    grad = [20.0 * (u(800 + d, n) - 0.5) for d in range(3)]
    nbr = [20.0 * (u(810 + d, m) - 0.5) for d in range(3)]
    for g, q in zip(grad, nbr):
        g[fc[::3]] = 0.0
        q[::3] = 0.0
        q[1::9] = delta_n * (u(820, m)[1::9] - 0.5)
        g[fc[1::9]] = delta_n * (u(821, m)[1::9] - 0.5)
    alpha, nbr_alpha = u(830, n), u(831, m)
    return dict(n=n, fc=fc, m=m, delta_n=delta_n, grad=grad, nbr=nbr, w=0.3 + 0.4 * u(832, m), Sf=[u(840 + d, m) - 0.5 for d in range(3)],
                K=40.0 * (u(850, n) - 0.5), nbrK=40.0 * (u(851, m) - 0.5), alpha=alpha, nbr_alpha=nbr_alpha, dc=0.5 + u(852, m),
                corr=u(853, m) - 0.5, sigma=0.07)


def angle_case(syn, m=429):
    """a contact-angle patch: unit normals nf of seeded direction, the boundary gradient at a seeded angle to them with |a12| <= 0.999, theta
    in [10, 170] degrees; face 0 has a12 = 1 exactly (g = (1e10, 0, 0): adding delta_n is absorbed; Sf = (2, 0, 0), magSf = 2)"""
    u = syn.splitmix_uniform
    delta_n = 1e-8 / 0.02 ** (1.0 / 3.0)
    S = np.stack([u(860 + d, m) - 0.5 for d in range(3)])
    S[:, np.sum(S * S, axis=0) < 1e-3] = 0.3
    magSf = np.sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2])
    nf = S / magSf
    e = np.stack([u(870 + d, m) - 0.5 for d in range(3)])
    t = np.cross(nf.T, e.T).T
    t /= np.sqrt(np.sum(t * t, axis=0))
    cosang = 1.98 * (u(880, m) - 0.5)
    cosang[1::10] = 0.9985 * np.sign(cosang[1::10] + 1e-30)     # near the bound on both sides
    size = 0.5 + 30.0 * u(881, m)
    g = size * (cosang * nf + np.sqrt(1.0 - cosang * cosang) * t)
    theta = 10.0 + 160.0 * u(882, m)
    theta[2], theta[3] = 10.0, 170.0
    g[:, 0] = (1e10, 0.0, 0.0)
    S[:, 0] = (2.0, 0.0, 0.0)
    magSf[0] = 2.0
    return dict(m=m, delta_n=delta_n, g=[np.ascontiguousarray(x) for x in g], Sf=[np.ascontiguousarray(x) for x in S], magSf=magSf, theta=theta)


# ---- the physical check ----------------------------------------------------------------------------------------------------------------------------
def circle_curvature(syn, nx=32, radius=0.25):
    """a 32 x 32 x 1 uniform box of unit depth, alpha = 0.5*(1 - tanh((r - R)/(1.5 h))) about the centre, Gauss-linear gradient with
    zero-gradient boundaries, then nHatf and K through the restatement -> alpha, K"""
    case = syn.box_case(nx, nx, 1)
    n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
    h = 1.0 / nx
    c = np.arange(n)
    x, y = (c % nx + 0.5) * h, (c // nx + 0.5) * h
    alpha = 0.5 * (1.0 - np.tanh((np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2) - radius) / (1.5 * h)))
    xface = (up - lo) == 1
    Sf = [np.where(xface, h, 0.0), np.where(xface, 0.0, h), np.zeros(lo.shape[0])]
    vol = np.full(n, h * h)
    sides = [(c[c % nx == 0], (-h, 0.0)), (c[c % nx == nx - 1], (h, 0.0)), (c[c // nx == 0], (0.0, -h)), (c[c // nx == nx - 1], (0.0, h))]
    af = 0.5 * (alpha[lo] + alpha[up])
    grad = []
    for d in range(2):
        s = np.zeros(n)
        np.add.at(s, lo, Sf[d] * af)
        np.subtract.at(s, up, Sf[d] * af)
        for cells, sv in sides:
            np.add.at(s, cells, sv[d] * alpha[cells])               # zero gradient: the face value is the cell's
        grad.append(s / vol)
    grad.append(np.zeros(n))
    delta_n = 1e-8 / float(np.mean(vol)) ** (1.0 / 3.0)
    L = dict(n=n, lo=lo, up=up, Sf=Sf, fcs=[cells.astype(np.int32) for cells, _ in sides])
    nhatf, _, _ = restate_nhatf(lo, up, np.full(lo.shape[0], 0.5), Sf, grad, delta_n)
    bn = []
    for cells, sv in sides:                                         # the boundary value of gradAlpha: the cell's, its normal part removed
        nf = (sv[0] / h, sv[1] / h, 0.0)
        gn = grad[0][cells] * nf[0] + grad[1][cells] * nf[1]
        gb = [grad[0][cells] - nf[0] * gn, grad[1][cells] - nf[1] * gn, np.zeros(cells.shape[0])]
        pS = [np.full(cells.shape[0], sv[0]), np.full(cells.shape[0], sv[1]), np.zeros(cells.shape[0])]
        bn.append(restate_patch_nhatf(gb, pS, delta_n)[0])
    return alpha, restate_curvature(L, nhatf, np.concatenate(bn), vol)
