"""The kEpsilon model restated twice (kEpsilon.C:132-136, :229-280; epsilonWallFunctionFvPatchScalarField.C:116-396; nutkWallFunction :60-77;
bound.C:32-60; fvcAverage.C:71-74): literal loops over Python floats with an explicit fma, and vectorised numpy.  The kernels of
csrc/turbulence.inc are compared with the vectorised form bit for bit; a CPU test shows that the two forms agree and that the inputs reach
every branch.

A mesh here is a dict(n, lo, up, patches: [(faceCells, is_wall)]); boundary face fields are patch-ordered.  Rounding: every operator on its own;
fma in the interpolate of bound (mi_face_interpolate's rule), in mag (the contraction of DESIGN 3.5a) and on the three diagonal squares of
magSqr(symm).  max(a, b) = (a > b) ? a : b; pos(x) = (x >= 0) ? 1 : 0."""
import math

import numpy as np

from assembly_support import shape_case
from interface_support import MESHES, div, fma, fma_v

SMALL = 1e-15
BIG = "big"                                 # a 20 x 20 x 3 box: more unique wall cells than one 256-thread workgroup
ALL_MESHES = MESHES + (BIG,)
POW_LOG_BOUND = 16 * 2.0 ** -52             # relative; the OpenCL full-profile bound for pow (16 ulp), the looser of pow and log
DEFAULTS = (0.09, 1.44, 1.92, 1.3, 0.41, 9.8)


def rmax(a, b):
    """the reference's max: (a > b) ? a : b -- a NaN first operand gives b, a NaN second operand gives itself"""
    return a if a > b else b


def rmax_v(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.where(a > b, a, b)


# ---- coefficients ----------------------------------------------------------------------------------------------------------------------------
def y_plus_lam(kappa, E):
    ypl = 11.0
    for _ in range(10):
        ypl = math.log(max(E * ypl, 1.0)) / kappa
    return ypl


def coeffs(Cmu=0.09, C1=1.44, C2=1.92, sigmaEps=1.3, kappa=0.41, E=9.8):
    """the literal host formulas of mi_ke_coeffs_init"""
    return dict(Cmu=Cmu, C1=C1, C2=C2, sigmaEps=sigmaEps, kappa=kappa, E=E, Cmu25=math.sqrt(math.sqrt(Cmu)), Cmu75=math.pow(Cmu, 0.75),
                yPlusLam=y_plus_lam(kappa, E))


# ---- meshes and wall layouts -------------------------------------------------------------------------------------------------------------------
def box_sides(nx, ny, nz):
    c = np.arange(nx * ny * nz, dtype=np.int32)
    i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
    return dict(xmin=c[i == 0], xmax=c[i == nx - 1], ymin=c[j == 0], ymax=c[j == ny - 1], zmin=c[k == 0], zmax=c[k == nz - 1])


def box_layout(dims):
    """six patches: xmin and ymin declared ONE wall patch (their edge cells have two faces in the same patch), xmax (not a wall), ymax (wall),
    zmin (not a wall), zmax (wall) and a baffle on the xmin cells (wall): cells on one, two, three and four wall patches, non-wall patches
    between wall patches in patch order, and enough cells with three or more wall faces for the order of their sum to show"""
    s = box_sides(*dims)
    return [(np.concatenate([s["xmin"], s["ymin"]]), True), (s["xmax"], False), (s["ymax"], True), (s["zmin"], False), (s["zmax"], True),
            (s["xmin"][::-1].copy(), True)]


def graph_layout(n, faced):
    """for a mesh without geometry: four patches over seeded cell sets that share cells; the last holds every twelfth cell twice"""
    sets = [(np.arange(0, n, 3), True), (np.arange(2, n, 5), False), (np.arange(1, n, 2)[::-1], True),
            (np.concatenate([np.arange(0, n, 6), np.arange(0, n, 12)]), True)]
    out = []
    for cells, wall in sets:
        cells = cells.astype(np.int32)
        out.append((np.ascontiguousarray(cells[faced[cells]]), wall))
    return out


def mesh(pkg, name):
    syn = pkg.synthetic
    if name in ("box", BIG):
        dims = (5, 4, 3) if name == "box" else (20, 20, 3)
        case = syn.box_case(*dims)
        n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
        patches = box_layout(dims)
    else:
        case = shape_case(pkg, name)
        n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
        faced = (np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)) > 0
        patches = graph_layout(n, faced)
    return dict(name=name, n=n, lo=np.ascontiguousarray(lo, dtype=np.int32), up=np.ascontiguousarray(up, dtype=np.int32),
                patches=[(np.ascontiguousarray(fc, dtype=np.int32), bool(w)) for fc, w in patches])


def boundary_cells(L):
    return np.concatenate([fc for fc, _ in L["patches"]]).astype(np.int32)


def wall_mask(L):
    """per boundary face: on a wall patch"""
    return np.concatenate([np.full(fc.shape[0], w) for fc, w in L["patches"]])


def wall_tables(L):
    """mi_ke_create on the host: the unique wall cells ascending, per cell its wall faces (boundary face indices) by patch then by face, the
    corner weight 1.0/(number of wall faces of the cell)"""
    per = {}
    off = 0
    for fc, wall in L["patches"]:
        if wall:
            for i, c in enumerate(fc.tolist()):
                per.setdefault(c, []).append(off + i)
        off += fc.shape[0]
    cells = sorted(per)
    return dict(cells=np.array(cells, dtype=np.int32), faces=[per[c] for c in cells], weight=np.array([1.0 / len(per[c]) for c in cells]))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def bound_cell(L):
    """a cell with internal faces, and it with all its neighbours"""
    lo, up = L["lo"], L["up"]
    c0 = int(lo[lo.shape[0] // 2])
    return c0, np.unique(np.concatenate([up[lo == c0], lo[up == c0], [c0]]))


def inputs(syn, L, seed, K=None):
    """everything the entries read.  k, eps, nut positive; gradU nine arrays; the wall arrays with y chosen so that yPlus straddles yPlusLam
    (about half the wall faces on each side); v: the field bound() sees -- 30 % negative, cells exactly 0.0 and -0.0, a negative cell whose
    neighbours are all negative, the rest above the bound -- with its boundary values bv"""
    u = syn.splitmix_uniform
    K = coeffs() if K is None else K
    n, nf = L["n"], L["lo"].shape[0]
    bc = boundary_cells(L)
    nb = bc.shape[0]
    k = 0.01 + u(seed, n)
    eps = 0.1 + 10.0 * u(seed + 1, n)
    nut = 1e-4 + 1e-2 * u(seed + 2, n)
    nu_f = 1e-5 * (0.5 + u(seed + 3, n))
    grad = [20.0 * (u(seed + 4 + i, n) - 0.5) for i in range(9)]
    U = [u(seed + 13 + d, n) - 0.5 for d in range(3)]
    Uw = [0.2 * (u(seed + 16 + d, nb) - 0.5) for d in range(3)]
    bdc = 50.0 + 100.0 * u(seed + 19, nb)
    bnuw = 1e-5 * (0.5 + u(seed + 20, nb))
    target = K["yPlusLam"] * np.exp(2.0 * (u(seed + 21, nb) - 0.5))
    by = target * bnuw / (K["Cmu25"] * np.sqrt(k[bc])) if nb else np.zeros(0)
    bnutw = 1e-4 * u(seed + 22, nb)
    bnutw[::5] = 0.0
    G0, eps0 = u(seed + 23, n), 0.1 + u(seed + 24, n)             # what the wall pass finds in G and epsilon: kept off the wall cells
    pick = u(seed + 25, n)
    v = 0.05 + u(seed + 26, n)
    v[pick < 0.3] = -u(seed + 27, n)[pick < 0.3] - 1e-3
    v[5::17] = 0.0
    v[6::17] = -0.0
    c0, nbrs = bound_cell(L)
    v[nbrs] = -0.5 - u(seed + 28, nbrs.shape[0])
    bv = u(seed + 29, nb) - 0.3
    lam = 0.3 + 0.4 * u(seed + 30, nf)
    magSf = 0.5 + u(seed + 31, nf)
    bms = 0.5 + u(seed + 32, nb)
    ssf, bssf = u(seed + 33, nf) - 0.5, u(seed + 34, nb) - 0.5
    return dict(K=K, k=k, eps=eps, nut=nut, nu=1.3e-5, nu_f=nu_f, grad=grad, U=U, Uw=Uw, bdc=bdc, by=by, bnuw=bnuw, bnutw=bnutw, G0=G0, eps0=eps0,
                v=v, bv=bv, lb=SMALL, lam=lam, magSf=magSf, bms=bms, ssf=ssf, bssf=bssf)


# ---- literal loops -------------------------------------------------------------------------------------------------------------------------------
def literal_production(nut, grad):
    out = []
    G = [g.tolist() for g in grad]
    for c, nt in enumerate(nut.tolist()):
        xx, xy, xz, yx, yy, yz, zx, zy, zz = [G[i][c] for i in range(9)]
        sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
        s = fma(xx, xx, 2.0 * (sxy * sxy))
        s = fma(2.0, sxz * sxz, s)
        s = fma(yy, yy, s)
        s = fma(2.0, syz * syz, s)
        s = fma(zz, zz, s)
        out.append((nt * 2.0) * s)
    return np.array(out)


def literal_terms(K, G, eps, k, nut, nu):
    """-> su, sp, deps of the epsilon equation, sp, dk of the k equation, nut afterwards; nu a number or a cell array"""
    nuv = nu.tolist() if isinstance(nu, np.ndarray) else [nu] * len(k)
    su, sp, de, spk, dk, nt = [], [], [], [], [], []
    for g, e, kk, t, v in zip(G.tolist(), eps.tolist(), k.tolist(), nut.tolist(), nuv):
        su.append(div((K["C1"] * g) * e, kk)); sp.append(div(K["C2"] * e, kk)); de.append(div(t, K["sigmaEps"]) + v)
        spk.append(div(e, kk)); dk.append(t + v); nt.append(div(K["Cmu"] * (kk * kk), e))
    return [np.array(x) for x in (su, sp, de, spk, dk, nt)]


def literal_wall_cells(L, I, G, eps, p15=None):
    """-> G, eps (cell fields with the wall cells overwritten), b_eps, b_pow per boundary face (NaN off the wall faces); p15: pow(k, 1.5) per
    boundary face to continue from (the device's own), otherwise Python's"""
    K, W = I["K"], wall_tables(L)
    G, eps = G.copy(), eps.copy()
    nb = I["by"].shape[0]
    beps, bpow = np.full(nb, np.nan), np.full(nb, np.nan)
    for c, faces, w in zip(W["cells"].tolist(), W["faces"], W["weight"].tolist()):
        kc = float(I["k"][c])
        Gc = ec = 0.0
        for bf in faces:
            p = math.pow(kc, 1.5) if p15 is None else float(p15[bf])
            sn = [float(I["bdc"][bf]) * (float(I["Uw"][d][bf]) - float(I["U"][d][c])) for d in range(3)]
            mgu = math.sqrt(fma(sn[2], sn[2], fma(sn[0], sn[0], sn[1] * sn[1])))
            den = K["kappa"] * float(I["by"][bf])
            ec = ec + ((w * K["Cmu75"]) * p) / den
            Gc = Gc + ((((w * (float(I["bnutw"][bf]) + float(I["bnuw"][bf]))) * mgu) * K["Cmu25"]) * math.sqrt(kc)) / den
            bpow[bf] = p
        G[c], eps[c] = Gc, ec
        for bf in faces:
            beps[bf] = ec
    return G, eps, beps, bpow


def literal_nut_wall(L, I, k, lg=None):
    """-> b_nutw, b_log per boundary face (NaN off the wall faces; b_log NaN where the branch is not taken); lg: the log values to continue from"""
    K = I["K"]
    bc, wall = boundary_cells(L), wall_mask(L)
    out, blog = np.full(bc.shape[0], np.nan), np.full(bc.shape[0], np.nan)
    for bf in np.nonzero(wall)[0].tolist():
        nuw = float(I["bnuw"][bf])
        yPlus = ((K["Cmu25"] * float(I["by"][bf])) * math.sqrt(float(k[bc[bf]]))) / nuw
        if yPlus > K["yPlusLam"]:
            l = math.log(K["E"] * yPlus) if lg is None else float(lg[bf])
            blog[bf] = l
            out[bf] = nuw * (((yPlus * K["kappa"]) / l) - 1.0)
        else:
            out[bf] = 0.0
    return out, blog


def _rows(L):
    n = L["n"]
    own, nei, bnd = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    for f, (P, N) in enumerate(zip(L["lo"].tolist(), L["up"].tolist())):
        own[P].append(f); nei[N].append(f)
    for i, c in enumerate(boundary_cells(L).tolist()):
        bnd[c].append(i)
    return own, nei, bnd


def literal_average(L, magSf, bms, ssf, bssf):
    """-> surfaceSum(magSf*ssf)/surfaceSum(magSf), surfaceSum(magSf): own faces ascending, losort faces, boundary faces patch by patch"""
    own, nei, bnd = _rows(L)
    m, b, x, bx = magSf.tolist(), bms.tolist(), ssf.tolist(), bssf.tolist()
    out, sums = [], []
    for c in range(L["n"]):
        s = t = 0.0
        for f in own[c] + nei[c]:
            s = s + m[f] * x[f]; t = t + m[f]
        for i in bnd[c]:
            s = s + b[i] * bx[i]; t = t + b[i]
        out.append(div(s, t)); sums.append(t)
    return np.array(out), np.array(sums)


def literal_bound(L, lb, lam, magSf, bms, bface, v):
    own, nei, bnd = _rows(L)
    lo, up = L["lo"].tolist(), L["up"].tolist()
    m, b, w, bf_, x = magSf.tolist(), bms.tolist(), lam.tolist(), bface.tolist(), v.tolist()
    out = []
    for c in range(L["n"]):
        s = t = 0.0
        for f in own[c] + nei[c]:
            mP, mN = rmax(x[lo[f]], lb), rmax(x[up[f]], lb)
            s = s + m[f] * fma(w[f], mP - mN, mN); t = t + m[f]
        for i in bnd[c]:
            s = s + b[i] * bf_[i]; t = t + b[i]
        avg = div(s, t)
        pos = 1.0 if -x[c] >= 0 else 0.0
        out.append(rmax(rmax(x[c], avg * pos), lb))
    return np.array(out)


# ---- the same, vectorised ----------------------------------------------------------------------------------------------------------------------
def restate_production(nut, grad, contracted=True, late_double=False):
    """contracted False: every operator of magSqr rounded; late_double: nut*(2*m) -- the alternatives the CPU test looks at"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = grad
    sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
    if contracted:
        s = fma_v(xx, xx, 2.0 * (sxy * sxy))
        s = fma_v(2.0, sxz * sxz, s)
        s = fma_v(yy, yy, s)
        s = fma_v(2.0, syz * syz, s)
        s = fma_v(zz, zz, s)
    else:
        s = xx * xx + 2.0 * (sxy * sxy) + 2.0 * (sxz * sxz) + yy * yy + 2.0 * (syz * syz) + zz * zz
    return nut * (2.0 * s) if late_double else (nut * 2.0) * s


def restate_terms(K, G, eps, k, nut, nu):
    with np.errstate(all="ignore"):
        return [((K["C1"] * G) * eps) / k, (K["C2"] * eps) / k, nut / K["sigmaEps"] + nu, eps / k, nut + nu, (K["Cmu"] * (k * k)) / eps]


def restate_wall_cells(L, I, G, eps, p15=None, reverse_patches=False, regroup=False):
    """-> G, eps, b_eps, b_pow as literal_wall_cells.  ufunc.at is unbuffered and walks its indices in order: the wall faces in boundary order
    give every cell its faces by patch, then by face, from 0.0.  reverse_patches / regroup: alternatives the CPU test shows to be visible"""
    K = I["K"]
    bc, wall = boundary_cells(L), wall_mask(L)
    wf = np.nonzero(wall)[0]
    c = bc[wf]
    count = np.bincount(c, minlength=L["n"])
    with np.errstate(all="ignore"):
        w = 1.0 / count[c]
        kc = I["k"][c]
        p = np.power(kc, 1.5) if p15 is None else p15[wf]
        sn = [I["bdc"][wf] * (I["Uw"][d][wf] - I["U"][d][c]) for d in range(3)]
        mgu = np.sqrt(fma_v(sn[2], sn[2], fma_v(sn[0], sn[0], sn[1] * sn[1])))
        den = K["kappa"] * I["by"][wf]
        e = (w * (K["Cmu75"] * p)) / den if regroup else ((w * K["Cmu75"]) * p) / den
        g = ((((w * (I["bnutw"][wf] + I["bnuw"][wf])) * mgu) * K["Cmu25"]) * np.sqrt(kc)) / den
    Gc, ec = np.zeros(L["n"]), np.zeros(L["n"])
    order = np.arange(wf.shape[0])
    if reverse_patches:
        pid = np.concatenate([np.full(fc.shape[0], i) for i, (fc, _) in enumerate(L["patches"])])[wf]
        order = np.argsort(-pid, kind="stable")
    np.add.at(ec, c[order], e[order]); np.add.at(Gc, c[order], g[order])
    G, eps = G.copy(), eps.copy()
    cells = np.unique(c)
    G[cells], eps[cells] = Gc[cells], ec[cells]
    nb = bc.shape[0]
    beps, bpow = np.full(nb, np.nan), np.full(nb, np.nan)
    beps[wf], bpow[wf] = ec[c], p
    return G, eps, beps, bpow


def restate_nut_wall(L, I, k, lg=None):
    """-> b_nutw, b_log, taken (per boundary face)"""
    K = I["K"]
    bc, wall = boundary_cells(L), wall_mask(L)
    with np.errstate(all="ignore"):
        yPlus = ((K["Cmu25"] * I["by"]) * np.sqrt(k[bc])) / I["bnuw"]
        taken = wall & (yPlus > K["yPlusLam"])
        l = np.log(K["E"] * yPlus) if lg is None else lg
        r = I["bnuw"] * (((yPlus * K["kappa"]) / l) - 1.0)
    return np.where(wall, np.where(taken, r, 0.0), np.nan), np.where(taken, l, np.nan), taken


def restate_average(L, magSf, bms, ssf, bssf, fused=False):
    """fused: the products contracted into the sum, the alternative the CPU test shows to be visible"""
    lo, up, bc = L["lo"], L["up"], boundary_cells(L)
    t = np.zeros(L["n"])
    np.add.at(t, lo, magSf); np.add.at(t, up, magSf); np.add.at(t, bc, bms)
    if fused:
        s = [0.0] * L["n"]
        for idx, a, b in ((lo, magSf, ssf), (up, magSf, ssf), (bc, bms, bssf)):
            for c, x, y in zip(idx.tolist(), a.tolist(), b.tolist()):
                s[c] = fma(x, y, s[c])
        s = np.array(s)
    else:
        s = np.zeros(L["n"])
        np.add.at(s, lo, magSf * ssf); np.add.at(s, up, magSf * ssf); np.add.at(s, bc, bms * bssf)
    with np.errstate(all="ignore"):
        return s / t, t


def restate_bound(L, lb, lam, magSf, bms, bface, v, plain_interpolate=False, strict_pos=False, select=False):
    """plain_interpolate: w*mP + (1 - w)*mN; strict_pos: pos as x > 0; select: avg where pos, 0 elsewhere, in place of the product -- the
    alternatives the CPU test looks at"""
    lo, up = L["lo"], L["up"]
    m = rmax_v(v, lb)
    i = lam * m[lo] + (1.0 - lam) * m[up] if plain_interpolate else fma_v(lam, m[lo] - m[up], m[up])
    avg, _ = restate_average(L, magSf, bms, i, bface)
    with np.errstate(all="ignore"):
        pos = (-v > 0) if strict_pos else (-v >= 0)
        t = np.where(pos, avg, 0.0) if select else avg * np.where(pos, 1.0, 0.0)
    return rmax_v(rmax_v(v, t), lb)


def needs_bound(v, bv, lb):
    """bound.C:35-37: min over the internal and the boundary values"""
    return min(float(v.min()) if v.size else math.inf, float(bv.min()) if bv.size else math.inf) < lb


# ---- channel_walk: three correct() steps on a small channel ------------------------------------------------------------------------------------
CHANNEL_DIMS = (6, 5, 4)
CHANNEL = dict(dt=0.02, nu=1e-4, alpha_eps=0.7, alpha_k=0.8, k_in=0.02, eps_in=0.5, steps=3)


def channel(pkg):
    """a 6 x 5 x 4 box of spacing 0.1: walls at ymin, ymax, zmin and zmax, a fixed-value inlet at xmin and a zero-gradient outlet at xmax, in the
    patch order wall, inlet, wall, outlet, wall, wall; a unit flux along x; seeded cell velocities, velocity gradients and wall distances (y is
    the caller's patch array) with yPlus on both sides of yPlusLam"""
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    nx, ny, nz = CHANNEL_DIMS
    case = syn.box_case(nx, ny, nz)
    n, lo, up = case.n_cells, np.ascontiguousarray(case.lower_addr, dtype=np.int32), np.ascontiguousarray(case.upper_addr, dtype=np.int32)
    nf, h = lo.shape[0], 0.1
    s = box_sides(nx, ny, nz)
    kinds = ["wall", "inlet", "wall", "outlet", "wall", "wall"]
    fcs = [s["ymin"], s["xmin"], s["ymax"], s["xmax"], s["zmin"], s["zmax"]]
    L = dict(name="channel", n=n, lo=lo, up=up, patches=[(np.ascontiguousarray(fc, dtype=np.int32), kd == "wall") for fc, kd in zip(fcs, kinds)])
    nb = boundary_cells(L).shape[0]
    pid = np.concatenate([np.full(fc.shape[0], i) for i, fc in enumerate(fcs)])
    kind_of = np.array(kinds)[pid]
    xface = (up.astype(np.int64) - lo) == 1
    phi = np.where(xface, h * h, 0.0)
    bphi = np.where(kind_of == "inlet", -h * h, np.where(kind_of == "outlet", h * h, 0.0))
    M = dict(L=L, K=coeffs(), n=n, lo=lo, up=up, nf=nf, nb=nb, kinds=kinds, pid=pid, kind_of=kind_of, V=np.full(n, h ** 3), magSf=np.full(nf, h * h),
             dc=np.full(nf, 1.0 / h), lam=np.full(nf, 0.5), bms=np.full(nb, h * h), bdc=np.full(nb, 2.0 / h), by=0.5 * h * np.exp(-2.3 * u(3001, nb)),
             phi=phi, bphi=bphi, U=[0.6 + 0.4 * u(3002, n), 0.1 * (u(3003, n) - 0.5), 0.1 * (u(3004, n) - 0.5)], Uw=[np.zeros(nb) for _ in range(3)],
             grad=[5.0 * (u(3010 + i, n) - 0.5) for i in range(9)], bnuw=np.full(nb, CHANNEL["nu"]), **CHANNEL)
    k = M["k_in"] * (0.8 + 0.4 * u(3020, n))
    eps = M["eps_in"] * (0.8 + 0.4 * u(3021, n))
    return M, dict(k=k, eps=eps, bk=boundary_values(M, k, M["k_in"]), beps=boundary_values(M, eps, M["eps_in"]))


def boundary_values(M, cell, inlet_value):
    """the fixed value on the inlet, the cell value elsewhere (zero gradient: the outlet, kqRWallFunction, the evaluated epsilonWallFunction)"""
    return np.where(M["kind_of"] == "inlet", inlet_value, cell[boundary_cells(M["L"])])


def patch_coeffs(M, bgamma, inlet_value):
    """per patch the internalCoeffs and boundaryCoeffs of fvm::div(phi, vf) - fvm::laplacian(gamma, vf): fixed value: the diffusion
    coefficient and (diff - phi)*value; zero gradient: the flux and nothing"""
    diff = (bgamma * M["bms"]) * M["bdc"]
    fixed = M["kind_of"] == "inlet"
    ic = np.where(fixed, diff, M["bphi"])
    bc = np.where(fixed, diff * inlet_value - M["bphi"] * inlet_value, 0.0)
    cut = np.cumsum([0] + [fc.shape[0] for fc, _ in M["L"]["patches"]])
    return [np.ascontiguousarray(ic[a:b]) for a, b in zip(cut[:-1], cut[1:])], [np.ascontiguousarray(bc[a:b]) for a, b in zip(cut[:-1], cut[1:])]


def wall_inputs(M, k, bnut):
    return dict(K=M["K"], k=k, U=M["U"], Uw=M["Uw"], bdc=M["bdc"], by=M["by"], bnuw=M["bnuw"], bnutw=bnut)


def restate_nut_update(M, k, eps, bk, beps, blog):
    """kEpsilon.C:135-136 / :278-279: nut = Cmu*sqr(k)/epsilon on the cells and on every boundary face, then nutkWallFunction on the wall faces"""
    K, wall = M["K"], wall_mask(M["L"])
    nut = (K["Cmu"] * (k * k)) / eps
    bnut = (K["Cmu"] * (bk * bk)) / beps
    nutw, _, taken = restate_nut_wall(M["L"], wall_inputs(M, k, None), k, lg=blog)
    return nut, np.where(wall, nutw, bnut), taken


def restate_bound_field(M, v, bv, lb):
    """bound.C:32-60 -> the field, its boundary values, whether it was bounded"""
    if not needs_bound(v, bv, lb):
        return v, bv, False
    bface = rmax_v(bv, lb)
    return restate_bound(M["L"], lb, M["lam"], M["magSf"], M["bms"], bface, v), bface, True


def restate_equation(orc, M, psi_old, psi, su, sp, gamma, bgamma, inlet_value, alpha, set_cells=None):
    """fvm::ddt + fvm::div - fvm::laplacian == su - fvm::Sp(sp), relax(alpha), [setValues on set_cells], and what the solver is given: through the
    oracle's sweeps (the unfused sequence of tests/assembly_full_size.py) -> dict of every array"""
    from assembly_full_size import oracle_assemble
    n, lo, up = M["n"], M["lo"], M["up"]
    gam = orc.face_interpolate(lo, up, M["lam"], gamma) * M["magSf"]
    a = oracle_assemble(orc, M, dict(vol=M["V"]), dict(rdt=1.0 / M["dt"], psi_old=[psi_old]), dict(flux=M["phi"], weights=M["lam"]),
                        dict(delta=M["dc"], gamma=gam), sp=(sp, 1.0), su=[(-1.0, [su])])
    fcs = [fc for fc, _ in M["L"]["patches"]]
    ic, bc = patch_coeffs(M, bgamma, inlet_value)
    out = dict(gam=gam, upper0=a["upper"], lower0=a["lower"], diag0=a["diag"], source0=a["source0"])
    diag, source = orc.relax(n, lo, up, alpha, a["diag"], a["lower"], a["upper"], a["source0"], psi, fcs, ic, bc, [0] * len(fcs))
    upper, lower = a["upper"], a["lower"]
    out.update(diag1=diag, source1=source)
    if set_cells is not None:
        sv = orc.set_values(n, lo, up, set_cells, psi[set_cells], psi, diag, source, upper, lower, fcs, ic, bc)
        psi, source, upper, lower, ic, bc = sv["psi"], sv["source"], sv["upper"], sv["lower"], sv["icoeffs"], sv["bcoeffs"]
    dt_, st_ = diag, source
    for fc, i, b in zip(fcs, ic, bc):
        dt_ = orc.patch_add(fc, i, dt_, 0); st_ = orc.patch_add(fc, b, st_, 0)
    out.update(psi=psi, upper=upper, lower=lower, source=source, ic=np.concatenate(ic), bc=np.concatenate(bc), diag_solve=dt_, source_solve=st_)
    return out


def restate_correct(orc, M, S, X):
    """kEpsilon::correct() :229-280 from the state S (k, eps, nut and their boundary values) -> (every intermediate, the next state).  X: what the
    restatement continues from -- the device's pow and log values and the two solutions of the engine's solver"""
    K, L, nu = M["K"], M["L"], M["nu"]
    wall = wall_mask(L)
    W = wall_tables(L)
    G = restate_production(S["nut"], M["grad"])
    G, eps, beps_w, _ = restate_wall_cells(L, wall_inputs(M, S["k"], S["bnut"]), G, S["eps"], p15=X["bpow"])
    beps = np.where(wall, beps_w, S["beps"])
    su, sp, de, _, _, _ = restate_terms(K, G, eps, S["k"], S["nut"], nu)
    out = dict(G=G, eps_wall=eps, beps_wall=beps, su=su, sp=sp, deps=de)
    e = restate_equation(orc, M, S["eps"], eps, su, sp, de, S["bnut"] / K["sigmaEps"] + nu, M["eps_in"], M["alpha_eps"], set_cells=W["cells"])
    out.update({"eps_" + key: v for key, v in e.items()})
    eps = X["eps_solved"]
    eps, beps, out["eps_bounded"] = restate_bound_field(M, eps, boundary_values(M, eps, M["eps_in"]), SMALL)
    _, _, _, spk, dk, _ = restate_terms(K, G, eps, S["k"], S["nut"], nu)
    q = restate_equation(orc, M, S["k"], S["k"], G, spk, dk, S["bnut"] + nu, M["k_in"], M["alpha_k"])
    out.update({"k_" + key: v for key, v in q.items()})
    out.update(sp_k=spk, dk=dk, eps_new=eps, beps_new=beps)
    k = X["k_solved"]
    k, bk, out["k_bounded"] = restate_bound_field(M, k, boundary_values(M, k, M["k_in"]), SMALL)
    nut, bnut, taken = restate_nut_update(M, k, eps, bk, beps, X["blog"])
    out.update(k_new=k, bk_new=bk, nut=nut, bnut=bnut)
    return out, dict(k=k, eps=eps, bk=bk, beps=beps, nut=nut, bnut=bnut), taken
