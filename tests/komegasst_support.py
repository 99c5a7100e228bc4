"""The kOmegaSST model restated twice (kOmegaSST.C:47-111, :284-296, :398-468; kOmegaSST.H:164-243; omegaWallFunctionFvPatchScalarField.C:209-394,
:548-596; fvMatrix.C:2208-2216, :2759-2814; fvmSup.C:100-214): literal loops over Python floats with an explicit fma, and vectorised
numpy.  The kernels of csrc/turbulence.inc are compared with the vectorised form bit for bit; a CPU test shows that the two forms agree and
that the inputs reach every branch.  Not pinned by a compiled reference.

Meshes, wall layouts and the wall arrays are those of turbulence_support.  Rounding: every field operator on its own; fma in gradK & gradOmega
(the dot product of DESIGN 3.5a), in mag (3.5n) and on the first square of the omega functor; max(a, b) = (a > b) ? a : b, min(a, b) = (a < b) ? a : b;
pow4(s) = sqr(sqr(s)).  tanh: numpy's, or the values the caller continues from (the device's)."""
import math

import numpy as np

from turbulence_support import (SMALL, boundary_cells, channel as ke_channel, div, fma, fma_v, inputs as ke_inputs, patch_coeffs,
                                restate_bound_field, restate_nut_wall, rmax, rmax_v, wall_inputs, wall_mask, wall_tables)

TANH_BOUND = 7 * 2.0 ** -52                 # relative; the OpenCL full-profile bound for tanh (5 ulp) plus 2 for the host's libm
MODEL = ("alphaK1", "alphaK2", "alphaOmega1", "alphaOmega2", "gamma1", "gamma2", "beta1", "beta2", "betaStar", "a1", "b1", "c1")
MODEL_DEFAULTS = (0.85, 1.0, 0.5, 0.856, 5.0 / 9.0, 0.44, 0.075, 0.0828, 0.09, 0.31, 1.0, 10.0)
WALL = ("Cmu", "kappa", "E", "wallBeta1")
WALL_DEFAULTS = (0.09, 0.41, 9.8, 0.075)


def rmin(a, b):
    return a if a < b else b


def rmin_v(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.where(a < b, a, b)


def coeffs(**given):
    """the literal host formulas of mi_sst_coeffs_init"""
    S = dict(zip(MODEL + WALL, MODEL_DEFAULTS + WALL_DEFAULTS))
    S.update(given)
    S.update(twoAlphaOmega2=2 * S["alphaOmega2"], fourAlphaOmega2=4 * S["alphaOmega2"], invBetaStar=1.0 / S["betaStar"],
             twoInvBetaStar=2.0 / S["betaStar"], c1a1BetaStar=(S["c1"] / S["a1"]) * S["betaStar"], c1BetaStar=S["c1"] * S["betaStar"],
             dAlphaK=S["alphaK1"] - S["alphaK2"], dAlphaOmega=S["alphaOmega1"] - S["alphaOmega2"], dBeta=S["beta1"] - S["beta2"],
             dGamma=S["gamma1"] - S["gamma2"], Cmu25=math.sqrt(math.sqrt(S["Cmu"])))
    ypl = 11.0
    for _ in range(10):
        ypl = math.log(max(S["E"] * ypl, 1.0)) / S["kappa"]
    S["yPlusLam"] = ypl
    return S


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def inputs(syn, L, seed):
    """turbulence_support.inputs (k, nut, nu, nu_f, gradU, the wall arrays, G0) and what kOmegaSST adds: omega over four decades, the wall
    distance y over two, a larger nu, gradK and gradOmega with a product of both signs over seven decades and exactly tiny on every seventh cell, what the
    wall pass finds in omega (omega0), and an assembled diagonal and source with the cell volumes.  The ranges are chosen so that every arm of
    every max / min of the model is taken by at least a twentieth of the cells (tests/test_komegasst.py asserts it)"""
    u = syn.splitmix_uniform
    I = ke_inputs(syn, L, seed)
    n = L["n"]
    omega = 10.0 ** (4.0 * u(seed + 40, n))
    y = 10.0 ** (-3.0 + 2.0 * u(seed + 41, n))
    gk = [2.0 * (u(seed + 42 + d, n) - 0.5) for d in range(3)]
    scale = 13.6 * omega * I["k"] / (y * y) * 10.0 ** (1.0 - 4.0 * u(seed + 45, n))   # (4*alphaOmega2)*k/(CDkOmega*sqr(y)) from about 0.1 to 1000
    go = [scale * (u(seed + 46 + d, n) - 0.5) for d in range(3)]
    for d in range(3):
        gk[d][3::7] *= 1e-30
    I.update(S=coeffs(), nu=1e-4, nu_f=1e-4 * (0.5 + u(seed + 53, n)), omega=omega, y=y, gradK=gk, gradOmega=go, omega0=0.1 + 100.0 * u(seed + 49, n), V=1e-3 * (0.5 + u(seed + 50, n)),
             diagL=1.0 + u(seed + 51, n), sourceL=u(seed + 52, n) - 0.5)
    return I


# ---- literal loops -------------------------------------------------------------------------------------------------------------------------------
def _magsqr_symm(g):
    xx, xy, xz, yx, yy, yz, zx, zy, zz = g
    sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
    s = fma(xx, xx, 2.0 * (sxy * sxy))
    s = fma(2.0, sxz * sxz, s)
    s = fma(yy, yy, s)
    s = fma(2.0, syz * syz, s)
    return fma(zz, zz, s)


def literal_production(nut, grad):
    """-> S2, G, mag(symm(gradU))"""
    G = [g.tolist() for g in grad]
    S2, out, mag = [], [], []
    for c, nt in enumerate(nut.tolist()):
        m = _magsqr_symm([G[i][c] for i in range(9)])
        S2.append(2.0 * m); out.append(nt * (2.0 * m)); mag.append(math.sqrt(m))
    return np.array(S2), np.array(out), np.array(mag)


def literal_wall_cells(L, I, G, omega):
    """-> G, omega (cell fields with the wall cells overwritten), b_omega per boundary face (NaN off the wall faces)"""
    S, W = I["S"], wall_tables(L)
    G, omega = G.copy(), omega.copy()
    bom = np.full(I["by"].shape[0], np.nan)
    ck = S["Cmu25"] * S["kappa"]
    for c, faces, w in zip(W["cells"].tolist(), W["faces"], W["weight"].tolist()):
        kc = float(I["k"][c])
        Gc = oc = 0.0
        for bf in faces:
            y, nuw = float(I["by"][bf]), float(I["bnuw"][bf])
            sn = [float(I["bdc"][bf]) * (float(I["Uw"][d][bf]) - float(I["U"][d][c])) for d in range(3)]
            mgu = math.sqrt(fma(sn[2], sn[2], fma(sn[0], sn[0], sn[1] * sn[1])))
            ov = div(6.0 * nuw, S["wallBeta1"] * (y * y))
            ol = div(math.sqrt(kc), ck * y)
            oc = oc + w * math.sqrt(fma(ov, ov, ol * ol))
            Gc = Gc + div((((w * (float(I["bnutw"][bf]) + nuw)) * mgu) * S["Cmu25"]) * math.sqrt(kc), S["kappa"] * y)
        G[c], omega[c] = Gc, oc
        for bf in faces:
            bom[bf] = oc
    return G, omega, bom


def _nu_list(nu, n):
    return nu.tolist() if isinstance(nu, np.ndarray) else [nu] * n


def literal_args(S, gk, go, k, omega, y, nu):
    """-> CDkOmega, arg1, arg2, arg3: everything before the first tanh"""
    out = [[], [], [], []]
    cols = [a.tolist() for a in (*gk, *go, k, omega, y)]
    for c, (kx, ky, kz, ox, oy, oz, kk, om, yy) in enumerate(zip(*cols)):
        v = _nu_list(nu, len(cols[0]))[c]
        CD = div(S["twoAlphaOmega2"] * fma(kz, oz, fma(kx, ox, ky * oy)), om)
        CDp = rmax(CD, 1.0e-10)
        y2, sk = yy * yy, math.sqrt(kk)
        far = div(500.0 * v, y2 * om)
        a1 = rmin(rmin(rmax(div(S["invBetaStar"] * sk, om * yy), far), div(S["fourAlphaOmega2"] * kk, CDp * y2)), 10.0)
        a2 = rmin(rmax(div(S["twoInvBetaStar"] * sk, om * yy), far), 100.0)
        a3 = rmin(div(150.0 * v, om * y2), 10.0)
        for o, x in zip(out, (CD, a1, a2, a3)):
            o.append(x)
    return [np.array(o) for o in out]


def literal_blend(S, F1, F23, CD, omega, nut, S2, nu):
    """from F1, F23 and CDkOmega -> su, sp, susp, DomegaEff, DkEff"""
    out = [[], [], [], [], []]
    nuv = _nu_list(nu, len(F1))
    for f1, f23, cd, om, nt, s2, v in zip(F1.tolist(), F23.tolist(), CD.tolist(), omega.tolist(), nut.tolist(), S2.tolist(), nuv):
        bl = lambda X: f1 * S["d" + X[0].upper() + X[1:]] + S[X + "2"]
        lim = rmax(S["a1"] * om, (S["b1"] * f23) * math.sqrt(s2))
        row = (bl("gamma") * rmin(s2, (S["c1a1BetaStar"] * om) * lim), bl("beta") * om, div((f1 - 1.0) * cd, om), bl("alphaOmega") * nt + v,
               bl("alphaK") * nt + v)
        for o, x in zip(out, row):
            o.append(x)
    return [np.array(o) for o in out]


def literal_omega_sources(V, su, sp, susp, omega, diag, source):
    d, s = [], []
    for v, a, b, c, om, dl, sl in zip(*[x.tolist() for x in (V, su, sp, susp, omega, diag, source)]):
        d.append(dl - ((-(v * b)) - v * rmax(c, 0.0)))
        s.append(sl - ((-(v * a)) - (0.0 - (v * rmin(c, 0.0)) * om)))
    return np.array(d), np.array(s)


def literal_k_terms(S, G, k, omega):
    su, sp = [], []
    for g, kk, om in zip(G.tolist(), k.tolist(), omega.tolist()):
        su.append(rmin(g, (S["c1BetaStar"] * kk) * om)); sp.append(S["betaStar"] * om)
    return np.array(su), np.array(sp)


def literal_nut(S, F23, k, omega, s, ctor=False):
    out = []
    for f23, kk, om, x in zip(F23.tolist(), k.tolist(), omega.tolist(), s.tolist()):
        strain = ((S["b1"] * f23) * math.sqrt(2.0)) * x if ctor else (S["b1"] * f23) * math.sqrt(x)
        out.append(div(S["a1"] * kk, rmax(S["a1"] * om, strain)))
    return np.array(out)


# ---- the same, vectorised ----------------------------------------------------------------------------------------------------------------------
def restate_production(nut, grad):
    """-> S2, G, mag(symm(gradU))"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = grad
    sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
    s = fma_v(xx, xx, 2.0 * (sxy * sxy))
    s = fma_v(2.0, sxz * sxz, s)
    s = fma_v(yy, yy, s)
    s = fma_v(2.0, syz * syz, s)
    s = fma_v(zz, zz, s)
    S2 = 2.0 * s
    return S2, nut * S2, np.sqrt(s)


def restate_wall_cells(L, I, G, omega, reverse_patches=False, contracted=True):
    """-> G, omega, b_omega as literal_wall_cells.  ufunc.at walks its indices in order: the wall faces in boundary order give every cell its
    faces by patch, then by face, from 0.0.  reverse_patches / contracted=False: alternatives the CPU test shows to be visible"""
    S = I["S"]
    bc, wall = boundary_cells(L), wall_mask(L)
    wf = np.nonzero(wall)[0]
    c = bc[wf]
    count = np.bincount(c, minlength=L["n"])
    with np.errstate(all="ignore"):
        w = 1.0 / count[c]
        kc, y, nuw = I["k"][c], I["by"][wf], I["bnuw"][wf]
        sn = [I["bdc"][wf] * (I["Uw"][d][wf] - I["U"][d][c]) for d in range(3)]
        mgu = np.sqrt(fma_v(sn[2], sn[2], fma_v(sn[0], sn[0], sn[1] * sn[1])))
        ov = (6.0 * nuw) / (S["wallBeta1"] * (y * y))
        ol = np.sqrt(kc) / ((S["Cmu25"] * S["kappa"]) * y)
        o = w * np.sqrt(fma_v(ov, ov, ol * ol) if contracted else ov * ov + ol * ol)
        g = ((((w * (I["bnutw"][wf] + nuw)) * mgu) * S["Cmu25"]) * np.sqrt(kc)) / (S["kappa"] * y)
    Gc, oc = np.zeros(L["n"]), np.zeros(L["n"])
    order = np.arange(wf.shape[0])
    if reverse_patches:
        pid = np.concatenate([np.full(fc.shape[0], i) for i, (fc, _) in enumerate(L["patches"])])[wf]
        order = np.argsort(-pid, kind="stable")
    np.add.at(oc, c[order], o[order]); np.add.at(Gc, c[order], g[order])
    G, omega = G.copy(), omega.copy()
    cells = np.unique(c)
    G[cells], omega[cells] = Gc[cells], oc[cells]
    bom = np.full(bc.shape[0], np.nan)
    bom[wf] = oc[c]
    return G, omega, bom


def restate_f23(S, f3, k, omega, y, nu, regroup=False):
    """-> arg2, arg3, F2's and F3's tanh arguments sqr(arg2) and pow4(arg3), the first operand of arg2's max"""
    with np.errstate(all="ignore"):
        y2, sk = y * y, np.sqrt(k)
        far = (500.0 * nu) / (y2 * omega)
        near = ((2.0 * sk) / S["betaStar"]) / (omega * y) if regroup else (S["twoInvBetaStar"] * sk) / (omega * y)
        arg2 = rmin_v(rmax_v(near, far), 100.0)
        arg3 = rmin_v((150.0 * nu) / (omega * y2), 10.0)
        q3 = arg3 * arg3
    return arg2, arg3, arg2 * arg2, q3 * q3, near


def f23_of(f3, p2, p3):
    """numpy's F23 and tanh(pow4(arg3)) from the tanh arguments"""
    t3 = np.tanh(p3) if f3 else np.zeros_like(p3)
    F2 = np.tanh(p2)
    return (F2 * (1.0 - t3) if f3 else F2), t3


def restate_blend(S, f3, gk, go, k, omega, y, nut, S2, nu, cont=None, plain_dot=False, regroup=False):
    """mi_sst_blend -> dict of F1, su, sp, susp, domega, dk, CD, arg1, arg2, arg3, F23, t3, p1, p2, p3 (the tanh arguments).  cont: dict(F1, F23) to
    continue from (the device's); otherwise numpy's tanh.  plain_dot: the dot product without fma; regroup: the host-formed constants
    regrouped inside the expression ((c1/a1)*(betaStar*omega), sqrt(k)/betaStar, F1*psi1 + (1 - F1)*psi2) -- alternatives the CPU test looks at"""
    with np.errstate(all="ignore"):
        dot = (gk[0] * go[0] + gk[1] * go[1]) + gk[2] * go[2] if plain_dot else fma_v(gk[2], go[2], fma_v(gk[0], go[0], gk[1] * go[1]))
        CD = (S["twoAlphaOmega2"] * dot) / omega
        CDp = rmax_v(CD, 1.0e-10)
        y2, sk = y * y, np.sqrt(k)
        far = (500.0 * nu) / (y2 * omega)
        near = (sk / S["betaStar"]) / (omega * y) if regroup else (S["invBetaStar"] * sk) / (omega * y)
        third = (S["fourAlphaOmega2"] * k) / (CDp * y2)
        arg1 = rmin_v(rmin_v(rmax_v(near, far), third), 10.0)
        q1 = arg1 * arg1
        p1 = q1 * q1
        arg2, arg3, p2, p3, near2 = restate_f23(S, f3, k, omega, y, nu, regroup)
        if cont is None:
            F1 = np.tanh(p1)
            F23, t3 = f23_of(f3, p2, p3)
        else:
            F1, F23, t3 = cont["F1"], cont["F23"], cont.get("t3")
        if regroup:
            bl = lambda X: F1 * S[X + "1"] + (1.0 - F1) * S[X + "2"]
            cbo = (S["c1"] / S["a1"]) * (S["betaStar"] * omega)
        else:
            bl = lambda X: F1 * S["d" + X[0].upper() + X[1:]] + S[X + "2"]
            cbo = S["c1a1BetaStar"] * omega
        lim = rmax_v(S["a1"] * omega, (S["b1"] * F23) * np.sqrt(S2))
        out = dict(F1=F1, su=bl("gamma") * rmin_v(S2, cbo * lim), sp=bl("beta") * omega, susp=((F1 - 1.0) * CD) / omega,
                   domega=bl("alphaOmega") * nut + nu, dk=bl("alphaK") * nut + nu, CD=CD, arg1=arg1, arg2=arg2, arg3=arg3, F23=F23, t3=t3,
                   p1=p1, p2=p2, p3=p3)
        out.update(near=near, far=far, third=third, near2=near2)
    return out


def blend_arms(S, R, omega, S2):
    """which arm every max / min of mi_sst_blend takes, per cell, from its restated result R -> dict of masks"""
    with np.errstate(all="ignore"):
        m = rmax_v(R["near"], R["far"])
        inner = rmin_v(m, R["third"])
        m2 = rmax_v(R["near2"], R["far"])
        strain, a1o = (S["b1"] * R["F23"]) * np.sqrt(S2), S["a1"] * omega
        prod = (S["c1a1BetaStar"] * omega) * rmax_v(a1o, strain)
        return dict(arg1_near=(R["near"] > R["far"]) & (m < R["third"]) & (m < 10.0), arg1_far=~(R["near"] > R["far"]) & (m < R["third"]) & (m < 10.0),
                    arg1_third=~(m < R["third"]) & (R["third"] < 10.0), arg1_cap10=~(inner < 10.0),
                    arg2_near=(R["near2"] > R["far"]) & (m2 < 100.0), arg2_far=~(R["near2"] > R["far"]) & (m2 < 100.0), arg2_cap100=~(m2 < 100.0),
                    arg3_below=R["arg3"] < 10.0, arg3_cap10=~(R["arg3"] < 10.0),
                    cd_low=~(R["CD"] > 1.0e-10), cd_negative=R["CD"] < 0.0, cd_high=R["CD"] > 1.0e-10,
                    limiter_omega=a1o > strain, limiter_strain=~(a1o > strain), su_S2=S2 < prod, su_product=~(S2 < prod),
                    susp_positive=R["susp"] > 0.0, susp_negative=R["susp"] < 0.0)


def restate_omega_sources(V, su, sp, susp, omega, diag, source, sequential=False):
    """mi_sst_omega_sources.  sequential: fvm::Sp, then fvm::SuSp and the explicit part applied to the left side one after the other -- the
    grouping of mi_fvm_sp followed by mi_fvm_susp, which the CPU test shows to differ"""
    with np.errstate(all="ignore"):
        if sequential:
            return (diag + V * sp) + V * rmax_v(susp, 0.0), (source + V * su) - (V * rmin_v(susp, 0.0)) * omega
        return diag - ((-(V * sp)) - V * rmax_v(susp, 0.0)), source - ((-(V * su)) - (0.0 - (V * rmin_v(susp, 0.0)) * omega))


def restate_k_terms(S, G, k, omega, regroup=False):
    with np.errstate(all="ignore"):
        lim = S["c1"] * (S["betaStar"] * k) * omega if regroup else (S["c1BetaStar"] * k) * omega
        return rmin_v(G, lim), S["betaStar"] * omega


def restate_nut(S, f3, k, omega, y, s, nu, ctor=False, F23=None):
    """mi_sst_nut -> nut, F23 (numpy's tanh unless F23 is given), the tanh arguments p2, p3"""
    _, _, p2, p3, _ = restate_f23(S, f3, k, omega, y, nu)
    if F23 is None:
        F23, _ = f23_of(f3, p2, p3)
    with np.errstate(all="ignore"):
        strain = ((S["b1"] * F23) * math.sqrt(2.0)) * s if ctor else (S["b1"] * F23) * np.sqrt(s)
        return (S["a1"] * k) / rmax_v(S["a1"] * omega, strain), F23, p2, p3


# ---- the channel walk ----------------------------------------------------------------------------------------------------------------------------
SST_CHANNEL = dict(omega_in=250.0, alpha_omega=0.7, f3=False)


def channel(pkg):
    """turbulence_support.channel with what kOmegaSST needs: the face area vectors (for the Gauss gradients of k and omega), the distance of
    every cell centre to the nearest wall plane, seeded boundary values of gradU, and omega (a fixed value on the inlet)"""
    from turbulence_support import CHANNEL_DIMS, boundary_values
    u = pkg.synthetic.splitmix_uniform
    M, S0 = ke_channel(pkg)
    nx, ny, nz = CHANNEL_DIMS
    h, n, nb = 0.1, M["n"], M["nb"]
    step = M["up"].astype(np.int64) - M["lo"]
    Sf = [np.where(step == 1, h * h, 0.0), np.where(step == nx, h * h, 0.0), np.where(step == nx * ny, h * h, 0.0)]
    normal = {0: (1, -1.0), 1: (0, -1.0), 2: (1, 1.0), 3: (0, 1.0), 4: (2, -1.0), 5: (2, 1.0)}    # patch -> (axis, sign): ymin, xmin, ymax, xmax, zmin, zmax
    bSf = [np.zeros(nb) for _ in range(3)]
    for p, (axis, sign) in normal.items():
        bSf[axis][M["pid"] == p] = sign * h * h
    c = np.arange(n)
    j, kk = (c // nx) % ny, c // (nx * ny)
    y = h * np.minimum(np.minimum(j + 0.5, ny - j - 0.5), np.minimum(kk + 0.5, nz - kk - 0.5))
    M.update(SST_CHANNEL, S=coeffs(), Sf=Sf, bSf=bSf, y=y, bgrad=[5.0 * (u(3040 + i, nb) - 0.5) for i in range(9)])
    omega = M["omega_in"] * (0.8 + 0.4 * u(3030, n))
    return M, dict(k=S0["k"], bk=S0["bk"], omega=omega, bomega=boundary_values(M, omega, M["omega_in"]))


def restate_grad(orc, M, vf, bvf):
    """fvc::grad with the Gauss linear scheme -> the cell gradient [x, y, z] and its boundary values (gaussGrad.C:277-303:
    gb = g + n*(snGrad - (n & g)), n = Sf/magSf, snGrad = deltaCoeffs*(value - cell value))"""
    n, lo, up = M["n"], M["lo"], M["up"]
    bc = boundary_cells(M["L"])
    g = orc.gauss_grad(n, lo, up, M["Sf"], orc.face_interpolate(lo, up, M["lam"], vf), None)
    a = 0
    for fc, _ in M["L"]["patches"]:
        b = a + fc.shape[0]
        for d in range(3):
            g[d] = orc.patch_add_product(fc, M["bSf"][d][a:b], bvf[a:b], g[d], 0)
        a = b
    g = [x / M["V"] for x in g]
    nh = [M["bSf"][d] / M["bms"] for d in range(3)]
    sn = M["bdc"] * (bvf - vf[bc])
    gc = [g[d][bc] for d in range(3)]
    dd = sn - fma_v(nh[2], gc[2], fma_v(nh[0], gc[0], nh[1] * gc[1]))
    return g, [gc[d] + (nh[d] * dd) for d in range(3)]


def restate_nut_update(M, k, omega, bk, bomega, s, bs, blog, F23, bF23, ctor=False):
    """:466-467 (the constructor :287-296): nut on the cells and on every boundary face, then nutkWallFunction on the wall faces"""
    S, wall = M["S"], wall_mask(M["L"])
    nut, _, _, _ = restate_nut(S, M["f3"], k, omega, M["y"], s, M["nu"], ctor, F23)
    bnut, _, _, _ = restate_nut(S, M["f3"], bk, bomega, M["by"], bs, M["nu"], ctor, bF23)
    nutw, _, taken = restate_nut_wall(M["L"], wall_inputs(M, k, None), k, lg=blog)
    return nut, np.where(wall, nutw, bnut), taken


def restate_equation(orc, M, psi_old, psi, gamma, bgamma, inlet_value, alpha, sp_su=None, rhs=None, set_cells=None):
    """fvm::ddt + fvm::div - fvm::laplacian == the right-hand side, relax(alpha), [setValues on set_cells], and what the solver is given, through
    the oracle's sweeps.  sp_su = (sp, su): == su - fvm::Sp(sp) inside the assembly (the k equation); rhs = dict(su, sp, susp): the omega
    equation's right-hand side by restate_omega_sources on the assembled left side -> dict of every array"""
    from assembly_full_size import oracle_assemble
    n, lo, up = M["n"], M["lo"], M["up"]
    gam = orc.face_interpolate(lo, up, M["lam"], gamma) * M["magSf"]
    extra = {} if sp_su is None else dict(sp=(sp_su[0], 1.0), su=[(-1.0, [sp_su[1]])])
    a = oracle_assemble(orc, M, dict(vol=M["V"]), dict(rdt=1.0 / M["dt"], psi_old=[psi_old]), dict(flux=M["phi"], weights=M["lam"]),
                        dict(delta=M["dc"], gamma=gam), **extra)
    out = dict(gam=gam, upper0=a["upper"], lower0=a["lower"], diagL=a["diag"], sourceL=a["source0"])
    diag, source = a["diag"], a["source0"]
    if rhs is not None:
        diag, source = restate_omega_sources(M["V"], rhs["su"], rhs["sp"], rhs["susp"], psi, diag, source)
    out.update(diag0=diag, source0=source)
    fcs = [fc for fc, _ in M["L"]["patches"]]
    ic, bc = patch_coeffs(M, bgamma, inlet_value)
    diag, source = orc.relax(n, lo, up, alpha, diag, a["lower"], a["upper"], source, psi, fcs, ic, bc, [0] * len(fcs))
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


def restate_correct(orc, M, St, X):
    """kOmegaSST::correct() :412-467 from the state St (k, omega, nut and their boundary values) -> (every intermediate, the next state, the wall
    faces on the log branch).  X: what the restatement continues from -- the device's F1 / F23 on the cells and on the boundary faces, its
    log values and the two solutions of the engine's solver.  bS2: the boundary values of S2, from the seeded boundary gradU"""
    from turbulence_support import boundary_values
    S, L, nu, f3 = M["S"], M["L"], M["nu"], M["f3"]
    wall, W = wall_mask(L), wall_tables(L)
    S2, G, _ = restate_production(St["nut"], M["grad"])
    bS2, _, _ = restate_production(St["bnut"], M["bgrad"])
    G, omega, bom_w = restate_wall_cells(L, dict(wall_inputs(M, St["k"], St["bnut"]), S=S), G, St["omega"])
    bomega = np.where(wall, bom_w, St["bomega"])
    gk, bgk = restate_grad(orc, M, St["k"], St["bk"])
    go, bgo = restate_grad(orc, M, omega, bomega)
    B = restate_blend(S, f3, gk, go, St["k"], omega, M["y"], St["nut"], S2, nu, cont=dict(F1=X["F1"], F23=X["F23"]))
    Bb = restate_blend(S, f3, bgk, bgo, St["bk"], bomega, M["by"], St["bnut"], bS2, nu, cont=dict(F1=X["bF1"], F23=X["bF23"]))
    out = dict(S2=S2, bS2=bS2, G=G, omega_wall=omega, bomega_wall=bomega, CD=B["CD"], arg1=B["arg1"], bCD=Bb["CD"], barg1=Bb["arg1"],
               bdomega=Bb["domega"], bdk=Bb["dk"])
    out.update({"gradK%d" % d: gk[d] for d in range(3)}); out.update({"gradOmega%d" % d: go[d] for d in range(3)})
    out.update({"bgradK%d" % d: bgk[d] for d in range(3)}); out.update({"bgradOmega%d" % d: bgo[d] for d in range(3)})
    out.update({key: B[key] for key in ("su", "sp", "susp", "domega", "dk")})
    e = restate_equation(orc, M, St["omega"], omega, B["domega"], Bb["domega"], M["omega_in"], M["alpha_omega"],
                         rhs=dict(su=B["su"], sp=B["sp"], susp=B["susp"]), set_cells=W["cells"])
    out.update({"omega_" + key: v for key, v in e.items()})
    omega = X["omega_solved"]
    omega, bomega, out["omega_bounded"] = restate_bound_field(M, omega, boundary_values(M, omega, M["omega_in"]), SMALL)
    suk, spk = restate_k_terms(S, G, St["k"], omega)
    q = restate_equation(orc, M, St["k"], St["k"], B["dk"], Bb["dk"], M["k_in"], M["alpha_k"], sp_su=(spk, suk))
    out.update({"k_" + key: v for key, v in q.items()})
    out.update(su_k=suk, sp_k=spk, omega_new=omega, bomega_new=bomega)
    k = X["k_solved"]
    k, bk, out["k_bounded"] = restate_bound_field(M, k, boundary_values(M, k, M["k_in"]), SMALL)
    nut, bnut, taken = restate_nut_update(M, k, omega, bk, bomega, S2, bS2, X["blog"], X["nutF23"], X["bnutF23"])
    out.update(k_new=k, bk_new=bk, nut=nut, bnut=bnut)
    return out, dict(k=k, omega=omega, bk=bk, bomega=bomega, nut=nut, bnut=bnut), taken
