"""The Spalart-Allmaras model restated twice (RAS/SpalartAllmaras/SpalartAllmaras.C:45-137, :437-464; LES/SpalartAllmaras/SpalartAllmaras.C:45-172,
:331-357; SpalartAllmarasDDES.C:45-93; SpalartAllmarasIDDES.C:45-140; nutUSpaldingWallFunctionFvPatchScalarField.C:39-110):
literal loops over Python floats with an explicit fma, and vectorised numpy.  The kernels of csrc/spalart.inc are compared with the vectorised
form bit for bit; a CPU test shows that the two forms agree and that the inputs reach every arm.

Rounding: every field operator on its own; fma in magSqr(Vector) (3.5s), magSqr(SymmTensor) (3.5o), magSqr(Tensor) of skew(gradU) and in the
Newton step of the wall functor.  max(a, b) = (a > b) ? a : b; min(a, b) = (a < b) ? a : b; pos(x) = x >= 0; neg(x) = x < 0.  pow, tanh and exp
are the library's: the restatement takes the values to continue from (`cont`) and returns the argument of each, so that a test can hold the
device's value to numpy's ON THE SAME ARGUMENT and everything after it bit for bit."""
import math

import numpy as np

from interface_support import div, fma, fma_v
from komegasst_support import TANH_BOUND, rmin, rmin_v
from turbulence_support import POW_LOG_BOUND, boundary_cells, rmax, rmax_v, wall_mask

SMALL, ROOTVSMALL = 1e-15, 1e-150
EXP_BOUND = 5 * 2.0 ** -52                  # relative; the OpenCL full-profile bound for exp (3 ulp) plus 2 for the host's libm
KINDS = ("RAS", "DES", "DDES", "IDDES")
MODEL = ("sigmaNut", "kappa", "Cb1", "Cb2", "Cw2", "Cw3", "Cv1", "Cv2", "CDES", "ck", "fwStar", "cl", "ct")
MODEL_DEFAULTS = (0.66666, 0.41, 0.1355, 0.622, 0.3, 2.0, 7.1, 5.0, 0.65, 0.07, 0.424, 3.55, 1.63)
WALL = ("wallKappa", "E")
WALL_DEFAULTS = (0.41, 9.8)
DERIVED = ("Cw1", "Cb2BySigmaNut", "Cv1_3", "Cw3_6", "onePlusCw3_6", "invCv2", "ct2", "cl2", "psiDen", "psiCoeff", "invE", "sqrt2")
# the library calls of each kind, in the order of the entry's optional outputs, with the bar each is held to
TRANSCENDENTALS = dict(RAS=("pow_fw",), DES=("pow_fw",), DDES=("pow_fw", "tanh_fd"),
                       IDDES=("pow_fw", "tanh_fd", "exp", "pow_hill_pos", "pow_hill_neg", "tanh_ft", "pow_fl", "tanh_fl"))
BOUNDS = dict(pow_fw=POW_LOG_BOUND, tanh_fd=TANH_BOUND, exp=EXP_BOUND, pow_hill_pos=POW_LOG_BOUND, pow_hill_neg=POW_LOG_BOUND, tanh_ft=TANH_BOUND,
              pow_fl=POW_LOG_BOUND, tanh_fl=TANH_BOUND)
OUTPUTS = ("su_grad", "su_prod", "sp", "dnu", "fv1", "s", "dtilda", "stilda")


def coeffs(**given):
    """the literal host formulas of mi_sa_coeffs_init"""
    K = dict(zip(MODEL + WALL, MODEL_DEFAULTS + WALL_DEFAULTS))
    K.update(given)
    kappa2 = K["kappa"] * K["kappa"]
    K["Cw1"] = K["Cb1"] / kappa2 + (1.0 + K["Cb2"]) / K["sigmaNut"]
    K["Cb2BySigmaNut"] = K["Cb2"] / K["sigmaNut"]
    K["Cv1_3"] = K["Cv1"] * (K["Cv1"] * K["Cv1"])
    c2 = K["Cw3"] * K["Cw3"]
    K["Cw3_6"] = c2 * (c2 * c2)
    K["onePlusCw3_6"] = 1.0 + K["Cw3_6"]
    K["invCv2"] = 1 / K["Cv2"]
    K["ct2"], K["cl2"] = K["ct"] * K["ct"], K["cl"] * K["cl"]
    K["psiDen"] = (K["Cw1"] * kappa2) * K["fwStar"]
    K["psiCoeff"] = K["Cb1"] / K["psiDen"]
    K["invE"] = 1 / K["E"]
    K["sqrt2"] = math.sqrt(2.0)
    return K


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def inputs(syn, L, seed):
    """nuTilda log-uniform over 1e-7..1e-2 (chi from 0.01 to 1000 at nu = 1e-5) and exactly 0 in a seventh of the cells, more than half of which also have
    gradU == 0 (STilda == 0 under the Ashford correction); y over 1e-4..1, delta and hmax over 1e-3..0.3, nuSgs over 1e-6..1e-3: the ranges
    are chosen so that every arm of every max / min / pos / neg is taken by a share of the cells (asserted by the CPU test).  The wall arrays:
    velocities up to 10, y over 1e-5..0.1, nutw over 1e-8..0.1 with zeros, Uw == U[c] exactly on every seventh boundary face"""
    u = syn.splitmix_uniform
    n = L["n"]
    bc = boundary_cells(L)
    nb = bc.shape[0]
    lg = lambda s, lo, hi, m=n: np.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * u(seed + s, m))
    nt = lg(0, 1e-7, 1e-2)
    pick = u(seed + 1, n)
    nt[pick < 0.14] = 0.0
    grad = [20.0 * (u(seed + 2 + i, n) - 0.5) for i in range(9)]
    for g in grad:
        g[pick < 0.08] = 0.0
    gnt = [1e-2 * (u(seed + 11 + i, n) - 0.5) for i in range(3)]
    F = dict(nt=nt, grad=grad, gnt=gnt, y=lg(14, 1e-4, 1.0), nu=1e-5, nu_f=1e-5 * (0.5 + u(seed + 15, n)), delta=lg(16, 1e-3, 0.3),
             nusgs=lg(17, 1e-6, 1e-3), hmax=lg(18, 1e-3, 0.3), V=0.5 + u(seed + 19, n), diag=1.0 + u(seed + 20, n), source=u(seed + 21, n) - 0.5)
    U = [20.0 * (u(seed + 30 + d, n) - 0.5) for d in range(3)]
    Uw = [0.2 * (u(seed + 33 + d, nb) - 0.5) for d in range(3)]
    for d in range(3):
        Uw[d][::7] = U[d][bc[::7]]
    bnutw = lg(36, 1e-8, 1e-1, nb)
    bnutw[::5] = 0.0
    F["wall"] = dict(U=U, Uw=Uw, bdc=20.0 + 130.0 * u(seed + 37, nb), by=lg(38, 1e-5, 1e-1, nb), bnuw=1e-5 * (0.5 + u(seed + 39, nb)), bnutw=bnutw)
    return F


# ---- the cell pass, vectorised -------------------------------------------------------------------------------------------------------------------
def p3(s):
    return s * (s * s)


def p6(s):
    return p3(s * s)


def mag_skew_v(g, contracted=True):
    xy, xz, yx = 0.5 * (g[1] - g[3]), 0.5 * (g[2] - g[6]), 0.5 * (g[3] - g[1])
    yz, zx, zy = 0.5 * (g[5] - g[7]), 0.5 * (g[6] - g[2]), 0.5 * (g[7] - g[5])
    if not contracted:
        return np.sqrt(xy * xy + xz * xz + yx * yx + yz * yz + zx * zx + zy * zy)
    s = xy * xy
    for t in (xz, yx, yz, zx, zy):
        s = fma_v(t, t, s)
    return np.sqrt(s)


def mag_symm_v(g):
    xx, xy, xz, yx, yy, yz, zx, zy, zz = g
    sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
    s = fma_v(xx, xx, 2.0 * (sxy * sxy))
    s = fma_v(2.0, sxz * sxz, s)
    s = fma_v(yy, yy, s)
    s = fma_v(2.0, syz * syz, s)
    s = fma_v(zz, zz, s)
    return np.sqrt(s)


def rd_v(K, visc, S, ky2):
    return rmin_v(visc / (rmax_v(S, SMALL) * ky2 + ROOTVSMALL), 10.0)


def restate_terms(K, kind, ash, F, nu=None, cont=None, alt=()):
    """mi_sa_terms -> dict of the outputs (OUTPUTS), every library value (TRANSCENDENTALS[kind]), its argument ("arg_" + name) and the arm
    masks ("arm_" + name).  cont: dict of library values to continue from (the device's); otherwise numpy's.  alt: names of alternatives the
    CPU test shows to change a compared bit -- "skew_plain", "magsqr_plain", "fv2_other", "chibycv2_other", "stilda_other", "r_other" (the
    RAS form in an LES kind and the reverse), "cb2_regroup", "psi_regroup", "cw1_regroup" """
    cont = {} if cont is None else cont
    nt, g, gn, y = F["nt"], F["grad"], F["gnt"], F["y"]
    nu = F["nu"] if nu is None else nu
    ras = kind == "RAS"
    lib = lambda name, f, arg: (np.asarray(cont[name], dtype=np.float64) if name in cont else f(arg))
    R = {}
    with np.errstate(all="ignore"):
        chi = nt / nu
        chi3 = p3(chi)
        fv1 = chi3 / (chi3 + K["Cv1_3"])
        key = "_symm" if kind == "DDES" else ("_skew_plain" if "skew_plain" in alt else "_skew")
        if key not in F:                                         # the fma loops are slow: once per set of inputs
            F[key] = mag_symm_v(g) if kind == "DDES" else mag_skew_v(g, "skew_plain" not in alt)
        magG = F[key]
        S = K["sqrt2"] * magG
        ras_fv2 = ras != ("fv2_other" in alt)
        ras_c = ras != ("chibycv2_other" in alt)
        if ash:
            t = 1.0 + chi / K["Cv2"] if ras_fv2 else 1.0 + nt / (K["Cv2"] * nu)
            fv2 = 1.0 / p3(t)
            c = K["invCv2"] * chi if ras_c else chi / K["Cv2"]
            t3 = 1.0 + c
            fv3 = (((1.0 + chi * fv1) * K["invCv2"]) * (3.0 * t3 + c * c)) / p3(t3)
        else:
            fv2 = 1.0 - chi / (1.0 + chi * fv1)
            fv3 = np.ones_like(chi)
        ky = K["kappa"] * y
        ky2 = ky * ky
        dT = y
        if kind == "DES":
            cd = K["CDES"] * F["delta"]
            dT = rmin_v(cd, y)
            R["arm_des_delta"] = cd < y
        elif kind == "DDES":
            a = p3(8.0 * rd_v(K, F["nusgs"] + nu, S, ky2))
            th = lib("tanh_fd", np.tanh, a)
            fd = 1.0 - th
            inner = y - K["CDES"] * F["delta"]
            dT = rmax_v(y - fd * rmax_v(inner, 0.0), SMALL)
            R.update(tanh_fd=th, arg_tanh_fd=a, fd=fd, arm_ddes_inner=inner > 0.0, arm_fd_low=fd < 0.01, arm_fd_high=fd > 0.99)
        elif kind == "IDDES":
            nuSgs = F["nusgs"]
            raw = 0.25 - y / F["hmax"]
            alpha = rmax_v(raw, -5.0)
            a2 = alpha * alpha
            e = lib("exp", np.exp, a2)
            p1 = lib("pow_hill_pos", lambda x: np.power(x, -11.09), e)
            p2 = lib("pow_hill_neg", lambda x: np.power(x, -9.0), e)
            fHill = 2.0 * (np.where(alpha >= 0, 1.0, 0.0) * p1 + np.where(alpha < 0, 1.0, 0.0) * p2)
            fStep = rmin_v(2.0 * p2, 1.0)
            a = p3(8.0 * rd_v(K, nuSgs + nu, S, ky2))
            th = lib("tanh_fd", np.tanh, a)
            fd = 1.0 - th
            fHyb = rmax_v(1.0 - fd, fStep)
            at = p3(K["ct2"] * rd_v(K, nuSgs, S, ky2))
            ft = lib("tanh_ft", np.tanh, at)
            al = K["cl2"] * rd_v(K, nu, S, ky2)
            p10 = lib("pow_fl", lambda x: np.power(x, 10.0), al)
            fl = lib("tanh_fl", np.tanh, p10)
            fAmp = 1.0 - rmax_v(ft, fl)
            fRestore = rmax_v(fHill - 1.0, 0.0) * fAmp
            if "psi_regroup" in alt:
                q = (1.0 - (K["Cb1"] * fv2) / K["psiDen"]) / rmax_v(SMALL, fv1)
            else:
                q = (1.0 - K["psiCoeff"] * fv2) / rmax_v(SMALL, fv1)
            Psi = np.sqrt(rmin_v(100.0, q))
            dT = rmax_v(SMALL, (fHyb * (1.0 + fRestore * Psi)) * y + (((1.0 - fHyb) * K["CDES"]) * Psi) * F["delta"])
            R.update(tanh_fd=th, arg_tanh_fd=a, exp=e, arg_exp=a2, pow_hill_pos=p1, arg_pow_hill_pos=e, pow_hill_neg=p2, arg_pow_hill_neg=e,
                     tanh_ft=ft, arg_tanh_ft=at, pow_fl=p10, arg_pow_fl=al, tanh_fl=fl, arg_tanh_fl=p10, fd=fd,
                     arm_fd_low=fd < 0.01, arm_fd_high=fd > 0.99, arm_alpha_pos=alpha >= 0, arm_alpha_cap=~(raw > -5.0), arm_fstep_cap=~(2.0 * p2 < 1.0),
                     arm_fhyb_fd=(1.0 - fd) > fStep, arm_ft_over_fl=ft > fl, arm_fhill=(fHill - 1.0) > 0.0, arm_psi_cap=100.0 < q,
                     arm_fv1_small=SMALL > fv1)
        kd = K["kappa"] * dT
        kd2 = kd * kd
        ras_st = ras != ("stilda_other" in alt)
        ST = ((fv3 * K["sqrt2"]) * magG if ras_st else fv3 * S) + (fv2 * nt) / kd2
        den = rmax_v(ST, SMALL) * kd2
        if ras == ("r_other" in alt):
            den = den + ROOTVSMALL
        raw_r = nt / den
        r = rmin_v(raw_r, 10.0)
        gg = r + K["Cw2"] * (p6(r) - r)
        apw = K["onePlusCw3_6"] / (p6(gg) + K["Cw3_6"])
        pw = lib("pow_fw", lambda x: np.power(x, 1.0 / 6.0), apw)
        fw = gg * pw
        if "_m" not in F:
            F["_m"] = fma_v(gn[2], gn[2], fma_v(gn[0], gn[0], gn[1] * gn[1]))
        m = F["_m"] if "magsqr_plain" not in alt else gn[0] * gn[0] + gn[1] * gn[1] + gn[2] * gn[2]
        R["su_grad"] = (K["Cb2"] * m) / K["sigmaNut"] if "cb2_regroup" in alt else K["Cb2BySigmaNut"] * m
        R["su_prod"] = (K["Cb1"] * ST) * nt
        R["sp"] = (K["Cw1"] * (fw * nt)) / (dT * dT) if "cw1_regroup" in alt else ((K["Cw1"] * fw) * nt) / (dT * dT)
        R["dnu"] = (nt + nu) / K["sigmaNut"]
    R.update(fv1=fv1, s=S, dtilda=dT * np.ones_like(nt), stilda=ST, pow_fw=pw, arg_pow_fw=apw, fv2=fv2, fv3=fv3, r=r,
             arm_r_cap=~(raw_r < 10.0), arm_st_small=~(ST > SMALL), arm_ashford=np.full(nt.shape, bool(ash)))
    return R


def arms_of(kind, ash):
    """the arms mi_sa_terms can take with positive inputs, per kind: name -> (the mask's key, reached on both sides?)"""
    a = ["arm_r_cap", "arm_st_small"]
    if kind == "DES":
        a += ["arm_des_delta"]
    if kind == "DDES":
        a += ["arm_ddes_inner", "arm_fd_low", "arm_fd_high"]
    if kind == "IDDES":
        a += ["arm_fd_low", "arm_fd_high", "arm_alpha_pos", "arm_alpha_cap", "arm_fstep_cap", "arm_fhyb_fd", "arm_ft_over_fl", "arm_fhill", "arm_psi_cap",
              "arm_fv1_small"]
    return a


# ---- the cell pass, literal ------------------------------------------------------------------------------------------------------------------------
def _mag_skew(g):
    xy, xz, yx = 0.5 * (g[1] - g[3]), 0.5 * (g[2] - g[6]), 0.5 * (g[3] - g[1])
    yz, zx, zy = 0.5 * (g[5] - g[7]), 0.5 * (g[6] - g[2]), 0.5 * (g[7] - g[5])
    s = xy * xy
    for t in (xz, yx, yz, zx, zy):
        s = fma(t, t, s)
    return math.sqrt(s)


def _mag_symm(g):
    xx, xy, xz, yx, yy, yz, zx, zy, zz = g
    sxy, sxz, syz = 0.5 * (xy + yx), 0.5 * (xz + zx), 0.5 * (yz + zy)
    s = fma(xx, xx, 2.0 * (sxy * sxy))
    s = fma(2.0, sxz * sxz, s)
    s = fma(yy, yy, s)
    s = fma(2.0, syz * syz, s)
    s = fma(zz, zz, s)
    return math.sqrt(s)


def _rd(K, visc, S, ky2):
    return rmin(div(visc, rmax(S, SMALL) * ky2 + ROOTVSMALL), 10.0)


def literal_terms(K, kind, ash, F, T, nu=None):
    """cell by cell on Python floats; T: the library values to continue from (the restatement's) -> dict of OUTPUTS"""
    n = F["nt"].shape[0]
    nu = F["nu"] if nu is None else nu
    nuv = nu.tolist() if isinstance(nu, np.ndarray) else [nu] * n
    G = [x.tolist() for x in F["grad"]]
    GN = [x.tolist() for x in F["gnt"]]
    col = {key: F[key].tolist() for key in ("nt", "y", "delta", "nusgs", "hmax")}
    Tl = {key: np.asarray(v).tolist() for key, v in T.items()}
    out = {key: [] for key in OUTPUTS}
    for i in range(n):
        nt, y, v = col["nt"][i], col["y"][i], nuv[i]
        g = [G[k][i] for k in range(9)]
        chi = div(nt, v)
        chi3 = chi * (chi * chi)
        fv1 = div(chi3, chi3 + K["Cv1_3"])
        magG = _mag_symm(g) if kind == "DDES" else _mag_skew(g)
        S = K["sqrt2"] * magG
        if ash:
            t = 1.0 + div(chi, K["Cv2"]) if kind == "RAS" else 1.0 + div(nt, K["Cv2"] * v)
            fv2 = div(1.0, t * (t * t))
            c = K["invCv2"] * chi if kind == "RAS" else div(chi, K["Cv2"])
            t3 = 1.0 + c
            fv3 = div(((1.0 + chi * fv1) * K["invCv2"]) * (3.0 * t3 + c * c), t3 * (t3 * t3))
        else:
            fv2 = 1.0 - div(chi, 1.0 + chi * fv1)
            fv3 = 1.0
        ky = K["kappa"] * y
        ky2 = ky * ky
        dT = y
        if kind == "DES":
            dT = rmin(K["CDES"] * col["delta"][i], y)
        elif kind == "DDES":
            fd = 1.0 - Tl["tanh_fd"][i]
            dT = rmax(y - fd * rmax(y - K["CDES"] * col["delta"][i], 0.0), SMALL)
        elif kind == "IDDES":
            alpha = rmax(0.25 - div(y, col["hmax"][i]), -5.0)
            p1, p2 = Tl["pow_hill_pos"][i], Tl["pow_hill_neg"][i]
            fHill = 2.0 * ((1.0 if alpha >= 0 else 0.0) * p1 + (1.0 if alpha < 0 else 0.0) * p2)
            fStep = rmin(2.0 * p2, 1.0)
            fd = 1.0 - Tl["tanh_fd"][i]
            fHyb = rmax(1.0 - fd, fStep)
            fAmp = 1.0 - rmax(Tl["tanh_ft"][i], Tl["tanh_fl"][i])
            fRestore = rmax(fHill - 1.0, 0.0) * fAmp
            Psi = math.sqrt(rmin(100.0, div(1.0 - K["psiCoeff"] * fv2, rmax(SMALL, fv1))))
            dT = rmax(SMALL, (fHyb * (1.0 + fRestore * Psi)) * y + (((1.0 - fHyb) * K["CDES"]) * Psi) * col["delta"][i])
        kd = K["kappa"] * dT
        kd2 = kd * kd
        ST = ((fv3 * K["sqrt2"]) * magG if kind == "RAS" else fv3 * S) + div(fv2 * nt, kd2)
        den = rmax(ST, SMALL) * kd2
        if kind != "RAS":
            den = den + ROOTVSMALL
        r = rmin(div(nt, den), 10.0)
        r2 = r * r
        gg = r + K["Cw2"] * (r2 * (r2 * r2) - r)
        fw = gg * Tl["pow_fw"][i]
        gn = [GN[k][i] for k in range(3)]
        out["su_grad"].append(K["Cb2BySigmaNut"] * fma(gn[2], gn[2], fma(gn[0], gn[0], gn[1] * gn[1])))
        out["su_prod"].append((K["Cb1"] * ST) * nt)
        out["sp"].append(div((K["Cw1"] * fw) * nt, dT * dT))
        out["dnu"].append(div(nt + v, K["sigmaNut"]))
        out["fv1"].append(fv1); out["s"].append(S); out["dtilda"].append(dT); out["stilda"].append(ST)
    return {key: np.array(v, dtype=np.float64) for key, v in out.items()}


def restate_nut(K, nt, fv1=None, nu=None):
    """mi_sa_nut -> nut, fv1: the stored fv1, or recomputed from nuTilda and nu"""
    with np.errstate(all="ignore"):
        if fv1 is None:
            chi3 = p3(nt / nu)
            fv1 = chi3 / (chi3 + K["Cv1_3"])
        return fv1 * nt, fv1


def restate_sources(V, diag, source, su_grad, su_prod, sp, summed=False):
    """the equation's grouping (fvMatrix.C:2731-2756, :2773-2800, :2208-2216): diag + V*sp; (source + V*su_grad) + V*su_prod.  summed:
    source + V*(su_grad + su_prod), which the CPU test shows to differ"""
    if summed:
        return diag + V * sp, source + V * (su_grad + su_prod)
    return diag + V * sp, (source + V * su_grad) + V * su_prod


# ---- the wall function ------------------------------------------------------------------------------------------------------------------------------
def _mag3_v(a):
    return np.sqrt(fma_v(a[2], a[2], fma_v(a[0], a[0], a[1] * a[1])))


def restate_wall(L, K, W, ev=None, contracted=True):
    """mi_sa_nut_spalding_wall -> dict(nut per boundary face (the input off the walls), exp (nb, 10; NaN where no step was taken), iters per
    boundary face (-1 off the walls), arg: the argument kUu of every exp, errs: every err compared with 0.01, uts: every ut compared with ROOTVSMALL, capped: kUu == 50 taken,
    zero: the ut0 <= ROOTVSMALL arm).  ev: the exp values to continue from; contracted False: every operator of the functor rounded"""
    bc, wall = boundary_cells(L), wall_mask(L)
    nb = bc.shape[0]
    wf = np.nonzero(wall)[0]
    c = bc[wf]
    kappa, invE = K["wallKappa"], K["invE"]
    with np.errstate(all="ignore"):
        d = [W["U"][k][c] - W["Uw"][k][wf] for k in range(3)]
        sn = [W["bdc"][wf] * (W["Uw"][k][wf] - W["U"][k][c]) for k in range(3)]
        magUp, mgu = _mag3_v(d), _mag3_v(sn)
        y, nuw = W["by"][wf], W["bnuw"][wf]
        ut = np.sqrt((W["bnutw"][wf] + nuw) * mgu)
        started = ut > ROOTVSMALL
        active = started.copy()
        taken = np.zeros(wf.shape[0], dtype=np.int32)
        E, ARG = np.full((nb, 10), np.nan), np.full((nb, 10), np.nan)
        errs, uts, capped = [], [ut.copy()], np.zeros(wf.shape[0], dtype=bool)
        kM, yn = kappa * magUp, y / nuw
        for it in range(10):
            i = np.nonzero(active)[0]
            if i.shape[0] == 0:
                break
            u0 = ut[i]
            q = kM[i] / u0
            kUu = rmin_v(q, 50.0)
            capped[i] |= ~(q < 50.0)
            e = np.exp(kUu) if ev is None else ev[wf[i], it]
            E[wf[i], it] = e
            ARG[wf[i], it] = kUu
            if contracted:
                fk = fma_v(-kUu, fma_v(kUu, 0.5, 1.0), e - 1.0)
                f = fma_v(invE, fma_v(-(1.0 / 6.0) * kUu, kUu * kUu, fk), magUp[i] / u0 - (u0 * y[i]) / nuw[i])
            else:
                fk = e - 1.0 - kUu * (1.0 + 0.5 * kUu)
                f = -(u0 * y[i]) / nuw[i] + magUp[i] / u0 + invE * (fk - ((1.0 / 6.0) * kUu) * (kUu * kUu))
            df = (magUp[i] / (u0 * u0) + yn[i]) + ((invE * kUu) * fk) / u0
            new = u0 + f / df
            err = np.abs((u0 - new) / u0)
            ut[i] = new
            taken[i] += 1
            errs.append(err); uts.append(new)
            active[i] = (new > ROOTVSMALL) & (err > 0.01)
        uTau = np.where(started, rmax_v(0.0, ut), 0.0)
        nutw = rmax_v(0.0, (uTau * uTau) / (mgu + ROOTVSMALL) - nuw)
    nut, iters = W["bnutw"].copy(), np.full(nb, -1, dtype=np.int32)
    nut[wf], iters[wf] = nutw, taken
    return dict(nut=nut, exp=E, arg=ARG, iters=iters, errs=np.concatenate(errs) if errs else np.zeros(0), uts=np.concatenate(uts), capped=capped,
                zero=~started, mgu=mgu)


def literal_wall(L, K, W, ev):
    """face by face on Python floats, continuing from the exp values ev (nb, 10) -> nut, iters as restate_wall"""
    bc, wall = boundary_cells(L), wall_mask(L)
    kappa, invE = K["wallKappa"], K["invE"]
    nut, iters = W["bnutw"].copy(), np.full(bc.shape[0], -1, dtype=np.int32)
    col = lambda a: a.tolist()
    U, Uw = [col(x) for x in W["U"]], [col(x) for x in W["Uw"]]
    bdc, by, bnuw, bnutw = col(W["bdc"]), col(W["by"]), col(W["bnuw"]), col(W["bnutw"])
    mag = lambda a: math.sqrt(fma(a[2], a[2], fma(a[0], a[0], a[1] * a[1])))
    for bf in np.nonzero(wall)[0].tolist():
        c = int(bc[bf])
        magUp = mag([U[k][c] - Uw[k][bf] for k in range(3)])
        mgu = mag([bdc[bf] * (Uw[k][bf] - U[k][c]) for k in range(3)])
        y, nuw = by[bf], bnuw[bf]
        ut = math.sqrt((bnutw[bf] + nuw) * mgu)
        uTau, taken = 0.0, 0
        if ut > ROOTVSMALL:
            it = 0
            while True:
                kUu = rmin(div(kappa * magUp, ut), 50.0)
                e = float(ev[bf, taken])
                taken += 1
                fk = fma(-kUu, fma(kUu, 0.5, 1.0), e - 1.0)
                f = fma(invE, fma(-(1.0 / 6.0) * kUu, kUu * kUu, fk), div(magUp, ut) - div(ut * y, nuw))
                df = (div(magUp, ut * ut) + div(y, nuw)) + div((invE * kUu) * fk, ut)
                new = ut + div(f, df)
                err = abs(div(ut - new, ut))
                ut = new
                if not (ut > ROOTVSMALL and err > 0.01):
                    break
                it += 1
                if not it < 10:
                    break
            uTau = rmax(0.0, ut)
        nut[bf] = rmax(0.0, div(uTau * uTau, mgu + ROOTVSMALL) - nuw)
        iters[bf] = taken
    return nut, iters


def within(dev, ref, bound):
    """|dev - ref| <= bound*|ref| where ref is finite; NaN and infinities at the same places"""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(ref)
    same_special = np.array_equal(np.isnan(dev), np.isnan(ref)) and np.array_equal(dev[~ok & ~np.isnan(ref)], ref[~ok & ~np.isnan(ref)])
    if not np.any(ok):
        return same_special, 0.0
    with np.errstate(all="ignore"):
        rel = np.where(ref[ok] != 0.0, np.abs(dev[ok] - ref[ok]) / np.abs(ref[ok]), np.where(dev[ok] == 0.0, 0.0, np.inf))
    worst = float(rel.max())
    return same_special and worst <= bound, worst


# ---- the channel walk ----------------------------------------------------------------------------------------------------------------------------
SA_CHANNEL = dict(nt_in=5e-4, alpha_nt=0.8)


def channel(pkg):
    """komegasst_support.channel (the 6 x 5 x 4 channel with its face area vectors, the cells' wall distance y and seeded boundary values of
    gradU) with what Spalart-Allmaras adds: seeded delta and hmax on the cells and on the boundary faces (the caller's arrays, as y is), and
    nuTilda with a fixed value on the inlet and zero gradient elsewhere -> M, the initial state"""
    from komegasst_support import channel as sst_channel
    from turbulence_support import boundary_values
    u = pkg.synthetic.splitmix_uniform
    M, _ = sst_channel(pkg)
    n, nb = M["n"], M["nb"]
    M.update(SA_CHANNEL, SA=coeffs(), delta=0.1 * (0.3 + u(3050, n)), bdelta=0.1 * (0.3 + u(3051, nb)), hmax=0.1 * (0.5 + u(3052, n)),
             bhmax=0.1 * (0.5 + u(3053, nb)))
    nt = M["nt_in"] * (0.8 + 0.4 * u(3054, n))
    return M, dict(nt=nt, bnt=boundary_values(M, nt, M["nt_in"]))


def channel_wall(M, bnut):
    return dict(U=M["U"], Uw=M["Uw"], bdc=M["bdc"], by=M["by"], bnuw=M["bnuw"], bnutw=bnut)


def restate_channel_nut(M, nt, bnt, bnut_old, ev, fv1=None, bfv1=None):
    """nut / nuSgs = fv1*nuTilda on the cells and on the boundary faces (fv1 stored, or recomputed from nu), then nutUSpaldingWallFunction on the
    wall faces, which read their OWN earlier value -> nut, bnut, the wall function's restatement"""
    K, wall = M["SA"], wall_mask(M["L"])
    nut, _ = restate_nut(K, nt, fv1=fv1, nu=M["nu"])
    bcalc, _ = restate_nut(K, bnt, fv1=bfv1, nu=M["nu"])
    W = restate_wall(M["L"], K, channel_wall(M, np.where(wall, bnut_old, bcalc)), ev=ev)
    return nut, W["nut"], W


def restate_channel_constructor(M, St, X):
    """updateSubGridScaleFields() of the LES classes (LES/SpalartAllmaras.C:45-49, :310), and for the RAS class the viscosity line :426, from
    a boundary nut of zero -> the state with nut and bnut"""
    nut, bnut, _ = restate_channel_nut(M, St["nt"], St["bnt"], np.zeros(M["nb"]), X["ev"])
    return dict(St, nut=nut, bnut=bnut)


def restate_channel_correct(orc, M, kind, ash, St, X):
    """correct() of one model from the state St (nuTilda, nut and their boundary values) -> (every intermediate, the next state).  X: what the
    restatement continues from -- the device's library values on the cells (lib) and on the boundary faces (blib), the solution of the
    engine's solver (nt_solved) and the wall function's exp values (ev)"""
    from assembly_full_size import oracle_assemble
    from komegasst_support import restate_grad
    from turbulence_support import boundary_values, patch_coeffs, restate_bound_field
    K, L, nu = M["SA"], M["L"], M["nu"]
    n, lo, up = M["n"], M["lo"], M["up"]
    g, bg = restate_grad(orc, M, St["nt"], St["bnt"])
    F = dict(nt=St["nt"], grad=M["grad"], gnt=g, y=M["y"], nu=nu, delta=M["delta"], nusgs=St["nut"], hmax=M["hmax"])
    Fb = dict(nt=St["bnt"], grad=M["bgrad"], gnt=bg, y=M["by"], nu=nu, delta=M["bdelta"], nusgs=St["bnut"], hmax=M["bhmax"])
    R, Rb = restate_terms(K, kind, ash, F, cont=X["lib"]), restate_terms(K, kind, ash, Fb, cont=X["blib"])
    out = {"gradNt%d" % d: g[d] for d in range(3)}
    out.update({"bgradNt%d" % d: bg[d] for d in range(3)})
    out.update({key: R[key] for key in OUTPUTS})
    out.update({"b" + key: Rb[key] for key in OUTPUTS})
    gam = orc.face_interpolate(lo, up, M["lam"], R["dnu"]) * M["magSf"]
    terms = (dict(vol=M["V"]), dict(rdt=1.0 / M["dt"], psi_old=[St["nt"]]), dict(flux=M["phi"], weights=M["lam"]), dict(delta=M["dc"], gamma=gam))
    left = oracle_assemble(orc, M, *terms)
    a = oracle_assemble(orc, M, *terms, sp=(R["sp"], 1.0), su=[(-1.0, [R["su_grad"]]), (-1.0, [R["su_prod"]])])
    out.update(gam=gam, upper0=a["upper"], lower0=a["lower"], diagL=left["diag"], sourceL=left["source0"], diag0=a["diag"], source0=a["source0"])
    fcs = [fc for fc, _ in L["patches"]]
    ic, bc = patch_coeffs(M, Rb["dnu"], M["nt_in"])
    diag, source = orc.relax(n, lo, up, M["alpha_nt"], a["diag"], a["lower"], a["upper"], a["source0"], St["nt"], fcs, ic, bc, [0] * len(fcs))
    ds, ss = diag, source
    for fc, i, b in zip(fcs, ic, bc):
        ds = orc.patch_add(fc, i, ds, 0); ss = orc.patch_add(fc, b, ss, 0)
    out.update(diag1=diag, source1=source, ic=np.concatenate(ic), bc=np.concatenate(bc), diag_solve=ds, source_solve=ss)
    nt = X["nt_solved"]
    nt, bnt, out["bounded"] = restate_bound_field(M, nt, boundary_values(M, nt, M["nt_in"]), 0.0)
    stored = kind == "RAS"                              # RAS :463 takes the fv1 of before the solve; the LES classes recompute it (:45-49)
    nut, bnut, W = restate_channel_nut(M, nt, bnt, St["bnut"], X["ev"], fv1=R["fv1"] if stored else None, bfv1=Rb["fv1"] if stored else None)
    out.update(nt_new=nt, bnt_new=bnt, nut=nut, bnut=bnut, iters=W["iters"])
    return out, dict(nt=nt, bnt=bnt, nut=nut, bnut=bnut)
