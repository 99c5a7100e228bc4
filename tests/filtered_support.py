"""Restatements shared by tests/test_filtered_schemes.py and tests/test_cubic_scheme.py, written from the comment blocks of
include/mi_ldu.h (the filtered centred limiters; the explicit correction of `Gauss cubic`).  The yardstick is numpy: one array operation
per field operator, so nothing is contracted but what is written as an fma (exact rational arithmetic, one rounding).  Beside it a
scalar-by-scalar second restatement of either family, for the hand-computed semantics cases and as a cross-check of the first.

Restated, not pinned by compiled reference functors: the reference's headers are not compiled into a fixture."""
import numpy as np

import test_limited_schemes as tl
from assembly_support import fma, fma_each, rmax, rmin

SMALL = 1e-15                                                   # doubleScalar.H
VSMALL = 1e-300
# (scheme name, kernel kind, V form, number of coefficients): the five names the reference registers
FILTERED = (("filteredLinear", 0, False, 0), ("filteredLinear2", 1, False, 2), ("filteredLinear2V", 1, True, 2),
            ("filteredLinear3", 2, False, 1), ("filteredLinear3V", 2, True, 1))
BRANCHES = ("fl2_df_pos", "fl2_df_nonpos", "fl2_all_zero", "fl2_starts_at_2", "k_zero", "fl3_small", "fl3_clamp_0", "fl_floor", "fl_one",
            "zero_flux")


def schemes():
    """(scheme string, name, kind, vec, k, l) over all five names, k in {1, 0.33, 0}, l in {0, 0.5, 1}"""
    out = []
    for name, kind, vec, ncoef in FILTERED:
        for k in ((1.0, 0.33, 0.0) if ncoef >= 1 else (None,)):
            for l in ((0.0, 0.5, 1.0) if ncoef == 2 else (None,)):
                out.append((" ".join([name] + [repr(x) for x in (k, l) if x is not None]), name, kind, vec, k, l))
    return out


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def vmax(a, b):
    """the reference's max on arrays: (a > b) ? a : b"""
    return np.where(a > b, a, b)


def vmin(a, b):
    return np.where(a < b, a, b)


def dot_each(a, b):
    """Vector & Vector per face, contracted as every face pass: fma(az, bz, fma(ax, bx, ay*by))"""
    return fma_each(a[2], b[2], fma_each(a[0], b[0], a[1] * b[1]))


def face_differences(vec, pP, pN, gP, gN, d):
    """-> (df, dcP, dcN) per face.  Scalar: df = phiN - phiP, dc = d & gradc.  V: dfV = phiN - phiP, df = dfV & dfV,
    dc = dfV & (d & gradc), component j of the inner product d & grad(phi_j) (g[3*j + k] = d(phi_j)/dx_k)"""
    if not vec:
        return pN[0] - pP[0], dot_each(d, gP[:3]), dot_each(d, gN[:3])
    dfV = [pN[j] - pP[j] for j in range(3)]
    inner = lambda g: [dot_each(d, g[3 * j:3 * j + 3]) for j in range(3)]
    return dot_each(dfV, dfV), dot_each(dfV, inner(gP)), dot_each(dfV, inner(gN))


def limiter_each(kind, vec, k, l, df, dcP, dcN, hit=lambda key, n=1: None):
    """the limiter of a kind (0 filteredLinear, 1 filteredLinear2[V], 2 filteredLinear3[V]) from the face differences; one numpy operation
    per operator, left to right as the header parenthesises"""
    count = lambda key, mask: hit(key, int(np.count_nonzero(mask)))
    with np.errstate(all="ignore"):
        if kind == 0:
            lim = 2 - (0.5 * vmin(np.abs(df - dcP), np.abs(df - dcN))) / (vmax(np.abs(dcP), np.abs(dcN)) + SMALL)
            out = vmax(vmin(lim, 1.0), 0.8)
            count("fl_floor", out == 0.8); count("fl_one", out == 1.0)
            return out
        tP, tN = 2 * dcP, 2 * dcN
        count("k_zero", np.full(df.shape, k == 0))
        if kind == 1:
            pos = df > 0
            m = np.where(pos, vmin(vmax(df - tP, 0.0), vmax(df - tN, 0.0)), vmin(vmax(tP - df, 0.0), vmax(tN - df, 0.0)))
            lim = (l + 1.0) - (k * m) / (vmax(np.abs(df), vmax(np.abs(tP), np.abs(tN))) + (VSMALL if vec else SMALL))
            out = vmax(vmin(lim, 1.0), 0.0)
            count("fl2_df_pos", pos); count("fl2_df_nonpos", ~pos)
            zero = (df == 0) & (tP == 0) & (tN == 0)
            assert np.all(out[zero] == 1.0)
            count("fl2_all_zero", zero); count("fl2_starts_at_2", lim == 2.0)
            return out
        den = vmax((tN + tP) * (tN + tP), SMALL)
        lim = 1 - ((k * (tN - df)) * (tP - df)) / den
        out = vmax(vmin(lim, 1.0), 0.0)
        count("fl3_small", den == SMALL); count("fl3_clamp_0", lim < 0)
        return out


def weights_each(lim, cdw, flux):
    """limitedSurfaceInterpolationSchemeWeightsFunctor: fma(lim, cdw, (1 - lim)*pos(flux)), pos(): >= 0"""
    return fma_each(lim, cdw, (1.0 - lim) * (flux >= 0).astype(np.float64))


class Differences:
    """the face differences of one set of inputs, formed once and shared by every coefficient pair of a kind: scalar and V form"""

    def __init__(self, pP, pN, gP, gN, d):
        self.form = {False: face_differences(False, pP[:1], pN[:1], gP[:3], gN[:3], d), True: face_differences(True, pP, pN, gP, gN, d)}

    def weights(self, kind, vec, k, l, cdw, flux, hit=lambda key, n=1: None):
        """-> (weights, limiter)"""
        lim = limiter_each(kind, vec, k, l, *self.form[vec], hit=hit)
        hit("zero_flux", int(np.count_nonzero(flux == 0)))
        return weights_each(lim, cdw, flux), lim


def internal_differences(lo, up, phi, grad, Cc):
    """the internal faces: d = C[N] - C[P]; phi 3 cell arrays, grad 9"""
    return Differences([p[lo] for p in phi], [p[up] for p in phi], [g[lo] for g in grad], [g[up] for g in grad], [c[up] - c[lo] for c in Cc])


def patch_differences(fc, phi, nbr_phi, grad, nbr_grad, pd):
    """one coupled patch (LimitedScheme.C:145-195): phiP / gradcP through faceCells, phiN / gradcN the patchNeighbourField, d = patch delta"""
    return Differences([p[fc] for p in phi], list(nbr_phi), [g[fc] for g in grad], list(nbr_grad), list(pd))


class HitCount(tl.Hits):
    """Hits with a count per call; a count of zero records nothing"""

    def __call__(self, key, n=1):
        if n:
            self.n[key] = self.n.get(key, 0) + n


# ---- the scalar-by-scalar second restatement ---------------------------------------------------------------------------------------
def limiter_face(name, k, l, pP, pN, gP, gN, d):
    """one face, from the reference headers' expressions; pP, pN scalars (3-lists for the V names), gP, gN 3 (9) components"""
    if name.endswith("V"):
        dfV = [pN[j] - pP[j] for j in range(3)]
        df = tl.dot(dfV, dfV)
        dcP, dcN = tl.dot(dfV, tl.d_and_grad(d, gP)), tl.dot(dfV, tl.d_and_grad(d, gN))
    else:
        df = pN - pP
        dcP, dcN = tl.dot(d, gP), tl.dot(d, gN)
    if name == "filteredLinear":
        lim = 2 - 0.5 * rmin(abs(df - dcP), abs(df - dcN)) / (rmax(abs(dcP), abs(dcN)) + SMALL)
        return rmax(rmin(lim, 1), 0.8)
    tP, tN = 2 * dcP, 2 * dcN
    if name.startswith("filteredLinear2"):
        l_ = l + 1.0
        small = VSMALL if name.endswith("V") else SMALL
        if df > 0:
            lim = l_ - k * rmin(rmax(df - tP, 0), rmax(df - tN, 0)) / (rmax(abs(df), rmax(abs(tP), abs(tN))) + small)
        else:
            lim = l_ - k * rmin(rmax(tP - df, 0), rmax(tN - df, 0)) / (rmax(abs(df), rmax(abs(tP), abs(tN))) + small)
        return rmax(rmin(lim, 1), 0)
    assert name.startswith("filteredLinear3")
    s = tN + tP
    lim = 1 - k * (tN - df) * (tP - df) / rmax(s * s, SMALL)
    return rmax(rmin(lim, 1), 0)


# ---- cubic -------------------------------------------------------------------------------------------------------------------------
def cubic_coeffs(lam):
    """cubic.H:121-127, each field operator rounded on its own"""
    kSc = lam * (1 - lam * (3 - 2 * lam))
    kVecP = ((1 - lam) * (1 - lam)) * lam
    kVecN = (lam * lam) * (lam - 1)
    return kSc, kVecP, kVecN


def cubic_close(c0, gI, geo, flux):
    corr = c0 + ((dot_each(gI, geo["sf"]) / geo["mag_sf"]) / geo["dc"])
    return corr if flux is None else flux * corr


def cubic_internal(lo, up, geo, vf, grads, flux=None):
    """[faceFlux *] correction(vf) on the internal faces: geo dict(lam, sf[3], mag_sf, dc), vf one cell array per component, grads one
    [gx, gy, gz] per component.  The interpolate functor contracts its first product"""
    kSc, kP, kN = cubic_coeffs(geo["lam"])
    out = []
    for v, g in zip(vf, grads):
        c0 = fma_each(kSc, v[lo], (-kSc) * v[up])
        gI = [fma_each(kP, g[k][lo], kN * g[k][up]) for k in range(3)]
        out.append(cubic_close(c0, gI, geo, flux))
    return out


def cubic_patch(fc, geo, vf, nbr_vf, grads, nbr_grads, flux=None):
    """one coupled patch: field operators, two rounded products and a sum; only the dot product is contracted"""
    kSc, kP, kN = cubic_coeffs(geo["lam"])
    out = []
    for v, nv, g, ng in zip(vf, nbr_vf, grads, nbr_grads):
        c0 = kSc * v[fc] + (-kSc) * nv
        gI = [kP * g[k][fc] + kN * ng[k] for k in range(3)]
        out.append(cubic_close(c0, gI, geo, flux))
    return out


def cubic_face(lam, vP, vN, gP, gN, sf, mag_sf, dc, flux=None):
    """the second restatement, one internal face and one component"""
    kSc = lam * (1 - lam * (3 - 2 * lam))
    kVecP = (1 - lam) * (1 - lam) * lam
    kVecN = lam * lam * (lam - 1)
    c0 = fma(kSc, vP, -kSc * vN)
    gI = [fma(kVecP, gP[k], kVecN * gN[k]) for k in range(3)]
    corr = c0 + tl.dot(gI, sf) / mag_sf / dc
    return corr if flux is None else flux * corr


def cubic_geometry(pkg, m, seed):
    """face geometry of m faces for the bitwise tests: lambda in (0.3, 0.7), Sf of both signs, magSf = |Sf| as numpy rounds it, deltaCoeffs"""
    u = pkg.synthetic.splitmix_uniform
    sf = [u(seed + 1 + k, m) - 0.5 for k in range(3)]
    return dict(lam=0.3 + 0.4 * u(seed, m), sf=sf, mag_sf=np.sqrt(sf[0] * sf[0] + sf[1] * sf[1] + sf[2] * sf[2]) + 0.01, dc=0.5 + 3.0 * u(seed + 4, m))
