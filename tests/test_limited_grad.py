"""The limited gradient schemes cellLimited / cellMDLimited / faceLimited / faceMDLimited (finiteVolume/gradSchemes/limitedGradSchemes/*).

Two independent restatements of the four calcGrad bodies (cellLimitedGrads.C, cellMDLimitedGrads.C, faceLimitedGrads.C,
faceMDLimitedGrads.C): `literal`, the reference's loops transcribed line for line (face loop scattering to both cells, then the patches),
and `restate`, the same arithmetic vectorised over cells with a loop over each cell's face slots in the order the face loop reaches them.
No fma anywhere: the reference's loops are host code, every expression is rounded operation by operation as written, which
is what numpy and Python floats do.  The engine's row pass (mi_limited_grad) must equal them bit for bit (gpu)."""
import os
import subprocess

import numpy as np
import pytest

from assembly_support import ROW_MODES, bits, gpu_env, rmax, rmin, same, set_row_blocks, set_row_tables, shape_case, shaped_addressing, signed_flux

SMALL, VSMALL = 1e-15, 1e-300                                   # doubleScalar.H:57-58
KINDS = ("cellLimited", "cellMDLimited", "faceLimited", "faceMDLimited")
OTHER, COUPLED, FIXES = 0, 1, 2                                  # MI_GRAD_PATCH_*


def vmax(a, b):
    return np.where(a > b, a, b)


def vmin(a, b):
    return np.where(a < b, a, b)


def dot_uncontracted(a, b):
    """Vector & Vector uncontracted: (ax*bx + ay*by) + az*bz"""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


# ---- the reference's loops, line for line ---------------------------------------------------------------------------------------------
def literal(kind, k, lo, up, C, Cf, vf, grad, patches):
    """kind in KINDS, k the coefficient; C [n][3], Cf [nf][3] as lists; vf [n][nc]; grad [n][3*nc] (grad[c][3*j + i] = d(vf_j)/dx_i);
    patches: [(kind, faceCells, values [m][nc] (patchNeighbourField or boundary values), pCf [m][3])].  -> (grad, limiter or None)"""
    n, nc = len(vf), len(vf[0])
    g = [list(x) for x in grad]
    if k < SMALL:
        return g, None
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    gj = lambda c, j: g[c][3 * j:3 * j + 3]

    def md(c, j, maxD, minD, dcf):                              # cellMDLimitedGrad<scalar>::limitFace on component j's gradient
        gi = gj(c, j)
        e = dot_uncontracted(dcf, gi)
        if e > maxD:
            t = maxD - e
        elif e < minD:
            t = minD - e
        else:
            return
        m = dot_uncontracted(dcf, dcf)
        g[c][3 * j:3 * j + 3] = [gi[i] + dcf[i] * t / m for i in range(3)]

    def lf(lim, maxD, minD, e):                                  # cellLimitedGrad<scalar>::limitFace
        if e > maxD + VSMALL:
            return rmin(lim, maxD / e)
        if e < minD - VSMALL:
            return rmin(lim, minD / e)
        return lim

    rk = 1.0 / k - 1.0
    if kind in ("cellLimited", "cellMDLimited"):
        mx = [list(v) for v in vf]
        mn = [list(v) for v in vf]
        for f in range(len(lo)):
            o, nb = lo[f], up[f]
            for j in range(nc):
                mx[o][j] = rmax(mx[o][j], vf[nb][j]); mn[o][j] = rmin(mn[o][j], vf[nb][j])
                mx[nb][j] = rmax(mx[nb][j], vf[o][j]); mn[nb][j] = rmin(mn[nb][j], vf[o][j])
        for _, fc, val, _ in patches:
            for i, o in enumerate(fc):
                for j in range(nc):
                    mx[o][j] = rmax(mx[o][j], val[i][j]); mn[o][j] = rmin(mn[o][j], val[i][j])
        for c in range(n):
            for j in range(nc):
                mx[c][j] = mx[c][j] - vf[c][j]; mn[c][j] = mn[c][j] - vf[c][j]
                if k < 1.0:
                    t = rk * (mx[c][j] - mn[c][j])
                    mx[c][j] = mx[c][j] + t; mn[c][j] = mn[c][j] - t
        order = []                                             # (cell, face centre) of every limitFace call, in the loops' order
        for f in range(len(lo)):
            order += [(lo[f], Cf[f]), (up[f], Cf[f])]
        for _, fc, _, pcf in patches:
            order += [(o, pcf[i]) for i, o in enumerate(fc)]
        if kind == "cellLimited":
            lim = [[1.0] * nc for _ in range(n)]
            for c, cf in order:
                d = sub(cf, C[c])
                for j in range(nc):
                    lim[c][j] = lf(lim[c][j], mx[c][j], mn[c][j], dot_uncontracted(d, gj(c, j)))
            for c in range(n):
                g[c] = [g[c][3 * j + i] * lim[c][j] for j in range(nc) for i in range(3)]
            return g, lim
        for c, cf in order:
            d = sub(cf, C[c])
            for j in range(nc):
                md(c, j, mx[c][j], mn[c][j], d)
        return g, None
    # face kinds
    lim = [1.0] * n
    expand_md = k < 1.0
    for f in range(len(lo)):
        o, nb = lo[f], up[f]
        if kind == "faceLimited" and nc == 3:
            gradf = [dot_uncontracted(sub(Cf[f], C[o]), gj(o, j)) for j in range(3)]
            sO, sN = dot_uncontracted(gradf, vf[o]), dot_uncontracted(gradf, vf[nb])
            mxF, mnF = rmax(sO, sN), rmin(sO, sN)
            t = rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t
            lim[o] = lf(lim[o], mxF - sO, mnF - sO, dot_uncontracted(gradf, gradf))
            gradf = [dot_uncontracted(sub(Cf[f], C[nb]), gj(nb, j)) for j in range(3)]
            sO, sN = dot_uncontracted(gradf, vf[o]), dot_uncontracted(gradf, vf[nb])
            mxF, mnF = rmax(sO, sN), rmin(sO, sN)                     # faceLimitedGrads.C:241-254: not expanded
            lim[nb] = lf(lim[nb], mxF - sN, mnF - sN, dot_uncontracted(gradf, gradf))
            continue
        for j in range(nc):
            vO, vN = vf[o][j], vf[nb][j]
            mxF, mnF = rmax(vO, vN), rmin(vO, vN)
            if kind == "faceLimited" or expand_md:
                t = rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t
            if kind == "faceLimited":
                lim[o] = lf(lim[o], mxF - vO, mnF - vO, dot_uncontracted(sub(Cf[f], C[o]), gj(o, j)))
                lim[nb] = lf(lim[nb], mxF - vN, mnF - vN, dot_uncontracted(sub(Cf[f], C[nb]), gj(nb, j)))
            else:
                md(o, j, mxF - vO, mnF - vO, sub(Cf[f], C[o]))
                md(nb, j, mxF - vN, mnF - vN, sub(Cf[f], C[nb]))
    for pk, fc, val, pcf in patches:
        if pk == OTHER:
            continue
        for i, o in enumerate(fc):
            d = sub(pcf[i], C[o])
            if kind == "faceLimited" and nc == 3:
                gradf = [dot_uncontracted(d, gj(o, j)) for j in range(3)]
                sO, sN = dot_uncontracted(gradf, vf[o]), dot_uncontracted(gradf, val[i])
                mxF, mnF = rmax(sO, sN), rmin(sO, sN)
                t = rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t
                lim[o] = lf(lim[o], mxF - sO, mnF - sO, dot_uncontracted(gradf, gradf))
                continue
            for j in range(nc):
                vO, vN = vf[o][j], val[i][j]
                mxF, mnF = rmax(vO, vN), rmin(vO, vN)
                if kind == "faceLimited" or expand_md:
                    t = rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t
                if kind == "faceLimited":
                    lim[o] = lf(lim[o], mxF - vO, mnF - vO, dot_uncontracted(d, gj(o, j)))
                else:
                    md(o, j, mxF - vO, mnF - vO, d)
    if kind == "faceLimited":
        for c in range(n):
            g[c] = [x * lim[c] for x in g[c]]
        return g, [[x] for x in lim]
    return g, None


# ---- the same, vectorised over cells ----------------------------------------------------------------------------------------------------
class Slots:
    """every cell's faces in the order the reference's loops reach them: internal faces ascending (each seen from its owner and its
    neighbour), then the boundary faces by patch and face.  Event e < 2*nf: face e // 2 seen from its owner (e even) or neighbour (odd);
    e >= 2*nf: boundary face e - 2*nf.  start[c]:start[c + 1] are cell c's events, in that order."""

    def __init__(self, n, lo, up, bcell, face_kind_mask=None):
        nf = lo.shape[0]
        cells = np.empty(2 * nf + bcell.shape[0], dtype=np.int32)
        cells[0:2 * nf:2] = lo; cells[1:2 * nf:2] = up; cells[2 * nf:] = bcell
        keep = np.ones(cells.shape[0], bool)
        if face_kind_mask is not None:
            keep[2 * nf:] = face_kind_mask
        ev = np.nonzero(keep)[0]
        order = np.argsort(cells[ev], kind="stable")           # stable: ascending event number within a cell
        self.ev = ev[order].astype(np.int64)
        cnt = np.bincount(cells[ev], minlength=n)
        self.start = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=self.start[1:])
        self.S = int(cnt.max()) if n else 0
        self.nf = nf

    def slot(self, s):
        """-> (cells, event) of the cells that have an s-th face"""
        idx = self.start[:-1] + s
        c = np.nonzero(idx < self.start[1:])[0]
        return c, self.ev[idx[c]]


def _face_data(sl, c, e, lo, up, C, Cf, bcf, vf, bv):
    """dcf = Cf - C[c], the values across the face, c owns the face (internal owner side or boundary)"""
    nf = sl.nf
    internal = e < 2 * nf
    f = np.where(internal, e // 2, 0)
    b = np.where(internal, 0, e - 2 * nf)
    isOwner = internal & (e % 2 == 0)
    own = ~internal | isOwner
    other = np.where(isOwner, up[f], lo[f])
    d = [np.where(internal, Cf[i][f], bcf[i][b] if bcf is not None else 0.0) - C[i][c] for i in range(3)]
    w = [np.where(internal, vf[j][other], bv[j][b] if bv is not None else 0.0) for j in range(len(vf))]
    return d, w, own


def _lf(lim, m, maxD, minD, e):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c1 = m & (e > maxD + VSMALL)
        c2 = m & ~c1 & (e < minD - VSMALL)
        return np.where(c1, vmin(lim, maxD / e), np.where(c2, vmin(lim, minD / e), lim))


def _md(gi, m, maxD, minD, d):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = dot_uncontracted(d, gi)
        c1 = m & (e > maxD)
        c2 = m & ~c1 & (e < minD)
        t = np.where(c1, maxD - e, minD - e)
        msq = dot_uncontracted(d, d)
        u = c1 | c2
        return [np.where(u, gi[i] + d[i] * t / msq, gi[i]) for i in range(3)]


def restate(kind, k, n, lo, up, C, Cf, vf, grad, bcell=None, bkind=None, bv=None, bcf=None):
    """vectorised restatement: vf nc arrays [n], grad 3*nc arrays, boundary faces in patch order: bcell, bkind (per face), bv nc arrays,
    bcf 3 arrays.  -> (grad, limiter arrays or None)"""
    nc = len(vf)
    g = [np.array(x, dtype=np.float64) for x in grad]
    if k < SMALL:
        return g, None
    bcell = np.zeros(0, np.int32) if bcell is None else np.asarray(bcell, np.int32)
    face_kind = kind in ("faceLimited", "faceMDLimited")
    sl = Slots(n, lo, up, bcell, (np.asarray(bkind) != OTHER) if face_kind and bcell.shape[0] else None)
    rk = 1.0 / k - 1.0
    v = [np.asarray(x) for x in vf]
    if not face_kind:
        mx = [x.copy() for x in v]; mn = [x.copy() for x in v]
        for s in range(sl.S):
            c, e = sl.slot(s)
            _, w, _ = _face_data(sl, c, e, lo, up, C, Cf, bcf, v, bv)
            for j in range(nc):
                mx[j][c] = vmax(mx[j][c], w[j]); mn[j][c] = vmin(mn[j][c], w[j])
        for j in range(nc):
            mx[j] = mx[j] - v[j]; mn[j] = mn[j] - v[j]
            if k < 1.0:
                t = rk * (mx[j] - mn[j]); mx[j] = mx[j] + t; mn[j] = mn[j] - t
        lim = [np.ones(n) for _ in range(nc)]
        for s in range(sl.S):
            c, e = sl.slot(s)
            d, _, _ = _face_data(sl, c, e, lo, up, C, Cf, bcf, v, None)
            m = np.ones(c.shape[0], bool)
            for j in range(nc):
                gi = [g[3 * j + i][c] for i in range(3)]
                if kind == "cellLimited":
                    lim[j][c] = _lf(lim[j][c], m, mx[j][c], mn[j][c], dot_uncontracted(d, gi))
                else:
                    gi = _md(gi, m, mx[j][c], mn[j][c], d)
                    for i in range(3):
                        g[3 * j + i][c] = gi[i]
        if kind == "cellMDLimited":
            return g, None
        return [g[3 * j + i] * lim[j] for j in range(nc) for i in range(3)], lim
    lim = np.ones(n)
    for s in range(sl.S):
        c, e = sl.slot(s)
        d, w, own = _face_data(sl, c, e, lo, up, C, Cf, bcf, v, bv)
        m = np.ones(c.shape[0], bool)
        if kind == "faceLimited" and nc == 3:
            gf = [dot_uncontracted(d, [g[3 * j + i][c] for i in range(3)]) for j in range(3)]
            sc, so = dot_uncontracted(gf, [x[c] for x in v]), dot_uncontracted(gf, w)
            sO, sN = np.where(own, sc, so), np.where(own, so, sc)
            mxF, mnF = vmax(sO, sN), vmin(sO, sN)
            t = rk * (mxF - mnF)
            mxF, mnF = np.where(own, mxF + t, mxF), np.where(own, mnF - t, mnF)
            lim[c] = _lf(lim[c], m, mxF - sc, mnF - sc, dot_uncontracted(gf, gf))
            continue
        for j in range(nc):
            vc = v[j][c]
            pO, pN = np.where(own, vc, w[j]), np.where(own, w[j], vc)
            mxF, mnF = vmax(pO, pN), vmin(pO, pN)
            if kind == "faceLimited" or k < 1.0:
                t = rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t
            gi = [g[3 * j + i][c] for i in range(3)]
            if kind == "faceLimited":
                lim[c] = _lf(lim[c], m, mxF - vc, mnF - vc, dot_uncontracted(d, gi))
            else:
                gi = _md(gi, m, mxF - vc, mnF - vc, d)
                for i in range(3):
                    g[3 * j + i][c] = gi[i]
    if kind == "faceMDLimited":
        return g, None
    return [x * lim for x in g], [lim]


# ---- meshes: geometry, boundary patches, fields -----------------------------------------------------------------------------------------
def box_mesh(syn, dims):
    """the uniform box with its six wall patches (x-, x+, y-, y+, z-, z+), face centres on the boundary planes"""
    nx, ny, nz = dims
    case = syn.box_case(*dims)
    lo, up, n = case.lower_addr, case.upper_addr, case.n_cells
    h = 1.0 / nx
    c = np.arange(n)
    i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
    C = [(i + 0.5) * h, (j + 0.5) * h, (k + 0.5) * h]
    Cf = [0.5 * (x[lo] + x[up]) for x in C]
    fcs, pcf = [], []
    for ax, (idx, m) in enumerate(((i, nx), (j, ny), (k, nz))):
        for side in (0, m - 1):
            fc = np.nonzero(idx == side)[0].astype(np.int32)
            p = [C[q][fc].copy() for q in range(3)]
            p[ax] = np.full(fc.shape[0], 0.0 if side == 0 else m * h)
            fcs.append(fc); pcf.append(p)
    return dict(n=n, lo=lo, up=up, C=C, Cf=Cf, fcs=fcs, pcf=pcf, kinds=[FIXES] * 6)


def skewed(dims):
    """test_assembly.skewed_mesh with its patches given the three kinds in turn (coupled, fixesValue, other)"""
    from test_assembly import skewed_mesh
    M = skewed_mesh(dims)
    G, nI = M["G"], M["nI"]
    fcs, pcf, kinds = [], [], []
    for q, (name, ptype, cnt, start) in enumerate(M["patches"]):
        fcs.append(M["owner"][start:start + cnt].astype(np.int32))
        pcf.append([np.ascontiguousarray(G["Cf"][start:start + cnt, d]) for d in range(3)])
        kinds.append((COUPLED, FIXES, OTHER)[q % 3])
    return dict(n=M["n"], lo=M["lo"], up=M["up"], C=[np.ascontiguousarray(G["C"][:, d]) for d in range(3)],
                Cf=[np.ascontiguousarray(G["Cf"][:nI, d]) for d in range(3)], fcs=fcs, pcf=pcf, kinds=kinds)


def random_geometry(syn, n, lo, up, seed, n_patches=3):
    """seeded centres and a few patches of random cells (every kind) for a graph without geometry"""
    u = syn.splitmix_uniform
    C = [u(seed + d, n) for d in range(3)]
    Cf = [u(seed + 10 + d, lo.shape[0]) for d in range(3)]
    fcs, pcf = [], []
    for p in range(n_patches):
        m = max(1, n // 7)
        fc = np.sort((u(seed + 20 + p, m) * n).astype(np.int32))
        fcs.append(fc); pcf.append([u(seed + 30 + 3 * p + d, m) for d in range(3)])
    return dict(n=n, lo=lo, up=up, C=C, Cf=Cf, fcs=fcs, pcf=pcf, kinds=[COUPLED, FIXES, OTHER][:n_patches])


def graph_mesh(pkg, n=1500, seed=11):
    from conftest import random_graph_case
    case = random_graph_case(pkg, n, extra=2.5, seed=seed)
    return random_geometry(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, 40)


def fields(syn, M, nc, seed, gscale=40.0):
    """cell values with exact zeros of both signs, steep gradients (most cells limited), boundary values"""
    u = syn.splitmix_uniform
    n = M["n"]
    vf = []
    for j in range(nc):
        x = u(seed + j, n) - 0.5
        x[::5] = 0.0
        x[2::7] = -0.0
        vf.append(x)
    grad = [gscale * (u(seed + 10 + i, n) - 0.5) for i in range(3 * nc)]
    nb = sum(f.shape[0] for f in M["fcs"])
    bv = [u(seed + 30 + j, nb) - 0.5 for j in range(nc)]
    for x in bv:
        x[1::6] = -0.0
    return vf, grad, bv


def boundary_flat(M):
    """the patch-ordered concatenation: cells, kind per face, face centres"""
    fcs = M["fcs"]
    bcell = np.concatenate(fcs) if fcs else np.zeros(0, np.int32)
    bkind = np.concatenate([np.full(f.shape[0], k) for f, k in zip(fcs, M["kinds"])]) if fcs else np.zeros(0, int)
    bcf = [np.concatenate([p[d] for p in M["pcf"]]) for d in range(3)] if fcs else None
    return bcell, bkind, bcf


def literal_inputs(M, vf, grad, bv):
    n, nc = M["n"], len(vf)
    C = [[M["C"][d][c] for d in range(3)] for c in range(n)]
    Cf = [[M["Cf"][d][f] for d in range(3)] for f in range(M["lo"].shape[0])]
    V = [[vf[j][c] for j in range(nc)] for c in range(n)]
    G = [[grad[i][c] for i in range(3 * nc)] for c in range(n)]
    patches, off = [], 0
    for fc, kd, p in zip(M["fcs"], M["kinds"], M["pcf"]):
        m = fc.shape[0]
        patches.append((kd, fc.tolist(), [[bv[j][off + i] for j in range(nc)] for i in range(m)], [[p[d][i] for d in range(3)] for i in range(m)]))
        off += m
    return M["lo"].tolist(), M["up"].tolist(), C, Cf, V, G, patches


def run_restate(kind, k, M, vf, grad, bv):
    bcell, bkind, bcf = boundary_flat(M)
    return restate(kind, k, M["n"], M["lo"], M["up"], M["C"], M["Cf"], vf, grad, bcell, bkind, bv, bcf)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ["0", "1e-16", "0.5", "1"])
def test_parse_accepts(pkg, kind, k):
    eng = pkg.engine
    lim = eng.grad_limiter(f"{kind} Gauss linear {k}")
    assert lim.kind == KINDS.index(kind)
    assert lim.k == float(k)
    assert lim.identity == (1 if float(k) < SMALL else 0)
    assert eng.grad_limiter(f"  {kind}\tGauss  linear\n{k} ").k == float(k)


@pytest.mark.parametrize("scheme, why", [
    ("cellLimitedd Gauss linear 1", "unknown"),
    ("limitedLinear Gauss linear 1", "unknown"),
    ("Gauss linear", "unknown"),
    ("cellLimited leastSquares 1", "base"),
    ("faceLimited fourth 0.5", "base"),
    ("cellLimited Gauss upwind 1", "interpolation"),
    ("cellMDLimited Gauss pointLinear 1", "interpolation"),
    ("cellLimited cellLimited Gauss linear 1 1", "limited scheme over a limited"),
    ("faceMDLimited faceLimited Gauss linear 0.5 1", "limited scheme over a limited"),
    ("cellLimited", "base gradient"),
    ("cellLimited Gauss", "interpolation"),
    ("cellLimited Gauss linear", "coefficient"),
    ("cellLimited Gauss linear 1 2", "extra"),
    ("cellLimited Gauss linear one", "not a number"),
    ("cellLimited Gauss linear 1.5", "should be >= 0 and <= 1"),
    ("faceLimited Gauss linear -0.1", "should be >= 0 and <= 1"),
    ("faceMDLimited Gauss linear nan", "should be >= 0 and <= 1"),
    ("", "empty"),
])
def test_parse_refuses(pkg, scheme, why):
    eng = pkg.engine
    with pytest.raises(eng.MiError, match=why):
        eng.grad_limiter(scheme)


def test_exports(pkg):
    lib = pkg.engine.lib()
    for name in ("mi_grad_limiter_parse", "mi_grad_boundary_create", "mi_grad_boundary_destroy", "mi_limited_grad"):
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "Foam::fv::limitedGradScheme::New(" in syms
    assert syms.count("Foam::fvc::limitedGrad(") == 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nc", [1, 3])
def test_restatement_leaves_the_gradient_of_a_linear_field(pkg, kind, nc):
    """exact gradient of a linear field on the box, boundary values on the walls: nothing is limited, limiter 1 everywhere (spacing 1/8
    and dyadic coefficients: every centre, value and extrapolate is exact, so no face overshoots its bound by a rounding)"""
    M = box_mesh(pkg.synthetic, (8, 6, 5))
    a = [np.array([0.5, -0.25, 0.75]), np.array([-1.0, 0.5, 0.25]), np.array([0.125, 1.0, -0.5])][:nc]
    vf = [dot_uncontracted(M["C"], x) for x in a]
    bcf = boundary_flat(M)[2]
    bv = [dot_uncontracted(bcf, x) for x in a]
    grad = [np.full(M["n"], x[i]) for x in a for i in range(3)]
    for k in (1.0, 0.5):
        g, lim = run_restate(kind, k, M, vf, grad, bv)
        for x, y in zip(g, grad):
            assert same(x, y)
        if lim is not None:
            assert all(np.all(x == 1.0) for x in lim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nc", [1, 3])
def test_restatement_equals_the_literal_loops(pkg, kind, nc):
    """the vectorised restatement against the reference's loops transcribed line for line, on all three meshes; limiters in [0, 1]"""
    syn = pkg.synthetic
    for M in (box_mesh(syn, (5, 4, 3)), skewed((5, 4, 3)), graph_mesh(pkg, 200, 5)):
        vf, grad, bv = fields(syn, M, nc, 3 + nc)
        for k in (1.0, 0.5, 0.0):
            g, lim = run_restate(kind, k, M, vf, grad, bv)
            gl, liml = literal(kind, k, *literal_inputs(M, vf, grad, bv))
            for i in range(3 * nc):
                assert same(g[i], [row[i] for row in gl]), (kind, k, i)
            if k == 1.0 and kind.endswith("MDLimited"):
                assert not all(same(x, y) for x, y in zip(g, grad))   # the data reach the limiter
            if lim is None:
                assert liml is None
                continue
            for j in range(len(lim)):
                assert same(lim[j], [row[j] for row in liml]), (kind, k, j)
                assert np.all((lim[j] >= 0) & (lim[j] <= 1))
            if k == 1.0:
                assert np.any(lim[0] < 1)


def test_face_limited_vector_keeps_the_neighbour_side_bounds_unexpanded():
    """two cells, one face, k = 0.5: the owner's bounds are expanded by rk*(max - min), the neighbour's are not
    (faceLimitedGrads.C:241-254), so only the neighbour is limited"""
    lo, up = np.array([0], np.int32), np.array([1], np.int32)
    C = [np.array([0.0, 1.0]), np.zeros(2), np.zeros(2)]
    Cf = [np.array([0.5]), np.zeros(1), np.zeros(1)]
    vf = [np.array([0.0, 1.0]), np.zeros(2), np.zeros(2)]
    # both cells: d(U_x)/dx = 4, i.e. the face value extrapolated from either cell overshoots by 1
    grad = [np.full(2, 4.0)] + [np.zeros(2) for _ in range(8)]
    g, lim = restate("faceLimited", 0.5, 2, lo, up, C, Cf, vf, grad)
    # owner: gradf = 2, vsf = (0, 2), bounds [0 - 2, 2 + 2] - 0 -> extrapolate magSqr = 4 is inside: limiter 1
    # neighbour: gradf = -2, vsf = (0, -2), unexpanded bounds relative to -2: [0, 2] -> 4 > 2: limiter 2/4
    assert lim[0].tolist() == [1.0, 0.5]
    gl, liml = literal("faceLimited", 0.5, [0], [1], [[0.0, 0, 0], [1.0, 0, 0]], [[0.5, 0, 0]], [[0.0, 0, 0], [1.0, 0, 0]],
                       [[4.0] + [0.0] * 8, [4.0] + [0.0] * 8], [])
    assert [x[0] for x in liml] == [1.0, 0.5]
    # the scalar form expands both sides: neither is limited
    _, lim1 = restate("faceLimited", 0.5, 2, lo, up, C, Cf, [vf[0]], [np.full(2, 4.0), np.zeros(2), np.zeros(2)])
    assert lim1[0].tolist() == [1.0, 1.0]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _engine_run(eng, A, B, kind, k, M, vf, grad, bv, dev, host, with_limiter=True):
    """mi_limited_grad on device copies -> (grad, limiter or None) on the host"""
    import torch
    lim = eng.grad_limiter(f"{kind} Gauss linear {k!r}")
    nc = len(vf)
    bcf = boundary_flat(M)[2]
    gd = [dev(x) for x in grad]
    nl = 0 if kind.endswith("MDLimited") or not with_limiter else (nc if kind == "cellLimited" else 1)
    lo = [torch.full((M["n"],), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(nl)]
    A.limited_grad(lim, [dev(x) for x in vf], [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], gd, boundary=B,
                   bvalue=[dev(x) for x in bv] if B is not None else None, bcf=[dev(x) for x in bcf] if B is not None and bcf else None,
                   limiter_out=lo or None)
    return [host(x) for x in gd], ([host(x) for x in lo] if lo else None)


def _check(eng, A, B, kind, k, M, vf, grad, bv, dev, host, tag=""):
    g, lim = _engine_run(eng, A, B, kind, k, M, vf, grad, bv, dev, host)
    rg, rlim = run_restate(kind, k, M, vf, grad, bv)
    for i in range(len(grad)):
        assert same(g[i], rg[i]), (tag, kind, k, "grad", i, int(np.sum(bits(g[i]) != bits(rg[i]))))
    if rlim is not None:
        for j in range(len(rlim)):
            assert same(lim[j], rlim[j]), (tag, kind, k, "limiter", j)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "skewed", "graph", "skewed_noxcd"])
def test_every_kind_against_the_restatement(pkg, monkeypatch, name):
    if name.endswith("_noxcd"):   # the plain blockIdx.x mapping of the three-array gradient pass
        set_row_tables(monkeypatch, "noxcd"); name = name[:-len("_noxcd")]
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = box_mesh(syn, (13, 11, 9)) if name == "box" else skewed((9, 8, 7)) if name == "skewed" else graph_mesh(pkg)
    addr = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    for nc in (1, 3):
        vf, grad, bv = fields(syn, M, nc, 20 + nc)
        for kind in KINDS:
            for k in (1.0, 0.5):
                g = _check(eng, A, B, kind, k, M, vf, grad, bv, dev, host, name)
                assert not all(same(x, y) for x, y in zip(g, grad)), (kind, k)   # the data reach the limiter
    B.close()


@pytest.mark.gpu
def test_identity_writes_nothing(pkg):
    import torch
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = box_mesh(syn, (6, 5, 4))
    addr = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    vf, grad, bv = fields(syn, M, 3, 5)
    bcf = boundary_flat(M)[2]
    for kind in KINDS:
        for k in ("0", "1e-16"):
            gd = [dev(x) for x in grad]
            lo = [torch.full((M["n"],), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(3 if kind == "cellLimited" else 1)]
            A.limited_grad(f"{kind} Gauss linear {k}", [dev(x) for x in vf], [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], gd, B,
                           [dev(x) for x in bv], [dev(x) for x in bcf], None if kind.endswith("MDLimited") else lo)
            assert all(same(host(x), y) for x, y in zip(gd, grad))
            assert all(np.all(host(x) == -7.0) for x in lo)
    B.close()


@pytest.mark.gpu
def test_cyclic_patch_takes_the_patch_neighbour_field(pkg):
    """the box made periodic in x: the two cyclic patches are coupled, their values mi_matrix_patch_neighbour_field; the other four
    walls fixesValue"""
    import torch
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    dims = (12, 7, 6)
    M0 = box_mesh(syn, dims)
    case = syn.box_case(*dims)
    cyc = syn.add_cyclic_x(case)
    fcs = [i.face_cells for i in cyc.interfaces]
    nbrs = [cyc.interfaces[i.nbr_patch].face_cells for i in cyc.interfaces]
    caddr = eng.Addressing(ctx, M0["n"], M0["lo"], M0["up"], fcs, nbrs)
    mat = eng.Matrix(caddr)
    A = eng.Assembly(caddr)
    assert all(np.array_equal(a, b) for a, b in zip(fcs, M0["fcs"][:2]))
    M = dict(M0, kinds=[COUPLED, COUPLED] + [FIXES] * 4)
    B = eng.GradBoundary(caddr, M["fcs"], M["kinds"])
    nb = sum(f.shape[0] for f in M["fcs"])
    ncyc = sum(f.shape[0] for f in fcs)
    for nc in (1, 3):
        vf, grad, bv = fields(syn, M, nc, 50 + nc)
        bvd = [dev(x) for x in bv]
        for j in range(nc):
            pnf = torch.empty(ncyc, dtype=torch.float64, device="cuda:0")
            mat.patch_neighbour_field(dev(vf[j]), pnf)
            bvd[j][:ncyc] = pnf
            bv[j][:ncyc] = np.concatenate([vf[j][q] for q in nbrs])
        assert all(same(host(x), y) for x, y in zip(bvd, bv))
        bcf = boundary_flat(M)[2]
        for kind in KINDS:
            for k in (1.0, 0.5):
                gd = [dev(x) for x in grad]
                A.limited_grad(f"{kind} Gauss linear {k}", [dev(x) for x in vf], [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], gd, B,
                               bvd, [dev(x) for x in bcf])
                rg, _ = run_restate(kind, k, M, vf, grad, bv)
                assert all(same(host(x), y) for x, y in zip(gd, rg)), (nc, kind, k)
    assert nb == bv[0].shape[0]
    B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ROW_MODES)
def test_every_row_pass_shape(pkg, monkeypatch, mode):
    """gradient plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, and the unstaged fall-back (MI_ROW_CAP=64):
    every kind identical to the restatement"""
    set_row_blocks(monkeypatch, mode, grad=True)
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    for name in ("box", "graph"):
        case, addr = shaped_addressing(eng, ctx, syn, shape_case(pkg, name, symmetric=True), mode)
        M = random_geometry(syn, case.n_cells, case.lower_addr, case.upper_addr, 70)
        A = eng.Assembly(addr)
        B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
        for nc in (1, 3):
            vf, grad, bv = fields(syn, M, nc, 80 + nc, gscale=4.0)
            for kind in KINDS:
                _check(eng, A, B, kind, 0.5 if nc == 3 else 1.0, M, vf, grad, bv, dev, host, mode)
        B.close()


@pytest.mark.gpu
def test_in_place_equals_out_of_place(pkg):
    """the gradient limited where it lies equals a copy limited from the same inputs; the inputs stay as they were"""
    import torch
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = skewed((8, 7, 6))
    addr = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    vf, grad, bv = fields(syn, M, 3, 90)
    bcf = boundary_flat(M)[2]
    vfd, Cd, Cfd, bvd, bcfd = [dev(x) for x in vf], [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], [dev(x) for x in bv], [dev(x) for x in bcf]
    big = dev(np.stack(grad))                                  # 9 rows of one tensor, limited in place
    rows = [big[i] for i in range(9)]
    copy = [r.clone() for r in rows]
    for kind in KINDS:
        A.limited_grad(f"{kind} Gauss linear 0.5", vfd, Cd, Cfd, rows, B, bvd, bcfd)
        A.limited_grad(f"{kind} Gauss linear 0.5", vfd, Cd, Cfd, copy, B, bvd, bcfd)
        assert torch.equal(big.view(torch.int64), torch.stack(copy).view(torch.int64)), kind
    assert all(same(host(x), y) for x, y in zip(vfd, vf)) and all(same(host(x), y) for x, y in zip(bvd, bv))
    B.close()


@pytest.mark.gpu
def test_argument_errors(pkg):
    import torch
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = box_mesh(syn, (6, 5, 4))
    addr = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    other = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    Bo = eng.GradBoundary(other, M["fcs"], M["kinds"])
    vf, grad, bv = fields(syn, M, 3, 9)
    bcf = boundary_flat(M)[2]
    vfd, Cd, Cfd, bvd, bcfd = [dev(x) for x in vf], [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], [dev(x) for x in bv], [dev(x) for x in bcf]
    gd = [dev(x) for x in grad]
    lo3 = [torch.empty(M["n"], dtype=torch.float64, device="cuda:0") for _ in range(3)]
    call = lambda kind="cellLimited", **kw: A.limited_grad(f"{kind} Gauss linear 1", kw.get("vf", vfd), Cd, Cfd, kw.get("g", gd), kw.get("B", B),
                                                           kw.get("bv", bvd), kw.get("bcf", bcfd), kw.get("lim"))
    call(lim=lo3)                                               # valid
    call()
    with pytest.raises(eng.MiError, match="n_comp"):
        call(vf=vfd[:2], g=gd[:6])
    with pytest.raises(eng.MiError, match="another addressing"):
        call(B=Bo)
    with pytest.raises(eng.MiError, match="boundary has faces"):
        call(bv=None)
    with pytest.raises(eng.MiError, match="boundary has faces"):
        call(bcf=None)
    for kind in ("cellMDLimited", "faceMDLimited"):
        with pytest.raises(eng.MiError, match="limiter_out must be NULL"):
            call(kind, lim=lo3[:1])
    with pytest.raises(eng.MiError, match="alias"):
        call(g=[gd[0], vfd[1]] + gd[2:])
    with pytest.raises(eng.MiError, match="outputs must differ"):
        call(lim=[lo3[0], gd[4], lo3[2]])
    with pytest.raises(eng.MiError, match="missing"):
        call(g=gd[:8] + [None])
    bad = eng.GradLimiter(); bad.kind = 0; bad.k = 1.5; bad.identity = 0
    with pytest.raises(eng.MiError, match="coefficient"):
        A.limited_grad(bad, vfd, Cd, Cfd, gd, B, bvd, bcfd)
    bad.kind = 4; bad.k = 1.0
    with pytest.raises(eng.MiError, match="invalid"):
        A.limited_grad(bad, vfd, Cd, Cfd, gd, B, bvd, bcfd)
    # refused calls launch nothing: the gradient is what the two valid calls made of it
    ref, _ = run_restate("cellLimited", 1.0, M, vf, grad, bv)
    ref, _ = run_restate("cellLimited", 1.0, M, vf, ref, bv)
    assert all(same(host(x), y) for x, y in zip(gd, ref))
    with pytest.raises(eng.MiError, match="range"):
        eng.GradBoundary(addr, [np.array([0, M["n"]], np.int32)], ["fixesValue"])
    with pytest.raises(eng.MiError, match="kind"):
        eng.GradBoundary(addr, [np.array([0], np.int32)], [7])
    B.close(); Bo.close()


def fma_signed_zero(a, b, c):
    """one rounding (exact rational arithmetic), with IEEE's sign of a zero result: (+-0) + (+-0) keeps a common sign, any other
    exact zero is +0 -- a limited gradient has exact zeros of both signs (limiter 0)"""
    from fractions import Fraction
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r != 0:
        return float(r)
    if a * b == 0 and c == 0:
        sp, sc = bool(np.signbit(a)) != bool(np.signbit(b)), bool(np.signbit(c))
        return -0.0 if (sp and sc) else 0.0
    return 0.0


def correction_flux(lo, up, flux, cf, C, grad):
    """faceFlux*correction(U) of linearUpwind (linearUpwind.C:33-47) on the internal faces, the engine's contraction of the dot
    (fma(dz, gz, fma(dx, gx, dy*gy))); grad 9 arrays"""
    out = [np.empty(len(flux)) for _ in range(3)]
    for f, fl in enumerate(flux.tolist()):
        c = int(lo[f]) if fl > 0 else int(up[f])
        dx, dy, dz = cf[0][f] - C[0][c], cf[1][f] - C[1][c], cf[2][f] - C[2][c]
        for j in range(3):
            gx, gy, gz = grad[3 * j][c], grad[3 * j + 1][c], grad[3 * j + 2][c]
            out[j][f] = fl * (1.0 * fma_signed_zero(dz, gz, fma_signed_zero(dx, gx, dy * gy)))
    return out


@pytest.mark.gpu
def test_cell_limited_feeds_the_linear_upwind_correction(pkg):
    """`grad(U) cellLimited Gauss linear 1` -> `Gauss linearUpwind grad(U)`: mi_gauss_grad + the wall faces + /V, the limiter, then
    mi_linear_upwind_correction, against the restatement chain (the Gauss gradient is the engine's: it has its own tests)"""
    import torch
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = box_mesh(syn, (11, 9, 7))
    n, lo, up = M["n"], M["lo"], M["up"]
    nf = lo.shape[0]
    addr = eng.Addressing(ctx, n, lo, up)
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    u = syn.splitmix_uniform
    h = 1.0 / 11
    U = [np.sin(7.0 * M["C"][0] + j) * (u(100 + j, n) + 0.5) for j in range(3)]
    bv = [np.cos(3.0 * np.concatenate(M["fcs"]) + j) for j in range(3)]
    V = np.full(n, h ** 3)
    step = up - lo                                             # 1, nx, nx*ny: the face's normal direction on the box
    Sf = [np.where(step == s, h * h, 0.0) for s in (1, 11, 11 * 9)]
    Cd, Cfd, Vd = [dev(x) for x in M["C"]], [dev(x) for x in M["Cf"]], dev(V)
    grads = []
    for j in range(3):
        ssf = 0.5 * (U[j][lo] + U[j][up])
        g = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        A.gauss_grad([dev(x) for x in Sf], dev(ssf), None, g)
        off = 0
        for q, fc in enumerate(M["fcs"]):
            m = fc.shape[0]
            ax, sgn = q // 2, (-1.0 if q % 2 == 0 else 1.0)
            P = eng.Patch(ctx, n, fc)
            P.add_product(dev(np.full(m, sgn * h * h)), dev(bv[j][off:off + m]), g[ax], 0)
            P.close()
            off += m
        for d in range(3):
            eng._chk(eng.lib().mi_vec_div(ctx.h, n, eng._ptr(g[d]), eng._ptr(Vd), eng._ptr(g[d])))
        grads += g
    g0 = [host(x) for x in grads]
    A.limited_grad("cellLimited Gauss linear 1", [dev(x) for x in U], Cd, Cfd, grads, B, [dev(x) for x in bv],
                   [dev(x) for x in boundary_flat(M)[2]])
    rg, _ = run_restate("cellLimited", 1.0, M, U, g0, bv)
    assert all(same(host(x), y) for x, y in zip(grads, rg))
    assert not all(same(x, y) for x, y in zip(rg, g0))
    flux = signed_flux(u(7, nf))
    out = [torch.empty(nf, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    A.linear_upwind_correction(dev(flux), Cfd, Cd, [grads[3 * j:3 * j + 3] for j in range(3)], out)
    ref = correction_flux(lo, up, flux, M["Cf"], M["C"], rg)
    assert all(same(host(out[j]), ref[j]) for j in range(3))
    B.close()


@pytest.mark.gpu
def test_at_the_bench_size(pkg):
    """216^3 with the six walls: scalar cellLimited and vector cellMDLimited against the vectorised restatement"""
    eng, ctx, dev, host, _ = gpu_env(pkg)
    syn = pkg.synthetic
    M = box_mesh(syn, (216, 216, 216))
    addr = eng.Addressing(ctx, M["n"], M["lo"], M["up"])
    A = eng.Assembly(addr)
    B = eng.GradBoundary(addr, M["fcs"], M["kinds"])
    for kind, nc in (("cellLimited", 1), ("cellMDLimited", 3)):
        vf, grad, bv = fields(syn, M, nc, 110 + nc, gscale=400.0)
        _check(eng, A, B, kind, 1.0 if nc == 1 else 0.5, M, vf, grad, bv, dev, host, "216^3")
    B.close()
