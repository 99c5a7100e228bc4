"""The leastSquares gradient scheme restated (tests/test_least_squares_grad.py): the reference's loops line for line, generic over their
arithmetic, and the same vectorised; the meshes the tests run on.

The pin is this restatement, not a compiled reference: the reference's device code for the scheme cannot be the definition.
  vectors   leastSquaresVectors.C:123-225 (host loops) with inv(dd) in the host Field<symmTensor> form, symmTensorField.C:50-105: every
            expression rounded operation by operation, left to right as written
  gradient  the loop kept in the comment of leastSquaresGrad.C:109-118, then the patches (:139-189), the arithmetic of
            leastSquaresCalcGradFunctor (:39-53) contracted: delta rounded once, then one fma per gradient component
A mesh is a dict: n, lo, up, C [x, y, z], w, magSf (internal faces), fcs / kinds (the patches: faceCells, MI_GRAD_PATCH_*), and the
boundary face fields as patch-ordered concatenations bw, bms, bd [x, y, z]; where a test needs them Cf, bcf (face centres) and bSf."""
import numpy as np

SMALL = 1e-15                                                   # doubleScalar.H:57
OTHER, COUPLED, FIXES = 0, 1, 2                                 # MI_GRAD_PATCH_*


# ---- the reference's loops, line for line; generic over + - * / and an injected fma ----------------------------------------------------
def sqr(d):
    """SymmTensorI.H:546-554 -> xx xy xz yy yz zz"""
    return [d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]]


def mag_sqr(d):
    """VectorSpaceI.H:336-344"""
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def mag_sqr_symm(t):
    """SymmTensorI.H:276-284"""
    xx, xy, xz, yy, yz, zz = t
    return xx * xx + 2 * (xy * xy) + 2 * (xz * xz) + yy * yy + 2 * (yz * yz) + zz * zz


def det(t):
    """SymmTensorI.H:344-352"""
    xx, xy, xz, yy, yz, zz = t
    return xx * yy * zz + xy * yz * xz + xz * xy * yz - xx * yz * yz - xy * xy * zz - xz * yy * xz


def inv(t):
    """SymmTensorI.H:377-399: the cofactors / det"""
    xx, xy, xz, yy, yz, zz = t
    dt = det(t)
    c = [yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy, xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy]
    return [x / dt for x in c]


def symm_dot(t, v):
    """SymmTensorI.H:248-256"""
    xx, xy, xz, yy, yz, zz = t
    return [xx * v[0] + xy * v[1] + xz * v[2], xy * v[0] + yy * v[1] + yz * v[2], xz * v[0] + yz * v[1] + zz * v[2]]


def inv_field(dd, one):
    """symmTensorField.C:50-105: cell 0 alone decides removeCmpts; a removed component gets +1 before and -1 after, in every cell"""
    if not dd:
        return []
    zero = one - one
    scale = mag_sqr_symm(dd[0])
    rm = [(dd[0][i] * dd[0][i]) / scale < SMALL for i in (0, 3, 5)]
    if not any(rm):
        return [inv(t) for t in dd]
    units = [[one if i == q else zero for i in range(6)] for q, r in zip((0, 3, 5), rm) if r]
    plus = [list(t) for t in dd]
    for u in units:
        plus = [[x + y for x, y in zip(t, u)] for t in plus]
    out = [inv(t) for t in plus]
    for u in units:
        out = [[x - y for x, y in zip(t, u)] for t in out]
    return out


def literal_vectors(lo, up, C, w, magSf, patches, one=1.0):
    """leastSquaresVectors.C:123-225.  C[c] = [x, y, z]; patches: (coupled, faceCells, pw, pMagSf, pd) with pd[i] = [x, y, z].
    -> pVectors[f], nVectors[f], patchLsP[patch][i]"""
    zero = one - one
    dd = [[zero] * 6 for _ in C]
    for f, (own, nei) in enumerate(zip(lo, up)):
        d = [C[nei][i] - C[own][i] for i in range(3)]
        s = magSf[f] / mag_sqr(d)
        wdd = [s * x for x in sqr(d)]
        dd[own] = [a + (one - w[f]) * b for a, b in zip(dd[own], wdd)]
        dd[nei] = [a + w[f] * b for a, b in zip(dd[nei], wdd)]
    for coupled, fc, pw, pms, pd in patches:
        for i, c in enumerate(fc):
            d = pd[i]
            s = (one - pw[i]) * pms[i] / mag_sqr(d) if coupled else pms[i] / mag_sqr(d)
            dd[c] = [a + s * b for a, b in zip(dd[c], sqr(d))]
    invDd = inv_field(dd, one)
    pV, nV = [], []
    for f, (own, nei) in enumerate(zip(lo, up)):
        d = [C[nei][i] - C[own][i] for i in range(3)]
        m = magSf[f] / mag_sqr(d)
        pV.append([(one - w[f]) * m * x for x in symm_dot(invDd[own], d)])
        nV.append([-w[f] * m * x for x in symm_dot(invDd[nei], d)])
    bP = []
    for coupled, fc, pw, pms, pd in patches:
        rows = []
        for i, c in enumerate(fc):
            d = pd[i]
            s = (one - pw[i]) * pms[i] / mag_sqr(d) if coupled else pms[i] * (one / mag_sqr(d))
            rows.append([s * x for x in symm_dot(invDd[c], d)])
        bP.append(rows)
    return pV, nV, bP


def literal_grad(n, lo, up, pV, nV, bP, vf, patches, fma, zero=0.0):
    """leastSquaresGrad.C:109-118 and :139-189.  vf[c] = the components of cell c; patches: (faceCells, values[i] = the components).
    -> grad[c][3*j + k] = d(vf_j)/dx_k"""
    nc = len(vf[0]) if vf else 0
    g = [[zero] * (3 * nc) for _ in range(n)]
    for f, (own, nei) in enumerate(zip(lo, up)):
        for j in range(nc):
            delta = vf[nei][j] - vf[own][j]
            for k in range(3):
                g[own][3 * j + k] = fma(pV[f][k], delta, g[own][3 * j + k])
                g[nei][3 * j + k] = fma(-nV[f][k], delta, g[nei][3 * j + k])
    for (fc, vals), ls in zip(patches, bP):
        for i, c in enumerate(fc):
            for j in range(nc):
                delta = vals[i][j] - vf[c][j]
                for k in range(3):
                    g[c][3 * j + k] = fma(ls[i][k], delta, g[c][3 * j + k])
    return g


def literal_inputs(L, conv=float):
    """a mesh as the literal loops take it, every number through conv (float, or fractions.Fraction for exact arithmetic)"""
    n = L["n"]
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    C = [list(r) for r in zip(*[col(L["C"][d]) for d in range(3)])] if n else []
    patches, off = [], 0
    bd = [col(L["bd"][d]) for d in range(3)]
    bw, bms = col(L["bw"]), col(L["bms"])
    for fc, kd in zip(L["fcs"], L["kinds"]):
        m = fc.shape[0]
        patches.append((kd == COUPLED, fc.tolist(), bw[off:off + m], bms[off:off + m], [[bd[d][off + i] for d in range(3)] for i in range(m)]))
        off += m
    return L["lo"].tolist(), L["up"].tolist(), C, col(L["w"]), col(L["magSf"]), patches


def literal_fields(L, vf, bv, conv=float):
    """cell values and boundary values as literal_grad takes them"""
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    V = [list(r) for r in zip(*[col(x) for x in vf])]
    B = [list(r) for r in zip(*[col(x) for x in bv])]
    patches, off = [], 0
    for fc in L["fcs"]:
        patches.append((fc.tolist(), B[off:off + fc.shape[0]]))
        off += fc.shape[0]
    return V, patches


# ---- the same, vectorised: the sums in the loops' order by the oracle's sequential sweeps ---------------------------------------------
def boundary_flat(L):
    """the patch-ordered concatenation: cells, coupled per face"""
    fcs = L["fcs"]
    bcell = np.concatenate(fcs).astype(np.int32) if fcs else np.zeros(0, np.int32)
    coupled = np.concatenate([np.full(f.shape[0], k == COUPLED) for f, k in zip(fcs, L["kinds"])]) if fcs else np.zeros(0, bool)
    return bcell, coupled


def _interleave(a, b):
    out = np.empty(2 * a.shape[0], dtype=a.dtype)
    out[0::2] = a; out[1::2] = b
    return out


def restate_vectors(orc, L):
    """-> pVectors, nVectors, boundary pVectors: three arrays each.  orc.patch_add is `intf[cell[i]] += v[i]` for i ascending, so events
    ordered as the loops visit them sum in the loops' order: face f's owner, then its neighbour, then the boundary faces by patch"""
    n, lo, up, C, w, magSf = L["n"], L["lo"], L["up"], L["C"], L["w"], L["magSf"]
    bcell, coupled = boundary_flat(L)
    bw, bms, bd = L["bw"], L["bms"], L["bd"]
    with np.errstate(all="ignore"):
        d = [C[i][up] - C[i][lo] for i in range(3)]
        m = magSf / mag_sqr(d)
        wdd = [m * x for x in sqr(d)]
        bm = mag_sqr(bd)
        bs = np.where(coupled, (1.0 - bw) * bms / bm, bms / bm)
        bt = [bs * x for x in sqr(bd)]
        cells = _interleave(lo, up)
        dd = []
        for i in range(6):
            x = orc.patch_add(cells, _interleave((1.0 - w) * wdd[i], w * wdd[i]), np.zeros(n), 0)
            dd.append(orc.patch_add(bcell, bt[i], x, 0))
        if n:
            t = [x[0] for x in dd]
            scale = mag_sqr_symm(t)
            add = np.zeros(6)
            for q in (0, 3, 5):
                if (t[q] * t[q]) / scale < SMALL:
                    add[q] = 1.0
            if add.any():
                dd = [x + a for x, a in zip(dd, add)]
                dd = [x - a for x, a in zip(inv(dd), add)]
            else:
                dd = inv(dd)
        vo, vn = symm_dot([x[lo] for x in dd], d), symm_dot([x[up] for x in dd], d)
        pV = [(1.0 - w) * m * x for x in vo]
        nV = [-w * m * x for x in vn]
        bs = np.where(coupled, (1.0 - bw) * bms / bm, bms * (1.0 / bm))
        bP = [bs * x for x in symm_dot([x[bcell] for x in dd], bd)]
    return pV, nV, bP


def restate_grad(orc, L, V, vf, bv):
    """-> 3*len(vf) arrays, grad[3*j + k].  orc.patch_add_product is `g[cell[i]] = fma(a[i], b[i], g[cell[i]])` for i ascending"""
    n, lo, up = L["n"], L["lo"], L["up"]
    pV, nV, bP = V
    bcell, _ = boundary_flat(L)
    cells = _interleave(lo, up)
    out = []
    for j in range(len(vf)):
        delta = vf[j][up] - vf[j][lo]
        d2 = _interleave(delta, delta)
        bdelta = bv[j] - vf[j][bcell]
        for k in range(3):
            g = orc.patch_add_product(cells, _interleave(pV[k], -nV[k]), d2, np.zeros(n), 0)
            out.append(orc.patch_add_product(bcell, bP[k], bdelta, g, 0))
    return out


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def skewed_ls(syn, dims=(5, 4, 3)):
    """test_assembly.skewed_mesh (perturbed points, non-orthogonal) with its walls cut into their four sides: six patches, x- and y-
    coupled, the others fixesValue or other; seeded weights in (0.3, 0.7), delta = Cf - C on every patch"""
    from test_assembly import skewed_mesh
    M = skewed_mesh(dims)
    G, nI, (nx, ny, nz) = M["G"], M["nI"], dims
    (_, _, c0, s0), (_, _, c1, s1), (_, _, cw, sw) = M["patches"]
    assert cw == 2 * (nx * nz + nx * ny)
    ranges = [(s0, c0), (s1, c1), (sw, nx * nz), (sw + nx * nz, nx * nz), (sw + 2 * nx * nz, nx * ny), (sw + 2 * nx * nz + nx * ny, nx * ny)]
    kinds = [COUPLED, OTHER, COUPLED, FIXES, OTHER, FIXES]
    b = np.concatenate([np.arange(s, s + c) for s, c in ranges])
    fcs = [M["owner"][s:s + c].astype(np.int32) for s, c in ranges]
    col = lambda a, idx: [np.ascontiguousarray(a[idx, k]) for k in range(3)]
    bcell = M["owner"][b]
    u = syn.splitmix_uniform
    return dict(n=M["n"], lo=M["lo"], up=M["up"], C=col(G["C"], slice(None)), w=0.3 + 0.4 * u(301, nI), magSf=np.ascontiguousarray(G["magSf"][:nI]),
                fcs=fcs, kinds=kinds, bw=0.3 + 0.4 * u(302, b.shape[0]), bms=np.ascontiguousarray(G["magSf"][b]),
                bd=[x - y for x, y in zip(col(G["Cf"], b), col(G["C"], bcell))], Cf=col(G["Cf"], slice(0, nI)), bcf=col(G["Cf"], b),
                bSf=col(G["Sf"], b))


def flat_ls(syn, dims=(7, 5, 1)):
    """one cell thick: the centres perturbed in x and y and sharing one z, the two z patches empty (zero faces), so dd.zz is zero in every
    cell and inv(dd) removes the component"""
    nx, ny, nz = dims
    assert nz == 1
    case = syn.box_case(*dims)
    n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
    u = syn.splitmix_uniform
    h = 1.0 / nx
    c = np.arange(n)
    i, j = c % nx, c // nx
    C = [(i + 0.5 + 0.3 * (u(311, n) - 0.5)) * h, (j + 0.5 + 0.3 * (u(312, n) - 0.5)) * h, np.full(n, 0.5 * h)]
    fcs, bcf = [], [[], [], []]
    for ax, (idx, m) in enumerate(((i, nx), (j, ny))):
        for side in (0, m - 1):
            fc = np.nonzero(idx == side)[0].astype(np.int32)
            p = [C[q][fc].copy() for q in range(3)]
            p[ax] = np.full(fc.shape[0], 0.0 if side == 0 else m * h)
            fcs.append(fc)
            for q in range(3):
                bcf[q].append(p[q])
    fcs += [np.zeros(0, np.int32), np.zeros(0, np.int32)]
    bcf = [np.concatenate(x) for x in bcf]
    bcell = np.concatenate(fcs)
    nb = bcell.shape[0]
    return dict(n=n, lo=lo, up=up, C=C, w=0.3 + 0.4 * u(313, lo.shape[0]), magSf=0.5 + u(314, lo.shape[0]), fcs=fcs,
                kinds=[COUPLED, OTHER, FIXES, COUPLED, OTHER, OTHER], bw=0.3 + 0.4 * u(315, nb), bms=0.5 + u(316, nb),
                bd=[x - y[bcell] for x, y in zip(bcf, C)], bcf=bcf)


def seeded_ls(syn, n, lo, up, seed):
    """geometry for a graph that has none: centres in the unit cube, seeded weights and magSf, and the boundary faces in one `other` and
    one `coupled` patch.  Every cell that has any face gets enough boundary faces to have at least four faces in all (dd non-singular),
    every third such cell one more; a cell without faces stays without.  b_weights is NaN off the coupled patch: it is read on coupled
    faces only"""
    u = syn.splitmix_uniform
    nf = lo.shape[0]
    cnt = np.bincount(lo, minlength=n) + np.bincount(up, minlength=n)
    need = np.where(cnt > 0, np.maximum(4 - cnt, 0) + (np.arange(n) % 3 == 0), 0)
    second = need // 2                                          # the coupled patch takes half of a cell's boundary faces, rounded down
    fcs = [np.repeat(np.arange(n), need - second).astype(np.int32), np.repeat(np.arange(n), second).astype(np.int32)]
    nb = int(need.sum())
    bw = 0.3 + 0.4 * u(seed + 5, nb)
    bw[:fcs[0].shape[0]] = np.nan
    bd = [u(seed + 8 + d, nb) - 0.5 for d in range(3)]
    return dict(n=n, lo=lo, up=up, C=[u(seed + d, n) for d in range(3)], w=0.3 + 0.4 * u(seed + 3, nf), magSf=0.5 + u(seed + 4, nf), fcs=fcs,
                kinds=[OTHER, COUPLED], bw=bw, bms=0.5 + u(seed + 6, nb), bd=bd)


def fields(syn, L, nc, seed):
    """cell values with exact zeros of both signs and boundary values -> vf, bv"""
    u = syn.splitmix_uniform
    n, nb = L["n"], sum(f.shape[0] for f in L["fcs"])
    vf = []
    for j in range(nc):
        x = u(seed + j, n) - 0.5
        x[::5] = 0.0
        x[2::7] = -0.0
        vf.append(x)
    bv = [u(seed + 30 + j, nb) - 0.5 for j in range(nc)]
    for x in bv:
        x[1::6] = -0.0
    return vf, bv


def all_finite(arrays):
    return all(bool(np.all(np.isfinite(x))) for x in arrays)
