"""fvc::reconstruct and fvc::surfaceSum restated (tests/test_reconstruct.py): the reference's evaluation written out loop by loop, generic
over its number type, and the same vectorised over cells; the meshes the tests run on.

The pin is this restatement, not a compiled reference:
  reconstruct   fvcReconstruct.C:45-84: inv(surfaceSum(SfHat*Sf)) & surfaceSum(SfHat*ssf), SfHat = Sf/magSf
  surfaceSum    fvcSurfaceIntegrate.C:262-360 with surfaceIntegrateFunctor<Type, false> (:40-132): a cell starts from +0.0 and ADDS its own
                faces ascending, its neighbour-side faces in losort order, then the boundary faces patch after patch
  inv           tensorField.C:226-305 (cell 0 alone decides removeCmpts) around TensorI.H:552-560 (det) and :588-604 (the cofactors / det),
                every operation rounded on its own -- an assumption about the reference's device functor
  T & s         TensorI.H:409-420 contracted as the engine's dot product: fma(R_az, s_z, fma(R_ax, s_x, R_ay*s_y)) -- the standing assumption
A mesh is a dict: n, lo, up, Sf [x, y, z], magSf (internal faces), fcs / kinds (the patches), bSf [x, y, z], bms (boundary faces, the
patch-ordered concatenation).  Tensors are nine components xx xy xz yx yy yz zx zy zz."""
import numpy as np

from least_squares_support import flat_ls, seeded_ls, skewed_ls

SMALL = 1e-15                                                   # doubleScalar.H:57


# ---- the arithmetic, generic over floats, Fractions and numpy arrays -----------------------------------------------------------------------
def det(t):
    """TensorI.H:552-560"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = t
    return xx * yy * zz + xy * yz * zx + xz * yx * zy - xx * yz * zy - xy * yx * zz - xz * yy * zx


def inv(t):
    """TensorI.H:588-604: the nine cofactor expressions, each / det"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = t
    d = det(t)
    c = [yy * zz - zy * yz, xz * zy - xy * zz, xy * yz - xz * yy,
         zx * yz - yx * zz, xx * zz - xz * zx, yx * xz - xx * yz,
         yx * zy - yy * zx, xy * zx - xx * zy, xx * yy - yx * xy]
    return [x / d for x in c]


def mag_sqr(t):
    """magSqr(Tensor): the nine squares summed left to right"""
    s = t[0] * t[0]
    for x in t[1:]:
        s = s + x * x
    return s


# ---- literal: loop by loop ----------------------------------------------------------------------------------------------------------------
def literal_surface_sum(n, lo, up, face_values, patches, zero=0.0, mag=False):
    """face_values[f]; patches: (faceCells, values[i]).  surfaceIntegrateFunctor<Type, false> per cell, then the patches' running add"""
    term = (lambda x: abs(x)) if mag else (lambda x: x)
    own = [[] for _ in range(n)]
    nei = [[] for _ in range(n)]                                # losort: a cell's neighbour-side faces ascending
    for f, (o, u) in enumerate(zip(lo, up)):
        own[o].append(f); nei[u].append(f)
    out = []
    for c in range(n):
        acc = zero
        for f in own[c]:
            acc = acc + term(face_values[f])
        for f in nei[c]:
            acc = acc + term(face_values[f])
        out.append(acc)
    for fc, vals in patches:
        for i, c in enumerate(fc):
            out[c] = out[c] + term(vals[i])
    return out


def literal_build(n, lo, up, Sf, magSf, patches, one=1.0):
    """Sf[f] = [x, y, z]; patches: (faceCells, pSf[i] = [x, y, z], pMagSf[i]).  -> SfHat[f], patch SfHat, inverse[c] (nine), removed (3 bools).
    Every cell must have a non-singular tensor (a float division by zero raises here)"""
    zero = one - one
    hat = [[x / m for x in s] for s, m in zip(Sf, magSf)]
    phat = [[[x / m for x in s] for s, m in zip(pS, pM)] for _, pS, pM in patches]
    T = []
    for a in range(3):
        for b in range(3):
            T.append(literal_surface_sum(n, lo, up, [h[a] * s[b] for h, s in zip(hat, Sf)],
                                         [(fc, [h[a] * s[b] for h, s in zip(ph, pS)]) for (fc, pS, _), ph in zip(patches, phat)], zero))
    T = [list(t) for t in zip(*T)]                              # T[c] = nine components
    if not T:
        return hat, phat, [], [False] * 3
    scale = mag_sqr(T[0])
    removed = [T[0][4 * d] / scale < SMALL for d in range(3)]
    if not any(removed):
        return hat, phat, [inv(t) for t in T], removed
    plus = T
    for d in range(3):
        if removed[d]:
            unit = [one if i == 4 * d else zero for i in range(9)]
            plus = [[x + y for x, y in zip(t, unit)] for t in plus]
    R = [inv(t) for t in plus]
    for d in range(3):
        if removed[d]:
            unit = [one if i == 4 * d else zero for i in range(9)]
            R = [[x - y for x, y in zip(t, unit)] for t in R]
    return hat, phat, R, removed


def literal_reconstruct(n, lo, up, hat, phat, R, ssf, patches, fma, zero=0.0):
    """ssf[f]; patches: (faceCells, values[i]).  -> out[c] = [x, y, z]"""
    s = [literal_surface_sum(n, lo, up, [h[k] * v for h, v in zip(hat, ssf)],
                             [(fc, [h[k] * v for h, v in zip(ph, vals)]) for (fc, vals), ph in zip(patches, phat)], zero) for k in range(3)]
    return [[fma(R[c][3 * a + 2], s[2][c], fma(R[c][3 * a], s[0][c], R[c][3 * a + 1] * s[1][c])) for a in range(3)] for c in range(n)]


def literal_inputs(L, conv=float):
    """a mesh as the literal loops take it, every number through conv (float, or fractions.Fraction for exact arithmetic)"""
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    Sf = [list(r) for r in zip(*[col(L["Sf"][d]) for d in range(3)])]
    bSf = [list(r) for r in zip(*[col(L["bSf"][d]) for d in range(3)])]
    bms = col(L["bms"])
    patches, off = [], 0
    for fc in L["fcs"]:
        m = fc.shape[0]
        patches.append((fc.tolist(), bSf[off:off + m], bms[off:off + m]))
        off += m
    return L["lo"].tolist(), L["up"].tolist(), Sf, col(L["magSf"]), patches


def literal_flux(L, ssf, bssf, conv=float):
    col = lambda a: [conv(x) for x in np.asarray(a, dtype=np.float64).tolist()]
    b = col(bssf)
    patches, off = [], 0
    for fc in L["fcs"]:
        patches.append((fc.tolist(), b[off:off + fc.shape[0]]))
        off += fc.shape[0]
    return col(ssf), patches


# ---- the same, vectorised over cells --------------------------------------------------------------------------------------------------------
def boundary_cells(L):
    return np.concatenate(L["fcs"]).astype(np.int32) if L["fcs"] else np.zeros(0, np.int32)


def restate_surface_sum(orc, L, v, bv=None, mag=False):
    """orc.patch_add is `intf[cell[i]] += v[i]` (fn 2: |v[i]|) for i ascending: all owner events in face order, then all neighbour events in
    face order, then the boundary faces in patch order give every cell its own faces, its losort faces, its boundary faces, from +0.0"""
    fn = 2 if mag else 0
    x = orc.patch_add(L["lo"], v, np.zeros(L["n"]), fn)
    x = orc.patch_add(L["up"], v, x, fn)
    return x if bv is None else orc.patch_add(boundary_cells(L), bv, x, fn)


def restate_build(orc, L):
    """-> dict(hat, bhat: three arrays each; inv: nine cell arrays; removed: (x, y, z) of 0 / 1)"""
    n = L["n"]
    with np.errstate(all="ignore"):
        hat = [L["Sf"][k] / L["magSf"] for k in range(3)]
        bhat = [L["bSf"][k] / L["bms"] for k in range(3)]
        T = [restate_surface_sum(orc, L, hat[a] * L["Sf"][b], bhat[a] * L["bSf"][b]) for a in range(3) for b in range(3)]
        removed = [0, 0, 0]
        if n:
            t0 = [float(x[0]) for x in T]
            scale = np.float64(mag_sqr([np.float64(x) for x in t0]))
            removed = [int(np.float64(t0[4 * d]) / scale < SMALL) for d in range(3)]   # 0/0 is NaN: the comparison is false
        if any(removed):
            add = [1.0 if (i % 4 == 0 and removed[i // 4]) else 0.0 for i in range(9)]
            R = [x - a for x, a in zip(inv([x + a for x, a in zip(T, add)]), add)]
        else:
            R = inv(T)
    return dict(hat=hat, bhat=bhat, inv=R, removed=tuple(removed))


def restate_reconstruct(orc, L, B, ssf, bssf):
    """one flux -> three cell arrays.  orc.patch_add_product(cells, a, b, c) is c[cell[i]] = fma(a[i], b[i], c[cell[i]]): on arange(n) an
    element-wise fma with one rounding"""
    n = L["n"]
    cells = np.arange(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        s = [restate_surface_sum(orc, L, B["hat"][k] * ssf, B["bhat"][k] * bssf) for k in range(3)]
        R = B["inv"]
        return [orc.patch_add_product(cells, R[3 * a + 2], s[2], orc.patch_add_product(cells, R[3 * a], s[0], R[3 * a + 1] * s[1], 0), 0)
                for a in range(3)]


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def skewed_rc(syn, dims=(5, 4, 3)):
    """test_assembly.skewed_mesh with the real Sf / magSf of its geometry and the six patches of skewed_ls: closed cells"""
    from test_assembly import skewed_mesh
    M, L = skewed_mesh(dims), skewed_ls(syn, dims)
    nI = M["nI"]
    return dict(n=L["n"], lo=L["lo"], up=L["up"], Sf=[np.ascontiguousarray(M["G"]["Sf"][:nI, k]) for k in range(3)], magSf=L["magSf"],
                fcs=L["fcs"], kinds=L["kinds"], bSf=L["bSf"], bms=L["bms"])


def flat_rc(syn, dims=(7, 5, 1)):
    """the one-cell-thick topology of flat_ls with seeded in-plane face vectors (sx, sy, 0), the x faces mostly along x and the y faces mostly
    along y, magSf their length; the two z patches empty: T.zz is zero in every cell and inv removes the component"""
    L = flat_ls(syn, dims)
    nx, ny, _ = dims
    u = syn.splitmix_uniform
    lo, up = L["lo"], L["up"]
    nf = lo.shape[0]
    xface = (up - lo) == 1

    def vectors(along_x, seed):
        m = along_x.shape[0]
        major, minor = 0.5 + u(seed, m), 0.4 * (u(seed + 1, m) - 0.5)
        sx, sy = np.where(along_x, major, minor), np.where(along_x, minor, major)
        return [sx, sy, np.zeros(m)], np.sqrt(sx * sx + sy * sy)

    Sf, magSf = vectors(xface, 321)
    sizes = [f.shape[0] for f in L["fcs"]]
    along_x = np.concatenate([np.full(m, p < 2) for p, m in enumerate(sizes)])          # flat_ls: the two x sides, then the two y sides
    sign = np.concatenate([np.full(m, -1.0 if p in (0, 2) else 1.0) for p, m in enumerate(sizes)])
    bSf, bms = vectors(along_x, 331)
    bSf = [sign * x for x in bSf]
    assert nf == (nx - 1) * ny + nx * (ny - 1)
    return dict(n=L["n"], lo=lo, up=up, Sf=Sf, magSf=magSf, fcs=L["fcs"], kinds=L["kinds"], bSf=bSf, bms=bms)


def seeded_rc(syn, n, lo, up, seed):
    """geometry for a graph that has none: seeded Sf in (-0.5, 0.5)^3, seeded magSf in (0.5, 1.5), and the boundary faces dealt out as
    seeded_ls deals them: every cell that has any face has at least four, a cell without faces stays without"""
    u = syn.splitmix_uniform
    S = seeded_ls(syn, n, lo, up, seed)
    nf, nb = lo.shape[0], sum(f.shape[0] for f in S["fcs"])
    return dict(n=n, lo=lo, up=up, Sf=[u(seed + 20 + d, nf) - 0.5 for d in range(3)], magSf=0.5 + u(seed + 23, nf), fcs=S["fcs"], kinds=S["kinds"],
                bSf=[u(seed + 24 + d, nb) - 0.5 for d in range(3)], bms=0.5 + u(seed + 27, nb))


def faceless_cells(L):
    """the cells without any face, internal or boundary"""
    cnt = np.bincount(L["lo"], minlength=L["n"]) + np.bincount(L["up"], minlength=L["n"]) + np.bincount(boundary_cells(L), minlength=L["n"])
    return np.nonzero(cnt == 0)[0]


def fluxes(syn, L, n_rhs, seed):
    """face fluxes with exact zeros of both signs, as least_squares_support.fields seeds them -> ssf, bssf (n_rhs arrays each)"""
    u = syn.splitmix_uniform
    nf, nb = L["lo"].shape[0], sum(f.shape[0] for f in L["fcs"])
    ssf, bssf = [], []
    for r in range(n_rhs):
        x = u(seed + r, nf) - 0.5
        x[::5] = 0.0
        x[2::7] = -0.0
        y = u(seed + 30 + r, nb) - 0.5
        y[1::6] = -0.0
        y[3::11] = 0.0
        ssf.append(x); bssf.append(y)
    return ssf, bssf
