"""The leastSquares gradient scheme (finiteVolume/gradSchemes/leastSquaresGrad): mi_grad_scheme_parse, the vectors built once per mesh on
the device (mi_ls_vectors_create) and the gradient as one row pass (mi_ls_grad), bit for bit against the restatement of
tests/least_squares_support.py -- restated, not pinned by a compiled reference: the reference's device code for this scheme cannot be
the definition."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from assembly_support import (DEGENERATE_MESHES, OTHER_TABLES, ROW_MODES, bits, fma, gpu_env, same, set_row_blocks, set_row_tables, shape_case,
                              shaped_addressing)
from least_squares_support import (COUPLED, SMALL, all_finite, boundary_flat, fields, flat_ls, literal_fields, literal_grad, literal_inputs,
                                   literal_vectors, restate_grad, restate_vectors, seeded_ls, skewed_ls)
from test_limited_grad import restate

LIMITERS = ("cellLimited", "cellMDLimited", "faceLimited", "faceMDLimited")
FACELESS = ("one_cell", "no_faces", "isolated")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme, base", [("Gauss linear", 0), ("leastSquares", 1), ("  Gauss\tlinear\n", 0), (" leastSquares ", 1)])
def test_parse_accepts_the_base_schemes(pkg, scheme, base):
    s = pkg.engine.grad_scheme(scheme)
    assert (s.base, s.limited) == (base, 0)
    assert (s.limiter.kind, s.limiter.identity, s.limiter.k) == (0, 0, 0.0)


@pytest.mark.parametrize("kind", LIMITERS)
@pytest.mark.parametrize("k", ["0", "1e-16", "0.5", "1"])
def test_parse_accepts_the_limited_schemes(pkg, kind, k):
    """over Gauss linear the limiter is mi_grad_limiter_parse's, field for field; over leastSquares the same one"""
    eng = pkg.engine
    ref = eng.grad_limiter(f"{kind} Gauss linear {k}")
    for base, text in ((0, "Gauss linear"), (1, "leastSquares")):
        for scheme in (f"{kind} {text} {k}", f"  {kind}\t{text.replace(' ', '  ')}\n{k} "):
            s = eng.grad_scheme(scheme)
            assert (s.base, s.limited) == (base, 1)
            assert bytes(s.limiter) == bytes(ref)
            assert (s.limiter.kind, s.limiter.k, s.limiter.identity) == (LIMITERS.index(kind), float(k), 1 if float(k) < SMALL else 0)


@pytest.mark.parametrize("scheme, why", [
    ("fourth", "gradient scheme 'fourth' is not supported"),
    ("cellLimited fourth 1", "base gradient scheme 'fourth' is not supported"),
    ("leastSquaress", "not supported"),
    ("Gauss upwind", "interpolation"),
    ("cellMDLimited Gauss pointLinear 1", "interpolation"),
    ("Gauss", "interpolation"),
    ("cellLimited Gauss", "interpolation"),
    ("cellLimited cellLimited leastSquares 1 1", "limited scheme over a limited"),
    ("faceMDLimited faceLimited Gauss linear 0.5 1", "limited scheme over a limited"),
    ("leastSquares 1", "extra '1'"),
    ("leastSquares linear", "extra 'linear'"),
    ("Gauss linear 1", "extra '1'"),
    ("cellLimited", "base gradient"),
    ("cellLimited leastSquares", "coefficient"),
    ("cellLimited Gauss linear", "coefficient"),
    ("cellLimited leastSquares 1 2", "extra '2'"),
    ("cellLimited Gauss linear 1 2", "extra '2'"),
    ("cellLimited leastSquares one", "not a number"),
    ("cellLimited leastSquares 1.5", "should be >= 0 and <= 1"),
    ("faceLimited leastSquares -0.1", "should be >= 0 and <= 1"),
    ("faceMDLimited leastSquares nan", "should be >= 0 and <= 1"),
    ("", "empty"),
    ("  \t\n", "empty"),
])
def test_parse_refuses(pkg, scheme, why):
    eng = pkg.engine
    with pytest.raises(eng.MiError, match=why):
        eng.grad_scheme(scheme)


def test_the_limiter_parser_still_refuses_a_least_squares_base(pkg):
    with pytest.raises(pkg.engine.MiError, match="base"):
        pkg.engine.grad_limiter("cellLimited leastSquares 1")


def test_exports(pkg):
    lib = pkg.engine.lib()
    for name in ("mi_grad_scheme_parse", "mi_ls_vectors_create", "mi_ls_vectors_destroy", "mi_ls_vectors_fields", "mi_ls_grad"):
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "Foam::fv::gradScheme::New(" in syms
    assert "Foam::leastSquaresVectors::leastSquaresVectors(" in syms
    assert syms.count(" T Foam::fvc::leastSquaresGrad(") == 2


def _columns(rows, m):
    """rows[i][k] -> m arrays"""
    return [np.array([r[k] for r in rows], dtype=np.float64) for k in range(m)]


@pytest.mark.parametrize("nc", [1, 3])
def test_restatement_equals_the_literal_loops(pkg, orc, nc):
    syn = pkg.synthetic
    L = skewed_ls(syn)
    lo, up, C, w, magSf, patches = literal_inputs(L)
    pV, nV, bP = literal_vectors(lo, up, C, w, magSf, patches)
    V = restate_vectors(orc, L)
    lit = _columns(pV, 3), _columns(nV, 3), _columns([r for p in bP for r in p], 3)
    for a, b in zip(lit, V):
        assert all(same(x, y) for x, y in zip(a, b))
    vf, bv = fields(syn, L, nc, 40 + nc)
    cells, bpatches = literal_fields(L, vf, bv)
    g = _columns(literal_grad(L["n"], lo, up, pV, nV, bP, cells, bpatches, fma), 3 * nc)
    assert all(same(x, y) for x, y in zip(g, restate_grad(orc, L, V, vf, bv)))
    assert all_finite(g) and any(np.any(x != 0.0) for x in g)


@pytest.mark.parametrize("mesh", ["skewed", "flat"])
def test_literal_loops_give_the_gradient_of_a_linear_field_exactly(pkg, mesh):
    """exact rational arithmetic, no tolerance: least squares reproduces a linear field on any mesh whose dd is non-singular -- a wrong
    sign, swapped ownLs / neiLs, a wrong inv or a wrong removeCmpts all break it.  On the one-cell-thick mesh the removed direction's
    derivative is exactly zero"""
    syn = pkg.synthetic
    L = skewed_ls(syn) if mesh == "skewed" else flat_ls(syn)
    F = Fraction
    lo, up, C, w, magSf, patches = literal_inputs(L, F)
    pV, nV, bP = literal_vectors(lo, up, C, w, magSf, patches, one=F(1))
    a = [[F(7, 10), F(-13, 10), F(9, 20)], [F(-1, 3), F(2, 7), F(5, 4)], [F(3, 2), F(1, 9), F(-2, 5)]]
    b = [F(1, 8), F(-3, 5), F(2)]
    at = lambda j, x: a[j][0] * x[0] + a[j][1] * x[1] + a[j][2] * x[2] + b[j]
    for nc in (1, 3):
        cells = [[at(j, x) for j in range(nc)] for x in C]
        bpatches = [(fc, [[at(j, [C[c][d] + pd[i][d] for d in range(3)]) for j in range(nc)] for i, c in enumerate(fc)]) for _, fc, _, _, pd in patches]
        g = literal_grad(L["n"], lo, up, pV, nV, bP, cells, bpatches, lambda x, y, z: x * y + z, zero=F(0))
        want = [a[j][k] if (mesh == "skewed" or k < 2) else F(0) for j in range(nc) for k in range(3)]
        assert all(row == want for row in g)


def test_one_cell_thick_mesh_has_no_z_component(pkg, orc):
    syn = pkg.synthetic
    L = flat_ls(syn)
    V = restate_vectors(orc, L)
    vf, bv = fields(syn, L, 3, 50)
    g = restate_grad(orc, L, V, vf, bv)
    assert all_finite([x for v in V for x in v] + g)
    for v in V:
        assert np.all(v[2] == 0.0) and np.any(v[0] != 0.0) and np.any(v[1] != 0.0)
    for j in range(3):
        assert np.all(g[3 * j + 2] == 0.0) and np.any(g[3 * j] != 0.0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
class Device:
    """one mesh under one addressing on the device: the boundary, the vectors and an Assembly"""

    def __init__(self, env, L, addr):
        self.eng, self.ctx, self.dev, self.host, self.E = env
        eng, dev = self.eng, self.dev
        self.L, self.addr = L, addr
        self.nf, self.nb = L["lo"].shape[0], sum(f.shape[0] for f in L["fcs"])
        self.A = eng.Assembly(addr)
        self.B = eng.GradBoundary(addr, L["fcs"], L["kinds"])
        self.lsv = eng.LsVectors(addr, self.B, [dev(x) for x in L["C"]], dev(L["w"]), dev(L["magSf"]), dev(L["bw"]), dev(L["bms"]),
                                 [dev(x) for x in L["bd"]])

    def vectors(self):
        p, nv, bp = ([self.E(m) for _ in range(3)] for m in (self.nf, self.nf, self.nb))
        self.lsv.fields(p, nv, bp)
        return tuple([self.host(x) for x in v] for v in (p, nv, bp))

    def grad(self, vf, bv):
        out = [self.E(self.L["n"]) for _ in range(3 * len(vf))]
        self.A.ls_grad(self.lsv, [self.dev(x) for x in vf], out, bvalue=[self.dev(x) for x in bv])
        return [self.host(x) for x in out]

    def close(self):
        self.lsv.close(); self.B.close()


def _addressings(eng, ctx, L):
    """the caller's numbering, and the same numbering under ordered addressing"""
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _check(D, ref, tag):
    """vectors and both gradients of one Device against the restatement ref = (V, {nc: (vf, bv, grad)})"""
    V, grads = ref
    got = D.vectors()
    for a, b, what in zip(got, V, ("pVectors", "nVectors", "boundary pVectors")):
        for k in range(3):
            assert same(a[k], b[k]), (tag, what, k, int(np.sum(bits(a[k]) != bits(b[k]))))
    for nc, (vf, bv, rg) in grads.items():
        g = D.grad(vf, bv)
        for i in range(3 * nc):
            assert same(g[i], rg[i]), (tag, "grad", nc, i, int(np.sum(bits(g[i]) != bits(rg[i]))))
    return got


def _reference(orc, syn, L, seed):
    V = restate_vectors(orc, L)
    grads = {}
    for nc in (1, 3):
        vf, bv = fields(syn, L, nc, seed + nc)
        grads[nc] = (vf, bv, restate_grad(orc, L, V, vf, bv))
    assert all_finite([x for v in V for x in v] + [x for _, _, g in grads.values() for x in g]), "a singular dd: change the seed"
    return V, grads


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["skewed", "flat"])
def test_vectors_and_gradients_against_the_restatement(pkg, orc, mesh):
    """the skewed 5x4x3 box with two coupled patches among six, and the one-cell-thick 7x5x1 mesh that takes the removeCmpts path"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    L = skewed_ls(syn) if mesh == "skewed" else flat_ls(syn)
    ref = _reference(orc, syn, L, 60)
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        got = _check(D, ref, (mesh, tag))
        if mesh == "flat":
            assert all(np.all(v[2] == 0.0) for v in got)
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_degenerate_meshes(pkg, orc, name):
    """cells and meshes without faces, hubs of thousands of faces, cell counts around the block boundaries, dense rows: every cell that has
    a face has at least four, so every restated output is finite; a cell without faces has the gradient +0 and its non-finite inverse
    reaches no output"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    case = shape_case(pkg, name)
    L = seeded_ls(syn, case.n_cells, case.lower_addr, case.upper_addr, 400)
    ref = _reference(orc, syn, L, 70)
    cnt = np.bincount(L["lo"], minlength=L["n"]) + np.bincount(L["up"], minlength=L["n"])
    empty = np.nonzero(cnt == 0)[0]
    assert (empty.shape[0] > 0) == (name in FACELESS)
    assert not np.isin(np.concatenate(L["fcs"]), empty).any()
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _check(D, ref, (name, tag))
        for nc, (vf, bv, _) in ref[1].items():
            for x in D.grad(vf, bv):
                assert same(x[empty], np.zeros(empty.shape[0]))
        D.close()


# (mesh, renumbered into the tile order) -> the mesh's geometry and its restatement, computed once: every `tiles*` mode renumbers the
# case the same way, the other modes leave it as it is
_SHAPE_REFS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("tables, mode", [("default", m) for m in ROW_MODES] + OTHER_TABLES)
def test_every_row_pass_shape(pkg, orc, monkeypatch, tables, mode):
    """gradient plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, the unstaged fall-back (MI_ROW_CAP=64), the
    32-bit row tables and the plain block mapping: the vectors and both gradients equal the restatement, hence each other across modes"""
    set_row_tables(monkeypatch, tables)
    set_row_blocks(monkeypatch, mode, grad=True)
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    for name in ("box", "graph"):
        case, addr = shaped_addressing(eng, ctx, syn, shape_case(pkg, name, symmetric=True), mode)
        cache = _SHAPE_REFS.setdefault((name, mode.startswith("tiles")), {})
        if not cache:
            L = seeded_ls(syn, case.n_cells, case.lower_addr, case.upper_addr, 500)
            cache.update(L=L, ref=_reference(orc, syn, L, 80))
        L = cache["L"]
        assert np.array_equal(L["lo"], case.lower_addr) and np.array_equal(L["up"], case.upper_addr)
        D = Device(env, L, addr)
        _check(D, cache["ref"], (name, tables, mode))
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["cellLimited leastSquares 1", "faceMDLimited leastSquares 0.5"])
def test_limited_least_squares(pkg, orc, scheme):
    """ls_grad then limited_grad, as cellLimitedGrad::calcGrad takes any basicGradScheme_: equal to test_limited_grad's restatement fed
    with the restated leastSquares gradient"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx, dev, host, E = env
    syn = pkg.synthetic
    L = skewed_ls(syn)
    s = eng.grad_scheme(scheme)
    assert s.base == 1 and s.limited == 1
    kind, k = LIMITERS[s.limiter.kind], s.limiter.k
    bcell, _ = boundary_flat(L)
    bkind = np.concatenate([np.full(f.shape[0], q) for f, q in zip(L["fcs"], L["kinds"])])
    V = restate_vectors(orc, L)
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        for nc in (1, 3):
            vf, bv = fields(syn, L, nc, 90 + nc)
            bv = [40.0 * x for x in bv]                         # boundary values far from the cell values: most boundary cells are limited
            ls = restate_grad(orc, L, V, vf, bv)
            want, _ = restate(kind, k, L["n"], L["lo"], L["up"], L["C"], L["Cf"], vf, ls, bcell, bkind, bv, L["bcf"])
            assert not all(same(x, y) for x, y in zip(want, ls))
            g = [E(L["n"]) for _ in range(3 * nc)]
            vfd, bvd = [dev(x) for x in vf], [dev(x) for x in bv]
            D.A.ls_grad(D.lsv, vfd, g, bvalue=bvd)
            D.A.limited_grad(s.limiter, vfd, [dev(x) for x in L["C"]], [dev(x) for x in L["Cf"]], g, boundary=D.B, bvalue=bvd,
                             bcf=[dev(x) for x in L["bcf"]])
            for i in range(3 * nc):
                assert same(host(g[i]), want[i]), (tag, scheme, nc, i)
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [1, 3])
def test_boundary_values_through_the_gauss_correction(pkg, orc, nc):
    """leastSquaresGrad.C:193 calls gaussGrad::correctBoundaryConditions: Patch.gauss_grad_correct on a patch that is not coupled, fed the
    leastSquares cell gradient, against the restated gaussGrad.C:277-303"""
    from test_div_dev_tgrad import gauss_grad_correct
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx, dev, host, E = env
    syn = pkg.synthetic
    L = skewed_ls(syn)
    V = restate_vectors(orc, L)
    vf, bv = fields(syn, L, nc, 110)
    ls = restate_grad(orc, L, V, vf, bv)
    D = Device(env, L, eng.Addressing(ctx, L["n"], L["lo"], L["up"]))
    gd = [E(L["n"]) for _ in range(3 * nc)]
    D.A.ls_grad(D.lsv, [dev(x) for x in vf], gd, bvalue=[dev(x) for x in bv])
    off = 0
    for fc, kd in zip(L["fcs"], L["kinds"]):
        m = fc.shape[0]
        sl = slice(off, off + m)
        off += m
        if kd == COUPLED:
            continue
        s, mag = [x[sl] for x in L["bSf"]], L["bms"][sl]
        dc = 1.0 / np.sqrt(sum(x[sl] * x[sl] for x in L["bd"]))
        sn = [dc * (bv[j][sl] - vf[j][fc]) for j in range(nc)]          # a fixedValue snGrad
        want = gauss_grad_correct(fc, s, mag, sn, ls)
        P = eng.Patch(ctx, L["n"], fc)
        out = [E(m) for _ in range(3 * nc)]
        P.gauss_grad_correct([dev(x) for x in s], dev(mag), [dev(x) for x in sn], gd, out)
        for i in range(3 * nc):
            assert same(host(out[i]), want[i]), (kd, i)
        P.close()
    D.close()


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    fill = -77.0
    env = gpu_env(pkg, fill=fill)
    eng, ctx, dev, host, E = env
    syn = pkg.synthetic
    L = skewed_ls(syn)
    n, nf, nb = L["n"], L["lo"].shape[0], sum(f.shape[0] for f in L["fcs"])
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    other = eng.Addressing(ctx, n, L["lo"], L["up"])
    B, Bo = eng.GradBoundary(addr, L["fcs"], L["kinds"]), eng.GradBoundary(other, L["fcs"], L["kinds"])
    Cd, wd, md, bwd, bmd, bdd = [dev(x) for x in L["C"]], dev(L["w"]), dev(L["magSf"]), dev(L["bw"]), dev(L["bms"]), [dev(x) for x in L["bd"]]
    make = lambda **kw: eng.LsVectors(kw.get("addr", addr), kw.get("B", B), kw.get("C", Cd), kw.get("w", wd), kw.get("m", md), kw.get("bw", bwd),
                                      kw.get("bm", bmd), kw.get("bd", bdd))
    with pytest.raises(eng.MiError, match="another addressing"):
        make(B=Bo)
    with pytest.raises(eng.MiError, match="another addressing"):
        make(addr=other)
    with pytest.raises(eng.MiError, match="centres"):
        make(C=[Cd[0], None, Cd[2]])
    with pytest.raises(eng.MiError, match="centres"):
        make(C=None)
    for key in ("w", "m"):
        with pytest.raises(eng.MiError, match="weights and magSf"):
            make(**{key: None})
    for key in ("bw", "bm", "bd"):
        with pytest.raises(eng.MiError, match="boundary has faces"):
            make(**{key: None})
    with pytest.raises(eng.MiError, match="boundary has faces"):
        make(bd=[bdd[0], bdd[1], None])
    lsv = make()
    A, Ao = eng.Assembly(addr), eng.Assembly(other)
    sentinel = lambda xs: all(bool(torch.all(x == fill)) for x in xs)
    # mi_ls_vectors_fields
    p, nv, bp = [E(nf) for _ in range(3)], [E(nf) for _ in range(3)], [E(nb) for _ in range(3)]
    for bad, why in (((p, nv, None), "boundary has faces"), ((p, [nv[0], p[1], nv[2]], bp), "outputs must differ"),
                     (([p[0], p[1], None], nv, bp), "missing"), ((p, None, bp), "missing")):
        with pytest.raises(eng.MiError, match=why):
            lsv.fields(*bad)
    assert sentinel(p + nv + bp)
    # mi_ls_grad
    vf, bv = fields(syn, L, 3, 120)
    vfd, bvd = [dev(x) for x in vf], [dev(x) for x in bv]
    g = [E(n) for _ in range(9)]
    for args, kw, why in (((vfd[:2], g[:6]), dict(bvalue=bvd[:2]), "n_comp"),
                          (([], []), dict(bvalue=[]), "n_comp"),
                          ((vfd, g), dict(bvalue=None), "boundary has faces"),
                          ((vfd, g), dict(bvalue=[bvd[0], None, bvd[2]]), "missing"),
                          (([vfd[0], None, vfd[2]], g), dict(bvalue=bvd), "missing"),
                          ((vfd, g[:8] + [None]), dict(bvalue=bvd), "missing"),
                          ((vfd, g[:4] + [vfd[1]] + g[5:]), dict(bvalue=bvd), "alias"),
                          ((vfd, g[:4] + [bvd[2]] + g[5:]), dict(bvalue=bvd), "alias"),
                          ((vfd, g[:4] + [g[0]] + g[5:]), dict(bvalue=bvd), "outputs must differ")):
        with pytest.raises(eng.MiError, match=why):
            A.ls_grad(lsv, *args, **kw)
    with pytest.raises(eng.MiError, match="another addressing"):
        Ao.ls_grad(lsv, vfd, g, bvalue=bvd)
    assert sentinel(g)
    assert all(same(host(x), y) for x, y in zip(vfd + bvd, vf + bv))
    A.ls_grad(lsv, vfd, g, bvalue=bvd)                          # the valid call after them writes every value
    assert not any(bool(torch.any(x == fill)) for x in g)
    lsv.close(); B.close(); Bo.close()
