"""fvc::reconstruct and fvc::surfaceSum (finiteVolume/fvc/fvcReconstruct.C, fvcSurfaceIntegrate.C): the inverse geometric tensor built once per
mesh on the device (mi_reconstruct_create), the reconstruction of up to four fluxes as one row pass (mi_fvc_reconstruct) and mi_surface_sum,
bit for bit against the restatement of tests/reconstruct_support.py -- restated, not pinned by a compiled reference."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from assembly_support import (DEGENERATE_MESHES, OTHER_TABLES, ROW_MODES, bits, block_counts, fma, gpu_env, same, set_row_blocks, set_row_tables,
                              shape_case, shaped_addressing)
from least_squares_support import all_finite
from reconstruct_support import (boundary_cells, faceless_cells, flat_rc, fluxes, literal_build, literal_flux, literal_inputs, literal_reconstruct,
                                 literal_surface_sum, restate_build, restate_reconstruct, restate_surface_sum, seeded_rc, skewed_rc)

EXPORTS = ("mi_surface_sum", "mi_reconstruct_create", "mi_reconstruct_destroy", "mi_reconstruct_fields", "mi_fvc_reconstruct")
FACELESS = ("one_cell", "no_faces", "isolated")
MESHES = {"skewed": skewed_rc, "flat": flat_rc}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    assert "typedef struct mi_reconstruct_s *mi_reconstruct_t;" in header
    assert "enum { MI_SURFACE_SUM, MI_SURFACE_SUM_MAG };" in header
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "Foam::reconstructData::reconstructData(" in syms and "Foam::reconstructData::fields(" in syms
    assert syms.count(" T Foam::fvc::reconstruct(") == 2                    # one flux, and up to four
    assert " T Foam::fvc::surfaceSum(" in syms and " T Foam::fvc::surfaceSumPatch(" in syms


def _columns(rows, m):
    return [np.array([r[k] for r in rows], dtype=np.float64) for k in range(m)]


@pytest.mark.parametrize("mesh", ["skewed", "flat"])
def test_restatement_equals_the_literal_loops(pkg, orc, mesh):
    """the vectorised restatement against the loops written out: SfHat, the inverse, removeCmpts and the reconstruction of one and of three fluxes"""
    syn = pkg.synthetic
    L = MESHES[mesh](syn)
    n = L["n"]
    lo, up, Sf, magSf, patches = literal_inputs(L)
    hat, phat, R, removed = literal_build(n, lo, up, Sf, magSf, patches)
    B = restate_build(orc, L)
    assert tuple(int(x) for x in removed) == B["removed"]
    assert all(same(x, y) for x, y in zip(_columns(hat, 3), B["hat"]))
    assert all(same(x, y) for x, y in zip(_columns([h for p in phat for h in p], 3), B["bhat"]))
    assert all(same(x, y) for x, y in zip(_columns(R, 9), B["inv"]))
    for n_rhs in (1, 3):
        ssf, bssf = fluxes(syn, L, n_rhs, 40 + n_rhs)
        for r in range(n_rhs):
            v, pv = literal_flux(L, ssf[r], bssf[r])
            lit = _columns(literal_reconstruct(n, lo, up, hat, phat, R, v, pv, fma), 3)
            got = restate_reconstruct(orc, L, B, ssf[r], bssf[r])
            assert all(same(x, y) for x, y in zip(lit, got)), (n_rhs, r)
            assert all_finite(lit) and np.any(lit[0] != 0.0)


@pytest.mark.parametrize("mag", [False, True])
def test_surface_sum_restatement_equals_the_literal_loops(pkg, orc, mag):
    syn = pkg.synthetic
    L = skewed_rc(syn)
    (ssf,), (bssf,) = fluxes(syn, L, 1, 47)
    v, pv = literal_flux(L, ssf, bssf)
    lit = np.array(literal_surface_sum(L["n"], L["lo"].tolist(), L["up"].tolist(), v, pv, mag=mag))
    assert same(lit, restate_surface_sum(orc, L, ssf, bssf, mag=mag))
    if mag:
        assert np.all(lit > 0.0)


def test_literal_loops_reconstruct_a_uniform_vector_exactly(pkg):
    """exact rational arithmetic, no tolerance: the flux U & Sf of a uniform U reconstructs to U in every (closed or open) cell -- a minus on the
    neighbour side, a wrong cofactor or a transposed inverse all break it"""
    F = Fraction
    L = skewed_rc(pkg.synthetic)
    n = L["n"]
    lo, up, Sf, magSf, patches = literal_inputs(L, F)
    hat, phat, R, removed = literal_build(n, lo, up, Sf, magSf, patches, one=F(1))
    assert removed == [False, False, False]
    U = [F(7, 10), F(-13, 10), F(9, 20)]
    dot = lambda s: U[0] * s[0] + U[1] * s[1] + U[2] * s[2]
    out = literal_reconstruct(n, lo, up, hat, phat, R, [dot(s) for s in Sf], [(fc, [dot(s) for s in pS]) for fc, pS, _ in patches],
                              lambda x, y, z: x * y + z, zero=F(0))
    assert all(row == U for row in out)


def test_one_cell_thick_mesh_removes_z(pkg, orc):
    syn = pkg.synthetic
    L = flat_rc(syn)
    B = restate_build(orc, L)
    assert B["removed"] == (0, 0, 1)
    assert all_finite(B["inv"])
    ssf, bssf = fluxes(syn, L, 3, 50)
    for r in range(3):
        out = restate_reconstruct(orc, L, B, ssf[r], bssf[r])
        assert all_finite(out)
        assert np.all(out[2] == 0.0) and np.any(out[0] != 0.0) and np.any(out[1] != 0.0)


def _seeded(pkg, name, seed=400):
    case = shape_case(pkg, name)
    return seeded_rc(pkg.synthetic, case.n_cells, case.lower_addr, case.upper_addr, seed)


def test_the_restatement_is_finite_on_the_closed_meshes(pkg, orc):
    syn = pkg.synthetic
    for make in (skewed_rc, flat_rc):
        L = make(syn)
        B = restate_build(orc, L)
        ssf, bssf = fluxes(syn, L, 1, 55)
        assert all_finite(B["inv"] + restate_reconstruct(orc, L, B, ssf[0], bssf[0]))
        assert faceless_cells(L).shape[0] == 0


@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_on_the_seeded_graphs_only_the_faceless_cells_are_not_finite(pkg, orc, name):
    """what the GPU comparison may skip: exactly the cells without any face, nothing more"""
    syn = pkg.synthetic
    L = _seeded(pkg, name)
    B = restate_build(orc, L)
    ssf, bssf = fluxes(syn, L, 1, 56)
    empty = np.zeros(L["n"], bool)
    empty[faceless_cells(L)] = True
    assert bool(empty.any()) == (name in FACELESS)
    for x in B["inv"] + restate_reconstruct(orc, L, B, ssf[0], bssf[0]):
        assert np.array_equal(~np.isfinite(x), empty)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
class Device:
    """one mesh under one addressing on the device: the boundary (or none), the handle and an Assembly"""

    def __init__(self, env, L, addr, boundary=True):
        self.eng, self.ctx, self.dev, self.host, self.E = env
        eng, dev = self.eng, self.dev
        self.L, self.addr = L, addr
        self.A = eng.Assembly(addr)
        self.B = eng.GradBoundary(addr, L["fcs"], L["kinds"]) if boundary else None
        self.rc = eng.Reconstruct(addr, self.B, [dev(x) for x in L["Sf"]], dev(L["magSf"]),
                                  [dev(x) for x in L["bSf"]] if boundary else None, dev(L["bms"]) if boundary else None)

    def fields(self):
        out = [self.E(self.L["n"]) for _ in range(9)]
        removed = self.rc.fields(out)
        return [self.host(x) for x in out], removed

    def reconstruct(self, ssf, bssf):
        out = [self.E(self.L["n"]) for _ in range(3 * len(ssf))]
        self.A.reconstruct(self.rc, [self.dev(x) for x in ssf], out, b_ssf=None if bssf is None else [self.dev(x) for x in bssf])
        return [self.host(x) for x in out]

    def close(self):
        self.rc.close()
        if self.B is not None:
            self.B.close()


def _addressings(eng, ctx, L):
    """the caller's numbering, and the same numbering under ordered addressing"""
    yield "caller", eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    yield "ordered", eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=True)


def _agree(got, want, tag):
    """bit for bit wherever the restatement is finite; elsewhere the engine's value is not finite either"""
    fin = np.isfinite(want)
    assert np.array_equal(bits(got)[fin], bits(want)[fin]), (tag, int(np.sum(bits(got)[fin] != bits(want)[fin])))
    assert not np.isfinite(got[~fin]).any(), tag


def _reference(orc, syn, L, seed, counts=(1, 2, 3, 4)):
    """-> (B, {n_rhs: (ssf, bssf, out[3*r + k])}); the four fluxes are seeded once, n_rhs takes the first n_rhs of them"""
    B = restate_build(orc, L)
    ssf, bssf = fluxes(syn, L, 4, seed)
    outs = [restate_reconstruct(orc, L, B, ssf[r], bssf[r]) for r in range(max(counts))]
    return B, {k: (ssf[:k], bssf[:k], [x for r in range(k) for x in outs[r]]) for k in counts}


def _check(D, ref, tag):
    B, runs = ref
    inv, removed = D.fields()
    assert removed == B["removed"], tag
    for i in range(9):
        _agree(inv[i], B["inv"][i], (tag, "inverse", i))
    for k, (ssf, bssf, want) in runs.items():
        got = D.reconstruct(ssf, bssf)
        for i in range(3 * k):
            _agree(got[i], want[i], (tag, "reconstruct", k, i))


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["skewed", "flat"])
def test_fields_and_reconstruction_against_the_restatement(pkg, orc, mesh):
    """the inverse, removeCmpts and n_rhs = 1..4 on the skewed 5x4x3 box and on the one-cell-thick mesh that removes z, in the caller's numbering
    and under ordered addressing; the fluxes carry exact zeros of both signs; n_rhs = k equals k single calls"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    L = MESHES[mesh](syn)
    ref = _reference(orc, syn, L, 60)
    assert all_finite(ref[0]["inv"] + ref[1][4][2])
    assert ref[0]["removed"] == ((0, 0, 1) if mesh == "flat" else (0, 0, 0))
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _check(D, ref, (mesh, tag))
        ssf, bssf, _ = ref[1][4]
        four = D.reconstruct(ssf, bssf)
        for r in range(4):
            one = D.reconstruct(ssf[r:r + 1], bssf[r:r + 1])
            assert all(same(one[k], four[3 * r + k]) for k in range(3)), (mesh, tag, r)
        if mesh == "flat":
            assert all(np.all(four[3 * r + 2] == 0.0) for r in range(4))
        D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEGENERATE_MESHES)
def test_degenerate_meshes(pkg, orc, name):
    """cells and meshes without faces (a non-finite inverse and output there, and nowhere else), hubs of thousands of faces, cell counts around
    the block boundaries, dense rows"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    L = _seeded(pkg, name)
    ref = _reference(orc, syn, L, 70, counts=(1, 4))
    for tag, addr in _addressings(eng, ctx, L):
        D = Device(env, L, addr)
        _check(D, ref, (name, tag))
        D.close()


_SHAPE_REFS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("tables, mode", [("default", m) for m in ROW_MODES] + OTHER_TABLES)
def test_every_row_pass_shape(pkg, orc, monkeypatch, tables, mode):
    """gradient-plan blocks of 256 / 1024 cells, the layout's tiles under ordered addressing, the unstaged fall-back (MI_ROW_CAP=64), the 32-bit
    row tables and the plain block mapping, n_rhs 1 and 4: everything equals the restatement, hence each other across the shapes"""
    set_row_tables(monkeypatch, tables)
    set_row_blocks(monkeypatch, mode, grad=True)
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    for name in ("box", "graph"):
        case, addr = shaped_addressing(eng, ctx, syn, shape_case(pkg, name, symmetric=True), mode)
        cache = _SHAPE_REFS.setdefault((name, mode.startswith("tiles")), {})
        if not cache:
            L = seeded_rc(syn, case.n_cells, case.lower_addr, case.upper_addr, 500)
            cache.update(L=L, ref=_reference(orc, syn, L, 80, counts=(1, 4)))
            assert all_finite(cache["ref"][0]["inv"] + cache["ref"][1][4][2])
        L = cache["L"]
        assert np.array_equal(L["lo"], case.lower_addr) and np.array_equal(L["up"], case.upper_addr)
        if mode == "fixed1024":
            # box: the largest block's own faces fit the 156 KiB of one resident workgroup with six staged arrays and not with seven, so
            # n_rhs 4 stages SfHat and three fluxes and reads the fourth from global memory; graph: not even SfHat alone fits, every call
            # stages what the smaller blocks hold and the largest takes the unstaged path
            own, fit = int(block_counts(case, 1024)[0].max()), lambda arrays: 156 * 1024 // 8 // arrays
            assert (fit(7) < own <= fit(6)) if name == "box" else own > fit(3), (name, own)
        D = Device(env, L, addr)
        _check(D, cache["ref"], (name, tables, mode))
        D.close()


@pytest.mark.gpu
def test_no_boundary_and_coupled_as_other(pkg, orc):
    """boundary NULL on a mesh given no patches; a coupled patch gives the bits of the same faces declared `other` (the kinds are not read)"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx = env[0], env[1]
    syn = pkg.synthetic
    L = skewed_rc(syn)
    bare = dict(L, fcs=[], kinds=[], bSf=[np.zeros(0)] * 3, bms=np.zeros(0))
    B = restate_build(orc, bare)
    ssf, _ = fluxes(syn, L, 2, 90)
    none = np.zeros(0)
    want = [x for r in range(2) for x in restate_reconstruct(orc, bare, B, ssf[r], none)]
    assert all_finite(want)
    addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    D = Device(env, bare, addr, boundary=False)
    inv, removed = D.fields()
    assert removed == B["removed"] and all(same(x, y) for x, y in zip(inv, B["inv"]))
    assert all(same(x, y) for x, y in zip(D.reconstruct(ssf, None), want))
    D.close()
    assert 1 in L["kinds"]
    ssf, bssf = fluxes(syn, L, 2, 91)
    runs = []
    for kinds in (L["kinds"], [0] * len(L["kinds"])):
        D = Device(env, dict(L, kinds=kinds), addr)
        runs.append(D.fields()[0] + D.reconstruct(ssf, bssf))
        D.close()
    assert all(same(x, y) for x, y in zip(*runs))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skewed", "hub_first", "isolated", "edge_1025"])
def test_surface_sum(pkg, orc, name):
    """both modes on the internal faces, then the patches with Patch.add (fn 0 / fn 2), against the restatement; and against row_face_op on
    a zeroed array, the pass it wraps"""
    env = gpu_env(pkg, fill=-77.0)
    eng, ctx, dev, host, E = env
    syn = pkg.synthetic
    L = skewed_rc(syn) if name == "skewed" else _seeded(pkg, name)
    (ssf,), (bssf,) = fluxes(syn, L, 1, 95)
    n = L["n"]
    for tag, addr in _addressings(eng, ctx, L):
        A = eng.Assembly(addr)
        for mode, mag in (("sum", False), ("mag", True)):
            out = E(n)
            A.surface_sum(dev(ssf), out, mode)
            assert same(host(out), restate_surface_sum(orc, L, ssf, None, mag=mag)), (name, tag, mode)
            zero = dev(np.zeros(n))
            A.row_face_op(2 if mag else 0, None, dev(ssf), zero)
            assert same(host(out), host(zero)), (name, tag, mode)
            off = 0
            for fc in L["fcs"]:
                P = eng.Patch(ctx, n, fc)
                P.add(dev(bssf[off:off + fc.shape[0]]), out, 2 if mag else 0)
                P.close()
                off += fc.shape[0]
            assert same(host(out), restate_surface_sum(orc, L, ssf, bssf, mag=mag)), (name, tag, mode, "patches")


class Misaligned:
    """a device address four bytes into a float64 tensor, as engine._ptr takes one: not aligned for a double"""

    def __init__(self, t):
        self.t, self.dtype = t, t.dtype

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def data_ptr(self):
        return self.t.data_ptr() + 4


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    fill = -77.0
    env = gpu_env(pkg, fill=fill)
    eng, ctx, dev, host, E = env
    syn = pkg.synthetic
    L = skewed_rc(syn)
    n, nf, nb = L["n"], L["lo"].shape[0], sum(f.shape[0] for f in L["fcs"])
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    other = eng.Addressing(ctx, n, L["lo"], L["up"])
    B, Bo = eng.GradBoundary(addr, L["fcs"], L["kinds"]), eng.GradBoundary(other, L["fcs"], L["kinds"])
    Sd, md, bSd, bmd = [dev(x) for x in L["Sf"]], dev(L["magSf"]), [dev(x) for x in L["bSf"]], dev(L["bms"])
    make = lambda **kw: eng.Reconstruct(kw.get("addr", addr), kw.get("B", B), kw.get("S", Sd), kw.get("m", md), kw.get("bS", bSd), kw.get("bm", bmd))
    sentinel = lambda xs: all(bool(torch.all(x == fill)) for x in xs)
    # mi_reconstruct_create
    for kw, why in ((dict(B=Bo), "another addressing"), (dict(addr=other), "another addressing"), (dict(S=None), "missing"),
                    (dict(S=[Sd[0], None, Sd[2]]), "missing"), (dict(m=None), "missing"), (dict(bS=None), "boundary has faces"),
                    (dict(bS=[bSd[0], bSd[1], None]), "boundary has faces"), (dict(bm=None), "boundary has faces"),
                    (dict(m=Misaligned(E(nf + 1))), "aligned"), (dict(bS=[bSd[0], Misaligned(E(nb + 1)), bSd[2]]), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            make(**kw)
    rc = make()
    A, Ao = eng.Assembly(addr), eng.Assembly(other)
    # mi_reconstruct_fields
    inv = [E(n) for _ in range(9)]
    for bad, why in ((None, "missing"), (inv[:8] + [None], "missing"), (inv[:4] + [inv[0]] + inv[5:], "outputs must differ"),
                     (inv[:8] + [Misaligned(E(n + 1))], "aligned")):
        with pytest.raises(eng.MiError, match=why):
            rc.fields(bad)
    assert sentinel(inv)
    # mi_fvc_reconstruct
    ssf, bssf = fluxes(syn, L, 4, 120)
    sd, bd = [dev(x) for x in ssf], [dev(x) for x in bssf]
    out = [E(n) for _ in range(12)]
    spare = E(nf + 1)
    for args, kw, why in ((([], []), dict(b_ssf=[]), "n_rhs"),
                          ((sd + sd[:1], out + out[:3]), dict(b_ssf=bd + bd[:1]), "n_rhs"),
                          ((sd, out), dict(b_ssf=None), "boundary has faces"),
                          ((sd, out), dict(b_ssf=[bd[0], None, bd[2], bd[3]]), "missing"),
                          (([sd[0], None, sd[2], sd[3]], out), dict(b_ssf=bd), "missing"),
                          ((sd, out[:11] + [None]), dict(b_ssf=bd), "missing"),
                          ((sd, None), dict(b_ssf=bd), "missing"),
                          (([sd[0], Misaligned(spare), sd[2], sd[3]], out), dict(b_ssf=bd), "aligned"),
                          ((sd, out[:5] + [Misaligned(E(n + 1))] + out[6:]), dict(b_ssf=bd), "aligned"),
                          ((sd, out[:4] + [sd[1]] + out[5:]), dict(b_ssf=bd), "alias"),
                          ((sd, out[:4] + [bd[2]] + out[5:]), dict(b_ssf=bd), "alias"),
                          ((sd, out[:4] + [out[0]] + out[5:]), dict(b_ssf=bd), "outputs must differ")):
        with pytest.raises(eng.MiError, match=why):
            A.reconstruct(rc, *args, **kw)
    with pytest.raises(eng.MiError, match="another addressing"):
        Ao.reconstruct(rc, sd, out, b_ssf=bd)
    assert sentinel(out) and bool(torch.all(spare == fill))
    assert all(same(host(x), y) for x, y in zip(sd + bd, ssf + bssf))
    A.reconstruct(rc, sd, out, b_ssf=bd)                        # the valid call after them writes every value
    assert not any(bool(torch.any(x == fill)) for x in out)
    # mi_surface_sum
    o = E(n)
    for args, why in (((sd[0], o, 2), "mode"), ((sd[0], o, -1), "mode"), ((None, o, "sum"), "missing"), ((sd[0], None, "mag"), "missing"),
                      ((Misaligned(spare), o, "sum"), "aligned"), ((sd[0], Misaligned(E(n + 1)), "sum"), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.surface_sum(*args)
    with pytest.raises(eng.MiError, match="alias"):
        A.surface_sum(o, o, "sum")                              # refused before anything reads the cell array as a face array
    assert sentinel([o]) and bool(torch.all(spare == fill))
    rc.close(); B.close(); Bo.close()
