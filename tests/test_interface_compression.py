"""The interfaceCompression scheme (transportModels/interfaceProperties/interfaceCompression/interfaceCompression.H inside
limitedSchemes/PhiScheme/PhiScheme.C) and alphaEqn.H's compression flux in one face pass (mi_interface_compression_weights,
mi_alpha_compression_flux and their coupled-patch forms), bit for bit against the restatement of tests/cmules_support.py."""
import os
import re

import numpy as np
import pytest

from assembly_support import bits, gpu_env, same, set_face_grid, shape_case
from reconstruct_support import skewed_rc
from cmules_support import (ic_inputs, literal_compression_flux, literal_ic_weights, restate_compression_flux_unfused, restate_ic_weights)

EXPORTS = ("mi_interface_compression_parse", "mi_interface_compression_weights", "mi_patch_interface_compression_weights",
           "mi_alpha_compression_flux", "mi_patch_alpha_compression_flux")
NAN = float("nan")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS


def test_the_scheme_word(pkg):
    """exactly `interfaceCompression`: PhiScheme takes no coefficient; the two LimitedScheme parsers go on refusing the word"""
    eng = pkg.engine
    eng.interface_compression("interfaceCompression")
    eng.interface_compression("  interfaceCompression ")
    for bad, why in (("interfaceCompression 1", "no coefficient"), ("vanLeer", "is not interfaceCompression"), ("interfacecompression", "is not"),
                     ("", "empty")):
        with pytest.raises(eng.MiError, match=why):
            eng.interface_compression(bad)
    for parse in (eng.limiter, eng.filtered):
        with pytest.raises(eng.MiError):
            parse("interfaceCompression")


def test_mirror_accepts_the_scheme_word(pkg, tmp_path):
    """foam/miFoam: interfaceCompressionScheme::New parses through mi_interface_compression_parse (no GPU), beside limitedScheme::New and
    filteredScheme::New, and refuses what it refuses; the weights and the flux and their patch forms are in the library"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    src = tmp_path / "ic.C"
    src.write_text('#include "miFoam.H"\n#include <cstdio>\nusing namespace Foam;\nint main(int argc, char** argv)\n{\n'
                   '    for (int i = 1; i < argc; ++i) { const interfaceCompressionScheme s = interfaceCompressionScheme::New(argv[i]); (void)s;\n'
                   '        std::printf("ok %s\\n", argv[i]); }\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "ic"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "foam"), "-I", os.path.join(os.path.dirname(PKG), "include"), str(src), "-o", str(exe),
                    "-L" + PKG, "-lmiFoam", "-lrapidcfd_amd", "-Wl,-rpath," + PKG], check=True, capture_output=True)
    out = subprocess.run([str(exe), "interfaceCompression"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok interfaceCompression\n", out.stderr
    for s, why in (("interfaceCompression 1", "no coefficient"), ("vanLeer", "is not interfaceCompression"), ("filteredLinear", "is not interfaceCompression")):
        bad = subprocess.run([str(exe), s], capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and why in (bad.stdout + bad.stderr), s
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    for name in ("Foam::interfaceCompressionScheme::New(", "Foam::interfaceCompressionWeights(", "Foam::patchInterfaceCompressionWeights(",
                 "Foam::alphaCompressionFlux(", "Foam::patchAlphaCompressionFlux("):
        assert syms.count(" T " + name) == 1, name


def _box(pkg):
    L = skewed_rc(pkg.synthetic)
    return L["n"], L["lo"], L["up"]


def _graph(pkg, name="edge_257"):
    case = shape_case(pkg, name)
    return case.n_cells, case.lower_addr, case.upper_addr


def _meshes(pkg):
    return (("box", _box(pkg), 900), ("edge_257", _graph(pkg), 910))


def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_branch(pkg):
    for name, (n, lo, up), seed in _meshes(pkg):
        alpha, cdw, flux = ic_inputs(pkg.synthetic, n, lo.shape[0], seed)
        P, N = alpha[lo], alpha[up]
        w, lim = restate_ic_weights(cdw, flux, P, N)
        lw, llim = literal_ic_weights(cdw, flux, P, N)
        assert same(w, lw) and same(lim, llim), name
        assert np.all((lim >= 0.0) & (lim <= 1.0))
        edge = (P == 0.0) | (P == 1.0) | (N == 0.0) | (N == 1.0)
        assert np.any(edge) and np.all(lim[edge] == 0.0)                        # a cell at 0 or 1: limiter exactly 0
        mid = (P == 0.5) & (N == 0.5)
        assert np.any(mid) and np.all(lim[mid] == 1.0)                          # both cells at 0.5: limiter exactly 1
        assert np.any((lim > 0.0) & (lim < 1.0))
        assert np.any(alpha < 0.0) and np.any(alpha > 1.0) and np.any((P < 0.0) | (N < 0.0)) and np.any((P > 1.0) | (N > 1.0))
        assert np.any(flux > 0.0) and np.any(flux < 0.0) and np.any((flux == 0.0) & ~np.signbit(flux)) and np.any((flux == 0.0) & np.signbit(flux))
        assert np.all(w[(lim == 0.0) & (flux >= 0)] == 1.0) and np.all(w[(lim == 0.0) & (flux < 0)] == 0.0) and same(w[lim == 1.0], cdw[lim == 1.0])


@pytest.mark.parametrize("patch", [False, True])
def test_the_fused_flux_is_the_unfused_sequence(pkg, patch):
    """the composition written per face (as the kernel writes it) equals the field-by-field sequence, internal faces and coupled patch faces"""
    for name, (n, lo, up), seed in _meshes(pkg):
        alpha, cdw, phir = ic_inputs(pkg.synthetic, n, lo.shape[0], seed)
        got = literal_compression_flux(cdw, phir, alpha[lo], alpha[up], patch)
        want = restate_compression_flux_unfused(cdw, phir, alpha[lo], alpha[up], patch)
        assert same(got, want), name
        assert np.any(want != 0.0) and np.all(np.isfinite(want))


def _patch_case(pkg):
    """a coupled patch of 429 faces (more than one workgroup, no multiple of 256) on every third cell of the 13 x 11 x 9 box; a third of
    the faces see the same value on both sides"""
    n = 13 * 11 * 9
    fc = np.arange(0, n, 3, dtype=np.int32)
    m = fc.shape[0]
    alpha, _, _ = ic_inputs(pkg.synthetic, n, 1, 920)
    nbr, cdw, flux = ic_inputs(pkg.synthetic, m, m, 921)
    nbr[::3] = alpha[fc][::3]
    return n, fc, alpha, nbr, cdw, flux


def test_the_patch_inputs_tell_the_two_interpolation_rules_apart(pkg):
    """w*P + (1 - w)*N with every operator rounded (a coupled patch) against fma(w, P - N, N) (an internal face)"""
    n, fc, alpha, nbr, cdw, flux = _patch_case(pkg)
    assert fc.shape[0] % 256 and fc.shape[0] > 256
    a, b = (restate_compression_flux_unfused(cdw, flux, alpha[fc], nbr, patch=p) for p in (True, False))
    assert not same(a, b) and np.all(np.isfinite(a))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int(np.sum(bits(got) != bits(want))))


def _addressings(eng, ctx, n, lo, up):
    yield "caller", eng.Addressing(ctx, n, lo, up)
    yield "ordered", eng.Addressing(ctx, n, lo, up, ordered=True)


def _unfused_on_the_device(A, dev, host, E, cdw, phir, alpha1):
    """the two weight calls, two mi_face_interpolate, host negations and products"""
    nf = cdw.shape[0]
    a1, a2, c = dev(alpha1), dev(1.0 - alpha1), dev(cdw)
    n = -phir
    w2, i2 = E(nf), E(nf)
    A.interface_compression_weights(c, dev(n), a2, w2)
    A.face_interpolate(w2, a2, i2)
    m = -(n * host(i2))
    w1, i1 = E(nf), E(nf)
    A.interface_compression_weights(c, dev(m), a1, w1)
    A.face_interpolate(w1, a1, i1)
    return m * host(i1)


@pytest.mark.gpu
def test_weights_limiter_and_fused_flux_on_the_box_and_the_graph(pkg):
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    for name, (n, lo, up), seed in _meshes(pkg):
        nf = lo.shape[0]
        alpha, cdw, flux = ic_inputs(pkg.synthetic, n, nf, seed)
        w, lim = restate_ic_weights(cdw, flux, alpha[lo], alpha[up])
        fused = restate_compression_flux_unfused(cdw, flux, alpha[lo], alpha[up])
        for tag, addr in _addressings(eng, ctx, n, lo, up):
            A = eng.Assembly(addr)
            wo, lo_, wo2, fo = E(nf), E(nf), E(nf), E(nf)
            A.interface_compression_weights(dev(cdw), dev(flux), dev(alpha), wo, lo_)
            A.interface_compression_weights(dev(cdw), dev(flux), dev(alpha), wo2)           # without the limiter output
            _eq(host(wo), w, (name, tag, "weights")); _eq(host(lo_), lim, (name, tag, "limiter")); _eq(host(wo2), w, (name, tag, "weights alone"))
            A.alpha_compression_flux(dev(cdw), dev(flux), dev(alpha), fo)
            _eq(host(fo), fused, (name, tag, "fused against the restatement"))
            _eq(host(fo), _unfused_on_the_device(A, dev, host, E, cdw, flux, alpha), (name, tag, "fused against the device's unfused sequence"))


@pytest.mark.gpu
def test_the_patch_forms_on_a_coupled_patch(pkg):
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    n, fc, alpha, nbr, cdw, flux = _patch_case(pkg)
    m = fc.shape[0]
    P = eng.Patch(ctx, n, fc)
    w, lim = restate_ic_weights(cdw, flux, alpha[fc], nbr)
    wo, lo_, fo = E(m), E(m), E(m)
    P.interface_compression_weights(dev(cdw), dev(flux), dev(alpha), dev(nbr), wo, lo_)
    _eq(host(wo), w, "patch weights"); _eq(host(lo_), lim, "patch limiter")
    wo2 = E(m)
    P.interface_compression_weights(dev(cdw), dev(flux), dev(alpha), dev(nbr), wo2)
    _eq(host(wo2), w, "patch weights alone")
    P.alpha_compression_flux(dev(cdw), dev(flux), dev(alpha), dev(nbr), fo)
    _eq(host(fo), restate_compression_flux_unfused(cdw, flux, alpha[fc], nbr, patch=True), "patch fused flux")


_GRID = {}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3, 8, 11])
def test_face_grids(pkg, monkeypatch, blocks):
    """both face passes walking their block_chunk loops: MI_FACE_GRID at 1, 3, 8 and 11 workgroups on the 13 x 11 x 9 box"""
    set_face_grid(monkeypatch, blocks)
    env = gpu_env(pkg, fill=NAN)
    eng, ctx, dev, host, E = env
    case = pkg.synthetic.box_case(13, 11, 9)
    n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
    nf = lo.shape[0]
    assert nf % 256 and nf > 256 * 11
    if not _GRID:
        alpha, cdw, flux = ic_inputs(pkg.synthetic, n, nf, 930)
        w, lim = restate_ic_weights(cdw, flux, alpha[lo], alpha[up])
        _GRID.update(alpha=alpha, cdw=cdw, flux=flux, w=w, lim=lim, fused=restate_compression_flux_unfused(cdw, flux, alpha[lo], alpha[up]))
    g = _GRID
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    wo, lo_, fo = E(nf), E(nf), E(nf)
    A.interface_compression_weights(dev(g["cdw"]), dev(g["flux"]), dev(g["alpha"]), wo, lo_)
    A.alpha_compression_flux(dev(g["cdw"]), dev(g["flux"]), dev(g["alpha"]), fo)
    _eq(host(wo), g["w"], ("weights", blocks)); _eq(host(lo_), g["lim"], ("limiter", blocks)); _eq(host(fo), g["fused"], ("fused", blocks))


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
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    L = skewed_rc(pkg.synthetic)
    n, lo, up = L["n"], L["lo"], L["up"]
    nf = lo.shape[0]
    alpha, cdw, flux = ic_inputs(pkg.synthetic, n, nf, 940)
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    a, c, f = dev(alpha), dev(cdw), dev(flux)
    w, lim, spare = E(nf), E(nf), E(nf + 1)
    for args, why in (((None, f, a, w, lim), "missing"), ((c, None, a, w, lim), "missing"), ((c, f, None, w, lim), "missing"), ((c, f, a, None, lim), "missing"),
                      ((c, f, a, w, w), "must differ"), ((c, f, a, c, lim), "alias"), ((c, f, a, w, f), "alias"),
                      ((Misaligned(spare), f, a, w, lim), "aligned"), ((c, f, a, Misaligned(spare), lim), "aligned"), ((c, f, Misaligned(spare), w, lim), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.interface_compression_weights(*args)
    for args, why in (((None, f, a, w), "missing"), ((c, f, None, w), "missing"), ((c, f, a, None), "missing"), ((c, f, a, f), "alias"),
                      ((c, f, a, Misaligned(spare)), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            A.alpha_compression_flux(*args)
    fc = [x for x, k in zip(L["fcs"], L["kinds"]) if k == 1][0]
    m = fc.shape[0]
    P = eng.Patch(ctx, n, fc)
    pc, pf, pn, pw, pl = dev(cdw[:m]), dev(flux[:m]), dev(alpha[fc]), E(m), E(m)
    for args, why in (((pc, pf, a, None, pw, pl), "missing"), ((pc, pf, a, pn, None, pl), "missing"), ((pc, pf, a, pn, pw, pw), "must differ"),
                      ((pc, pf, a, pn, pn, pl), "alias"), ((pc, pf, a, pn, Misaligned(spare), pl), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            P.interface_compression_weights(*args)
    for args, why in (((pc, pf, None, pn, pw), "missing"), ((pc, pf, a, pn, pc), "alias"), ((pc, Misaligned(spare), a, pn, pw), "aligned")):
        with pytest.raises(eng.MiError, match=why):
            P.alpha_compression_flux(*args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(y == fill)) for y in (w, lim, spare, pw, pl))
    assert same(host(c), cdw) and same(host(f), flux) and same(host(a), alpha) and same(host(pn), alpha[fc])
    A.interface_compression_weights(c, f, a, w, lim)            # the valid calls after them write every value
    P.alpha_compression_flux(pc, pf, a, pn, pw)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(y == fill)) for y in (w, lim, pw))
