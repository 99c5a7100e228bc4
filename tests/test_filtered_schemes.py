"""The filtered centred limiters of resolved runs -- filteredLinear, filteredLinear2[V] k l, filteredLinear3[V] k (limitedSchemes/
filteredLinear/filteredLinear.H:69-94, filteredLinear2/filteredLinear2.H:80-141, filteredLinear2V.H:80-152, filteredLinear3/
filteredLinear3.H:72-107, filteredLinear3V.H:72-112): mi_filtered_parse on the host, the restatements of tests/filtered_support.py against
each other and on hand-computed faces (CPU), then mi_filtered_weights / mi_patch_filtered_weights against the numpy restatement, bit for bit
on every face (gpu).  Restated from the headers, not pinned by compiled reference functors."""
import ctypes as C
import os

import numpy as np
import pytest

import filtered_support as fs
import test_limited_schemes as tl
from assembly_support import bits, gpu_env, same, set_face_grid, set_row_tables
from test_scheme_words import WHITESPACE, fields, padded


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _mesh(pkg, name):
    from conftest import random_graph_case
    if name == "box":
        return tl._graded_box(pkg, (9, 8, 7))
    case = random_graph_case(pkg, 600, extra=3.0, seed=13)
    return case, [pkg.synthetic.splitmix_uniform(90 + k, case.n_cells) for k in range(3)]


def _inputs(pkg, case, seed):
    """the fields of tests/test_limited_schemes.py (zero fluxes of both signs, equal and nearly equal neighbours, zero gradients), and on
    every 97th face both cells made equal in all three components with zero gradients: df = tdcP = tdcN = 0 in the V forms too"""
    flux, cdw, phi, grad = tl._fields(pkg, case.n_cells, case.n_faces, seed)
    for f in range(0, case.n_faces, 97):
        P, N = int(case.lower_addr[f]), int(case.upper_addr[f])
        for p in phi:
            p[N] = p[P]
        for g in grad:
            g[P] = g[N] = 0.0
    return flux, cdw, phi, grad


def _restate_all(pkg, name, seed, hit):
    """-> {scheme string: (weights, limiter)} of every scheme on a mesh, and the inputs"""
    case, Cc = _mesh(pkg, name)
    flux, cdw, phi, grad = _inputs(pkg, case, seed)
    D = fs.internal_differences(case.lower_addr, case.upper_addr, phi, grad, Cc)
    ref = {s: D.weights(kind, vec, k, l, cdw, flux, hit) for s, _, kind, vec, k, l in fs.schemes()}
    return case, Cc, (flux, cdw, phi, grad), ref


# ---- CPU: the parser ---------------------------------------------------------------------------------------------------------------
def test_parse_accepts_the_five_registered_names(pkg):
    eng = pkg.engine
    assert eng.FILTERED_KINDS == ("filteredLinear", "filteredLinear2", "filteredLinear3")
    got = lambda s: (lambda f: (f.kind, f.vector_form, f.k, f.l))(eng.filtered(s))
    assert got("filteredLinear") == (0, 0, 0.0, 0.0)
    assert got("filteredLinear2 0.25 0.5") == (1, 0, 0.25, 0.5)          # l as written: the engine adds the constructor's 1.0
    assert got("filteredLinear2V 0.25 0.5") == (1, 1, 0.25, 0.5)
    assert got("filteredLinear3 0.33") == (2, 0, 0.33, 0.0)
    assert got("filteredLinear3V 0.33") == (2, 1, 0.33, 0.0)
    for k in ("0", "1"):                                                 # both ends of [0, 1]
        assert got("filteredLinear3 " + k)[2] == float(k) and got("filteredLinear3V " + k)[2] == float(k)
        for l in ("0", "1"):
            assert got(f"filteredLinear2 {k} {l}")[2:] == (float(k), float(l)) and got(f"filteredLinear2V {k} {l}")[2:] == (float(k), float(l))
    assert len(fs.schemes()) == 1 + 9 + 9 + 3 + 3
    for s, name, kind, vec, k, l in fs.schemes():
        assert got(s) == (kind, int(vec), k or 0.0, l or 0.0), s
        assert eng.FILTERED_KINDS[kind] == name.rstrip("V")


@pytest.mark.parametrize("scheme, why", [
    ("filteredLinearV", "unknown"), ("filteredLinear2V01 1 0", "unknown"), ("filteredLinear4 1", "unknown"), ("filteredlinear", "unknown"),
    ("limitedLinear 1", "unknown"), ("limitedCubicV 1", "unknown"), ("vanLeer", "unknown"), ("SFCD", "unknown"), ("Gamma01 1", "unknown"),
    ("linear", "unknown"), ("cubic", "unknown"), ("", "empty"),
    ("filteredLinear 1", "extra"), ("filteredLinear2 1 0 0", "extra"), ("filteredLinear2V 1 0 0.5", "extra"), ("filteredLinear3 1 0", "extra"),
    ("filteredLinear3V 1 1", "extra"),
    ("filteredLinear2", "takes 2"), ("filteredLinear2 1", "takes 2"), ("filteredLinear2V 0.5", "takes 2"), ("filteredLinear3", "takes 1"),
    ("filteredLinear3V", "takes 1"),
    ("filteredLinear2 x 0", "not a number"), ("filteredLinear2 1 0.5a", "not a number"), ("filteredLinear3V k", "not a number"),
    ("filteredLinear3 1,", "not a number"),
    ("filteredLinear2 1.5 0", "k should be"), ("filteredLinear2V -0.1 0", "k should be"), ("filteredLinear3 1.0001", "k should be"),
    ("filteredLinear3V -1", "k should be"), ("filteredLinear3 nan", "k should be"),
    ("filteredLinear2 1 1.5", "l should be"), ("filteredLinear2V 0 -0.5", "l should be"), ("filteredLinear2 0.5 inf", "l should be"),
])
def test_parse_refuses_and_leaves_the_struct_untouched(pkg, scheme, why):
    eng = pkg.engine
    with pytest.raises(eng.MiError, match=why):
        eng.filtered(scheme)
    out = eng.FilteredLimiter(-7, -7, -7.5, -7.5)                        # a refused call writes nothing
    before = bytes(out)
    assert eng.lib().mi_filtered_parse(scheme.encode(), C.byref(out)) != 0
    assert bytes(out) == before


def test_parse_whitespace(pkg):
    eng = pkg.engine
    for clean in ("filteredLinear", "filteredLinear2V 0.25 0.5", "filteredLinear3 0.33"):
        want = fields(eng.filtered(clean))
        for text in padded(clean):
            assert fields(eng.filtered(text)) == want, text
    with pytest.raises(eng.MiError, match="empty"):
        eng.filtered(WHITESPACE)


def test_the_limited_parser_still_refuses_the_filtered_names(pkg):
    eng = pkg.engine
    for s in ("filteredLinear", "filteredLinear2 1 0", "filteredLinear2V 1 0", "filteredLinear3 1", "filteredLinear3V 1"):
        with pytest.raises(eng.MiError, match="unknown"):
            eng.limiter(s)
    assert len(eng.LIMITER_KINDS) == 12


def test_library_exports_the_entry_points(pkg):
    for name in ("mi_filtered_parse", "mi_filtered_weights", "mi_patch_filtered_weights"):
        assert hasattr(pkg.engine.lib(), name) and name in pkg.engine.SYMBOLS, name


# ---- CPU: the restatements -----------------------------------------------------------------------------------------------------------
def test_restatement_semantics():
    """one hand-computed face each, on the scalar-by-scalar restatement"""
    L = fs.limiter_face
    d = [1.0, 0.0, 0.0]
    g = lambda x: [x, 0.0, 0.0]
    z = g(0.0)
    # filteredLinear2, df > 0: df = 1, tdcP = 0.5, tdcN = 1.5: min(max(0.5, 0), max(-0.5, 0)) = 0 -> l_ = 1 -> 1
    assert L("filteredLinear2", 1.0, 0.0, 0.0, 1.0, g(0.25), g(0.75), d) == 1.0
    # ... both cells flatter than the face: tdcP = 0.5, tdcN = 0.25: min(0.5, 0.75) = 0.5; den = 1 + SMALL -> 1 - 0.5/(1 + 1e-15)
    assert L("filteredLinear2", 1.0, 0.0, 0.0, 1.0, g(0.25), g(0.125), d) == 1.0 - 0.5 / (1.0 + 1e-15)
    assert L("filteredLinear2", 0.5, 0.0, 0.0, 1.0, g(0.25), g(0.125), d) == 1.0 - 0.25 / (1.0 + 1e-15)
    # df <= 0: the mirrored branch, df = -1: max(tdcP - df, 0) = 0.5, max(tdcN - df, 0) = 0.75
    assert L("filteredLinear2", 1.0, 0.0, 1.0, 0.0, g(-0.25), g(-0.125), d) == 1.0 - 0.5 / (1.0 + 1e-15)
    # df == 0 takes the second branch: tdcP = 0.5, tdcN = 1: min(0.5, 1)/ (1 + SMALL)
    assert L("filteredLinear2", 1.0, 0.0, 0.3, 0.3, g(0.25), g(0.5), d) == 1.0 - 0.5 / (1.0 + 1e-15)
    # df = tdcP = tdcN = 0: l_ - 0/(0 + SMALL) = l_ >= 1 -> 1, and 0/(0 + VSMALL) in the V form
    for l in (0.0, 0.5, 1.0):
        assert L("filteredLinear2", 1.0, l, 0.3, 0.3, z, z, d) == 1.0
        assert L("filteredLinear2V", 1.0, l, [0.3] * 3, [0.3] * 3, z * 3, z * 3, d) == 1.0
    # l = 1: the limiter starts at 2 and is clamped to 1 while k*m/den <= 1: the face that gave 0.5 above now gives 1
    assert L("filteredLinear2", 1.0, 1.0, 0.0, 1.0, g(0.25), g(0.125), d) == 1.0
    assert L("filteredLinear2", 1.0, 0.0, 0.0, 1.0, z, z, d) == 1.0 - 1.0 / (1.0 + 1e-15)      # fully limited without the overshoot allowance
    assert L("filteredLinear2", 1.0, 1.0, 0.0, 1.0, z, z, d) == 1.0                          # 2 - 1/(1 + SMALL) is just above 1 -> 1
    # k = 0 gives 1 in every kind that reads k
    for name, pP, pN, gP, gN in (("filteredLinear2", 0.0, 1.0, z, z), ("filteredLinear3", 0.0, 1.0, z, g(3.0)),
                                 ("filteredLinear2V", [0.0] * 3, [1.0, 2.0, 3.0], z * 3, g(1.0) * 3),
                                 ("filteredLinear3V", [0.0] * 3, [1.0, 2.0, 3.0], z * 3, g(1.0) * 3)):
        assert L(name, 0.0, 0.0, pP, pN, gP, gN, d) == 1.0, name
    # filteredLinear3: dP = 0.5, dN = 1.5, df = 1: 1 - (1*0.5)*(-0.5)/4 = 1.0625 -> 1;  dP = dN = 0.5: 1 - 0.25/1 = 0.75
    assert L("filteredLinear3", 1.0, None, 0.0, 1.0, g(0.25), g(0.75), d) == 1.0
    assert L("filteredLinear3", 1.0, None, 0.0, 1.0, g(0.25), g(0.25), d) == 0.75
    assert L("filteredLinear3", 0.5, None, 0.0, 1.0, g(0.25), g(0.25), d) == 0.875
    # max(sqr(dN + dP), SMALL) takes SMALL: dP = -dN; (dN - df)*(dP - df) = (0.5 - 1)*(-0.5 - 1) = 0.75 -> 1 - 0.75/1e-15 -> clamps to 0
    assert L("filteredLinear3", 1.0, None, 0.0, 1.0, g(-0.25), g(0.25), d) == 0.0
    # ... and with df on the far side of both the product is negative: 1 + x/SMALL -> 1
    assert L("filteredLinear3", 1.0, None, 0.0, 0.0, g(-0.25), g(0.25), d) == 1.0
    # filteredLinear: the 0.8 floor (flat cells, a jump across the face) and 1 (the face difference equals a cell's)
    assert L("filteredLinear", None, None, 0.0, 1.0, z, z, d) == 0.8
    assert L("filteredLinear", None, None, 0.0, 1.0, g(1.0), g(0.5), d) == 1.0
    assert L("filteredLinear", None, None, 0.0, 1.0, g(0.5), g(0.5), d) == 1.0               # 2 - 0.5*0.5/(0.5 + SMALL) = 1.5 -> 1
    assert L("filteredLinear", None, None, 0.0, 1.0, g(0.25), g(0.25), d) == 0.8             # 2 - 0.375/0.25 = 0.5 -> the floor
    between = L("filteredLinear", None, None, 0.0, 1.0, g(0.3125), g(0.3125), d)             # 2 - 0.34375/0.3125 = 0.9: between the two
    assert between == 2 - 0.34375 / (0.3125 + 1e-15) and 0.8 < between < 1.0
    # the V form projects on dfV: dfV = (1, 0, 0), only component 0's gradient counts
    gv = g(0.25) + g(9.0) + g(-9.0)
    assert L("filteredLinear3V", 1.0, None, [0.0] * 3, [1.0, 0.0, 0.0], gv, gv, d) == 0.75
    # max(-0.0, 0) is +0.0, so a limiter clamped from -0.0 is +0.0
    assert bits(np.array([fs.vmax(np.array([-0.0]), 0.0)[0], tl.rmax(-0.0, 0)]))[0] == 0


def test_the_two_restatements_agree_and_reach_every_branch(pkg):
    """the numpy restatement against the scalar-by-scalar one on every face of the box and the graph with the seeds the gpu tests use;
    and those inputs alone reach every branch the semantics test names"""
    for name in ("box", "graph"):
        hit = fs.HitCount()
        case, Cc, (flux, cdw, phi, grad), ref = _restate_all(pkg, name, 300, hit)
        for key in fs.BRANCHES:
            assert hit.n.get(key, 0) > 0, (name, key, hit.n)
        lo, up = case.lower_addr, case.upper_addr
        for s, sname, kind, vec, k, l in fs.schemes():
            if (k, l) not in ((None, None), (0.33, None), (0.33, 0.5), (1.0, 1.0)):
                continue
            w, lim = ref[s]
            for f in range(0, case.n_faces, 3):
                P, N = int(lo[f]), int(up[f])
                d = [Cc[j][N] - Cc[j][P] for j in range(3)]
                pP, pN = [p[P] for p in phi], [p[N] for p in phi]
                gP, gN = [g[P] for g in grad], [g[N] for g in grad]
                x = fs.limiter_face(sname, k, l, pP if vec else pP[0], pN if vec else pN[0], gP, gN, d)
                assert bits(np.array([x]))[0] == bits(lim[f:f + 1])[0], (s, f)
                assert tl.weight(x, float(cdw[f]), float(flux[f])) == w[f], (s, f)


def test_mirror_exposes_the_filtered_schemes(pkg, tmp_path):
    """foam/miFoam: filteredScheme::New parses through mi_filtered_parse (no GPU) and refuses what it refuses"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    src = tmp_path / "flt.C"
    src.write_text('#include "miFoam.H"\n#include <cstdio>\nusing namespace Foam;\nint main(int argc, char** argv)\n{\n'
                   '    for (int i = 1; i < argc; ++i) { const filteredScheme s = filteredScheme::New(argv[i]);\n'
                   '        std::printf("%d %d %.17g %.17g\\n", s.data().kind, (int)s.vectorForm(), s.data().k, s.data().l); }\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "flt"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "foam"), "-I", os.path.join(os.path.dirname(PKG), "include"), str(src), "-o", str(exe),
                    "-L" + PKG, "-lmiFoam", "-lrapidcfd_amd", "-Wl,-rpath," + PKG], check=True, capture_output=True)
    names = ["filteredLinear", "filteredLinear2 1 0", "filteredLinear2V 0.25 0.5", "filteredLinear3 0.33", "filteredLinear3V 1"]
    out = subprocess.run([str(exe), *names], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [tuple(float(x) for x in line.split()) for line in out.stdout.split("\n") if line]
    assert got == [(0, 0, 0, 0), (1, 0, 1, 0), (1, 1, 0.25, 0.5), (2, 0, 0.33, 0), (2, 1, 1, 0)]
    for s, why in (("filteredLinearV", "unknown filtered scheme"), ("vanLeer", "unknown filtered scheme"), ("filteredLinear2 1", "takes 2"),
                   ("filteredLinear3 2", "k should be"), ("filteredLinear3 x", "not a number")):
        bad = subprocess.run([str(exe), s], capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and why in (bad.stdout + bad.stderr), s
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    assert syms.count("Foam::filteredWeights(") == 2 and syms.count("Foam::patchFilteredWeights(") == 2


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _device_case(pkg, name, seed=300):
    hit = fs.HitCount()
    case, Cc, (flux, cdw, phi, grad), ref = _restate_all(pkg, name, seed, hit)
    for key in fs.BRANCHES:
        assert hit.n.get(key, 0) > 0, (key, hit.n)
    return case, Cc, flux, cdw, phi, grad, ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "graph", "box_noxcd"])
def test_every_scheme_against_the_restatement(pkg, monkeypatch, name):
    if name.endswith("_noxcd"):   # the plain blockIdx.x mapping of k_limited_weights
        set_row_tables(monkeypatch, "noxcd"); name = name[:-len("_noxcd")]
    eng, ctx, dev, host, E = gpu_env(pkg)
    case, Cc, flux, cdw, phi, grad, ref = _device_case(pkg, name)
    nf = case.n_faces
    A = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
    fd, wd, pd_, gd, Cd = dev(flux), dev(cdw), [dev(x) for x in phi], [dev(x) for x in grad], [dev(x) for x in Cc]
    for s, _, kind, vec, k, l in fs.schemes():
        rw, rl = ref[s]
        w, lo_, w2 = E(nf), E(nf), E(nf)
        A.filtered_weights(eng.filtered(s), wd, fd, pd_[:3] if vec else pd_[:1], gd if vec else gd[:3], Cd, w, lo_)
        assert same(host(lo_), rl), s
        assert same(host(w), rw), s
        A.filtered_weights(s, wd, fd, pd_[:3] if vec else pd_[:1], gd if vec else gd[:3], Cd, w2)   # no limiter output: the same weights
        assert same(host(w2), rw), s


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 3])
def test_the_loop_walk_under_a_forced_grid(pkg, monkeypatch, grid):
    """MI_FACE_GRID 1: one workgroup walks all 1 321 faces; 3: chunks of 512, the last one partial"""
    set_face_grid(monkeypatch, grid)
    eng, ctx, dev, host, E = gpu_env(pkg)
    case, Cc, flux, cdw, phi, grad, ref = _device_case(pkg, "box")
    nf = case.n_faces
    assert nf == 1321 and nf > grid * 256
    A = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
    fd, wd, pd_, gd, Cd = dev(flux), dev(cdw), [dev(x) for x in phi], [dev(x) for x in grad], [dev(x) for x in Cc]
    for s, vec in (("filteredLinear2 0.33 0.5", False), ("filteredLinear3V 0.33", True)):
        w, lo_ = E(nf), E(nf)
        A.filtered_weights(s, wd, fd, pd_[:3] if vec else pd_[:1], gd if vec else gd[:3], Cd, w, lo_)
        assert same(host(lo_), ref[s][1]) and same(host(w), ref[s][0]), s


@pytest.mark.gpu
def test_cyclic_patch_against_the_restatement(pkg):
    """LimitedScheme.C:145-195 on the 12x7x6 cyclic channel (x-min <-> x-max): phiN and gradcN from mi_matrix_patch_neighbour_field"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    dims = (12, 7, 6)
    case = syn.box_case(*dims)
    n = case.n_cells
    flux, cdw, phi, grad = _inputs(pkg, case, 400)
    cyc = syn.add_cyclic_x(case)
    fcs = [i.face_cells for i in cyc.interfaces]
    nbrs = [cyc.interfaces[i.nbr_patch].face_cells for i in cyc.interfaces]
    mat = eng.Matrix(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr, fcs, nbrs))
    npf = [len(f) for f in fcs]
    off = [0, npf[0]]
    pdv, gd = [dev(x) for x in phi], [dev(x) for x in grad]
    nbr_phi, nbr_grad = [E(sum(npf)) for _ in range(3)], [E(sum(npf)) for _ in range(9)]
    for j in range(3):
        mat.patch_neighbour_field(pdv[j], nbr_phi[j])
    for c in range(9):
        mat.patch_neighbour_field(gd[c], nbr_grad[c])
    nph, ngh = [host(x) for x in nbr_phi], [host(x) for x in nbr_grad]
    assert same(nph[0], np.concatenate([phi[0][q] for q in nbrs]))
    h = 1.0 / dims[0]
    hit = fs.HitCount()
    for p in range(2):
        P = eng.Patch(ctx, n, fcs[p])
        m = npf[p]
        pflux = u(500 + p, m) - 0.45
        pflux[::5] = 0.0
        pcdw = 0.3 + 0.4 * u(510 + p, m)
        pdelta = [np.full(m, -h if p == 0 else h), 0.01 * (u(520 + p, m) - 0.5), np.zeros(m)]
        sl = lambda a: a[off[p]:off[p] + m]
        D = fs.patch_differences(fcs[p], phi, [sl(x) for x in nph], grad, [sl(x) for x in ngh], pdelta)
        for s, _, kind, vec, k, l in fs.schemes():
            nc = 3 if vec else 1
            w, lo_ = E(m), E(m)
            P.filtered_weights(s, dev(pcdw), dev(pflux), pdv[:nc], [sl(x).contiguous() for x in nbr_phi[:nc]], gd[:3 * nc],
                               [sl(x).contiguous() for x in nbr_grad[:3 * nc]], [dev(x) for x in pdelta], w, lo_)
            rw, rl = D.weights(kind, vec, k, l, pcdw, pflux, hit)
            assert same(host(lo_), rl), (p, s)
            assert same(host(w), rw), (p, s)
        P.close()
    for key in ("zero_flux", "fl2_df_pos", "fl2_df_nonpos", "fl_floor", "fl_one", "fl3_clamp_0"):
        assert hit.n.get(key, 0) > 0, (key, hit.n)


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg, fill=7.0)
    case = pkg.synthetic.box_case(6, 5, 4)
    n, nf = case.n_cells, case.n_faces
    flux, cdw, phi, grad = tl._fields(pkg, n, nf, 800)
    A = eng.Assembly(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr))
    fd, wd, pd_, gd, Cd = dev(flux), dev(cdw), [dev(x) for x in phi], [dev(x) for x in grad], [dev(np.arange(n, dtype=float) * 0.1) for _ in range(3)]
    w, l = E(nf), E(nf)
    call = lambda lim="filteredLinear3 1", **kw: A.filtered_weights(lim, kw.get("cdw", wd), kw.get("flux", fd), kw.get("phi", pd_[:1]), kw.get("grad", gd[:3]),
                                                                    kw.get("C", Cd), kw.get("w", w), kw.get("l", l))
    F = eng.FilteredLimiter
    for bad in (F(3, 0, 0.5, 0.0), F(-1, 0, 0.5, 0.0), F(12, 0, 0.5, 0.0), F(1, 2, 0.5, 0.0), F(0, 1, 0.0, 0.0)):   # kind, vector_form, filteredLinearV
        with pytest.raises(eng.MiError, match="invalid mi_filtered_limiter"):
            call(bad)
    with pytest.raises(eng.MiError, match="k should be"):
        call(F(2, 0, 1.5, 0.0))
    with pytest.raises(eng.MiError, match="k should be"):
        call(F(1, 0, float("nan"), 0.0))
    with pytest.raises(eng.MiError, match="l should be"):
        call(F(1, 0, 0.5, -0.25))
    with pytest.raises(eng.MiError, match="missing"):
        call(grad=[gd[0], None, gd[2]])
    with pytest.raises(eng.MiError, match="missing"):
        call("filteredLinear3V 1", phi=pd_[:1] + [None, None], grad=gd)
    with pytest.raises(eng.MiError, match="missing"):
        call(w=None)
    with pytest.raises(eng.MiError, match="aligned"):
        call(flux=E(nf + 1)[1:])
    with pytest.raises(eng.MiError, match="alias"):
        call(w=fd)
    with pytest.raises(eng.MiError, match="alias"):
        call(l=gd[1])
    with pytest.raises(eng.MiError, match="differ"):
        call(w=w, l=w)
    lim12 = eng.limiter("vanLeer"); lim12.kind = 12                     # the filtered kinds are no mi_limiter kinds
    with pytest.raises(eng.MiError, match="invalid mi_limiter"):
        A.limited_weights(lim12, wd, fd, pd_[:1], gd[:3], Cd, w, l)
    P = eng.Patch(ctx, n, np.arange(5, dtype=np.int32))
    m5, l5 = E(5), E(5)
    ones, zeros = dev(np.ones(5)), dev(np.zeros(5))
    pargs = lambda out, lo_: (dev(np.ones(5)), ones, pd_[:1], [zeros], gd[:3], [dev(np.zeros(5)) for _ in range(3)], [dev(np.ones(5)) for _ in range(3)], out, lo_)
    with pytest.raises(eng.MiError, match="alias"):
        P.filtered_weights("filteredLinear", *pargs(ones, l5))
    with pytest.raises(eng.MiError, match="invalid mi_filtered_limiter"):
        P.filtered_weights(F(3, 0, 0.5, 0.0), *pargs(m5, l5))
    with pytest.raises(eng.MiError, match="l should be"):
        P.filtered_weights(F(1, 1, 0.5, 2.0), *pargs(m5, l5))
    P.close()
    torch.cuda.synchronize()
    for t in (w, l, m5, l5):
        assert torch.all(t == 7.0)                                      # nothing was launched
    assert torch.all(ones == 1.0)
    call()                                                              # and the same call with a valid struct writes
    torch.cuda.synchronize()
    assert torch.all(w != 7.0) and torch.all(l != 7.0)
