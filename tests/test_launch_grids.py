"""The launch grids of the face passes and of the unique-cell patch passes of csrc/assembly.inc.

Every one of them is launched with grid_for(ctx, n) workgroups of 256 threads: one thread per item up to a cap (MI_FACE_GRID, 8192), so
that past 8192*256 = 2 097 152 items the kernel's own loop does the rest -- a grid-stride loop, or block_chunk's contiguous chunk per block
(permuted by xcd_block when the context maps blocks XCD-aware).  At the sizes the other test files use no such loop takes a second trip
and no block_chunk block is idle or partial in the middle, so here

  * (CPU) the arithmetic is restated in Python and the chunks of all blocks are shown to partition [0, n) exactly once;
  * (gpu) every entry that launches through grid_for runs on small meshes with the cap forced to 1, 3, 8 and 11 workgroups -- one block
    walks everything; fewer than 8: xcd_block is the identity; one block per XCD and no tail; 8 permuted blocks and 3 tail blocks --
    with and without the XCD-aware mapping, against the reference its own test file uses and against the default grid, bit for bit;
  * (gpu) the passes that no other test runs past the shipped cap run past it once, at their natural grid: five face passes on the
    129x127x44 box (2 134 909 faces = 8192*256 + 37 757), mi_fvm_set_values and the three patch kernels on the 130^3 box.

mi_fvm_set_values used to drop every label past the cap (k_set_values_cells had no loop): test_set_values_past_the_cap and the
set_values cases of test_entry_under_a_forced_grid fail without that loop."""
import os
import re

import numpy as np
import pytest

from assembly_support import gpu_env, same, set_face_grid, set_row_tables, shape_case, signed_flux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 8192                      # switches.hpp: MI_FACE_GRID
GRIDS = (1, 3, 8, 11)
NAN = float("nan")


# ---- the arithmetic, restated ------------------------------------------------------------------------------------------------------------
def grid_for(n, cap=CAP):
    """assembly.inc, grid_for(ctx, n): b = (n + 255)/256; b < 1 ? 1 : (b > cap ? cap : b), cap = the context's faceGrid, which
    mi_ctx_create raises to 1 when the switch says less"""
    cap = max(int(cap), 1)
    b = (n + 255) // 256
    return 1 if b < 1 else min(b, cap)


def xcd_block(b, G):
    """assembly.inc:25-29, xcd_block(): per = gridDim.x >> 3; the first 8*per blocks are dealt round-robin to 8 runs of `per` chunks
    (hardware places block b on XCD b % 8), the tail keeps its index"""
    b = np.asarray(b, dtype=np.int64)
    per = G >> 3
    return np.where(b < (per << 3), (b & 7) * per + (b >> 3), b)


def block_chunk(n, G, b, xcd):
    """assembly.inc:32-38, block_chunk(n, xcd, i0, i1) of block b of G: chunk = ((ceil(n/G) + 255) & ~255) items,
    i0 = min(lb*chunk, n), i1 = min(i0 + chunk, n) -- a block past the end gets the empty range [n, n)"""
    lb = xcd_block(b, G) if xcd else np.asarray(b, dtype=np.int64)
    chunk = (((n + G - 1) // G) + 255) & ~255
    i0 = np.minimum(lb * chunk, n)
    i1 = np.minimum(i0 + chunk, n)
    return i0, i1


def test_the_default_cap_is_the_one_restated_here():
    text = open(os.path.join(ROOT, "rapidcfd-dev_amd", "csrc", "switches.hpp")).read()
    assert int(re.search(r'X\(FACE_GRID,\s*"MI_FACE_GRID",\s*(-?\d+),\s*CTX,\s*DIAG', text).group(1)) == CAP
    for n in (0, 1, 255, 256, 257, 3502, CAP * 256 - 1, CAP * 256, CAP * 256 + 1, 2134909, 2**31 - 256):
        was = max(1, min((n + 255) // 256, 8192))                        # grid_for(n) before the cap became a switch
        assert grid_for(n) == was, n
    assert [grid_for(3502, g) for g in (-5, 0, 1, 3, 8, 11, 14, 15)] == [1, 1, 1, 3, 8, 11, 14, 14]


@pytest.mark.parametrize("G", [1, 3, 7, 8, 9, 11, 15, 16, 8191, 8192])
def test_block_chunks_partition_the_items(G):
    """every item of [0, n) lies in the chunk of exactly one block of a grid of G, with and without the XCD permutation -- also when the
    grid has more blocks than chunks (idle blocks) and when the last busy chunk is partial; xcd_block is a bijection of [0, G)"""
    b = np.arange(G)
    assert np.array_equal(np.sort(xcd_block(b, G)), b)
    if G < 8:
        assert np.array_equal(xcd_block(b, G), b)
    for n in (1, 255, 256, 257, 3502, G * 256 - 1, G * 256, G * 256 + 1, 2134909):
        for xcd in (False, True):
            i0, i1 = block_chunk(n, G, b, xcd)
            assert np.all((0 <= i0) & (i0 <= i1) & (i1 <= n)), (n, xcd)
            cover = np.zeros(n + 1, np.int64)
            np.add.at(cover, i0, 1)
            np.add.at(cover, i1, -1)
            assert np.all(np.cumsum(cover)[:n] == 1), (n, xcd)
            assert i1[i1 > i0].max() == n and np.all((i1 - i0)[i1 < n] % 256 == 0), (n, xcd)      # only the last busy chunk is partial


def test_the_shapes_the_gpu_tests_rest_on():
    # the 13x11x9 box, cap 11: chunks of 512, 7 busy blocks (the last one partial: 430 faces) and 4 idle ones
    nf = 3 * 13 * 11 * 9 - 13 * 11 - 13 * 9 - 11 * 9
    assert nf == 3502 and grid_for(nf, 11) == 11
    i0, i1 = block_chunk(nf, 11, np.arange(11), True)
    assert sorted((i1 - i0).tolist()) == [0] * 4 + [430] + [512] * 6
    assert [grid_for(nf, g) * 256 < nf for g in GRIDS] == [True] * 4      # every grid-stride loop strides
    # the 129x127x44 box: past the shipped cap; a second, partial trip of the grid-stride loops; chunks of 512, about half the blocks idle
    nf = 3 * 129 * 127 * 44 - 129 * 127 - 129 * 44 - 127 * 44
    assert nf == 2134909 == CAP * 256 + 37757 and nf % 256 == 125 and grid_for(nf) == CAP
    i0, i1 = block_chunk(nf, CAP, np.arange(CAP), True)
    assert int(np.max(i1 - i0)) == 512 and int(np.sum(i1 > i0)) == 4170 and int(np.sum(i1 == i0)) == 4022


# ---- small meshes under forced grids ----------------------------------------------------------------------------------------------------
class Env:
    """one context under a forced cap (None: the default) and one block mapping, outputs prefilled with NaN"""

    def __init__(self, pkg, monkeypatch, grid, tables="default"):
        set_row_tables(monkeypatch, tables)
        set_face_grid(monkeypatch, grid)
        self.eng, self.ctx, self.dev, self.host, self.N = gpu_env(pkg, fill=NAN)

    def assembly(self, q):
        return self.eng.Assembly(self.eng.Addressing(self.ctx, q["n"], q["lo"], q["up"]))

    def devs(self, arrays):
        return [self.dev(x) for x in arrays]

    def hosts(self, tag, tensors):
        return {f"{tag}{j}": self.host(t) for j, t in enumerate(tensors)}


def _ldu(pkg, mesh):
    """the 13x11x9 box (3 502 faces), asymmetric; the random graph of tests/assembly_support.py (9 000 cells, about 27 000 faces)"""
    case = pkg.synthetic.box_case(13, 11, 9, symmetric=False) if mesh == "box" else shape_case(pkg, "graph", symmetric=False)
    return dict(n=case.n_cells, nf=case.n_faces, lo=case.lower_addr, up=case.upper_addr, case=case)


def _geometry(pkg, mesh):
    """what tests/test_assembly.py skewed_mesh gives -- the distorted 13x11x9 box -- or the random graph with seeded `geometry` of the same
    ranges (the references read arrays only)"""
    if mesh == "box":
        from test_assembly import skewed_mesh
        M = skewed_mesh((13, 11, 9))
        assert M["nI"] == 3502
        return M
    u = pkg.synthetic.splitmix_uniform
    q = _ldu(pkg, "graph")
    n, nf = q["n"], q["nf"]
    G = dict(weights=0.2 + 0.6 * u(70, nf), delta=1.0 + u(71, nf), Sf=np.stack([u(72 + k, nf) - 0.5 for k in range(3)], axis=1), magSf=0.5 + u(75, nf),
             V=0.5 + u(76, n))
    return dict(n=n, nI=nf, lo=q["lo"], up=q["up"], G=G, corr=[0.3 * (u(77 + k, nf) - 0.5) for k in range(3)])


def _named(tag, arrays):
    return {f"{tag}{j}": a for j, a in enumerate(arrays)}


# -- fvc::interpolate, fvc::div, the flux and ddtCorr passes: the oracle, as tests/test_assembly.py and assembly_support.row_passes_bit_exact
def prep_rows(pkg, orc, mesh):
    u = pkg.synthetic.splitmix_uniform
    q = _ldu(pkg, mesh)
    n, nf = q["n"], q["nf"]
    q.update(w=u(9, nf), phi=u(10, nf) - 0.5, vol=0.5 + u(11, n), cellf=u(12, n), lam=u(30, nf), Sf=[u(20 + k, nf) - 0.5 for k in range(3)],
             V=[u(31 + k, n) - 0.5 for k in range(3)], rho=0.8 + u(35, n), aA=u(36, nf) - 0.5, aB=u(37, nf), phi0=u(18, nf) - 0.5, rdt=1.0 / 3e-4)
    return q


def prep_face_interpolate(pkg, orc, mesh):
    q = prep_rows(pkg, orc, mesh)
    q["ref"] = dict(sf=orc.face_interpolate(q["lo"], q["up"], q["w"], q["cellf"]))
    return q


def run_face_interpolate(env, q):
    sf = env.N(q["nf"])
    env.assembly(q).face_interpolate(env.dev(q["w"]), env.dev(q["cellf"]), sf)
    return dict(sf=env.host(sf))


def prep_fvc_div(given):
    def prep(pkg, orc, mesh):
        q = prep_rows(pkg, orc, mesh)
        n, lo, up = q["n"], q["lo"], q["up"]
        face = q["phi"] * orc.face_interpolate(lo, up, q["w"] if given else orc.upwind_weights(q["phi"]), q["cellf"])
        q["ref"] = dict(face=face, div=orc.surface_integrate(n, lo, up, face, q["vol"]))
        return q
    return prep


def run_fvc_div(given):
    def run(env, q):
        face, div = env.N(q["nf"]), env.N(q["n"])
        env.assembly(q).fvc_div(env.dev(q["phi"]), env.dev(q["w"]) if given else None, env.dev(q["cellf"]), env.dev(q["vol"]), face, div)
        return dict(face=env.host(face), div=env.host(div))
    return run


def prep_flux_div(pkg, orc, mesh):
    q = prep_rows(pkg, orc, mesh)
    phi, div = orc.flux_div(q["n"], q["lo"], q["up"], q["lam"], q["Sf"], q["V"], scale=q["rho"], add_a=q["aA"], add_b=q["aB"], vol=q["vol"])
    q["ref"] = dict(phi=phi, div=div)
    return q


def run_flux_div(env, q):
    phi, div = env.N(q["nf"]), env.N(q["n"])
    env.assembly(q).flux_div(env.dev(q["lam"]), env.devs(q["Sf"]), env.devs(q["V"]), phi, div, cell_scale=env.dev(q["rho"]), add_a=env.dev(q["aA"]),
                             add_b=env.dev(q["aB"]), vol=env.dev(q["vol"]))
    return dict(phi=env.host(phi), div=env.host(div))


def prep_ddt_phi_corr(pkg, orc, mesh):
    q = prep_rows(pkg, orc, mesh)
    q["ref"] = {tag: orc.ddt_phi_corr(q["lo"], q["up"], q["rdt"], q["lam"], q["Sf"], q["V"], r0, q["phi0"]) for tag, r0 in (("rho", q["rho"]), ("plain", None))}
    return q


def run_ddt_phi_corr(env, q):
    A, got = env.assembly(q), {}
    for tag in ("rho", "plain"):
        out = env.N(q["nf"])
        A.ddt_phi_corr(q["rdt"], env.dev(q["lam"]), env.devs(q["Sf"]), env.devs(q["V"]), env.dev(q["rho"]) if tag == "rho" else None, env.dev(q["phi0"]), out)
        got[tag] = env.host(out)
    return got


# -- ddtCorr of the backward and of the local schemes: the restatements of tests/test_backward_ddt.py and tests/test_local_ddt.py
def _ddt_corr_inputs(pkg, orc, q, density):
    """the fields of test_ddt_corr_against_the_restatement: phi0 near flux(U0), exact zeros (coefficient 0), exact equality (coefficient 1)"""
    u = pkg.synthetic.splitmix_uniform
    n, nf, lo, up = q["n"], q["nf"], q["lo"], q["up"]
    d = dict(lam=0.001 + 0.998 * u(9, nf), Sf=[u(10 + k, nf) - 0.5 for k in range(3)], U0=[u(13 + k, n) - 0.5 for k in range(3)],
             U00=[u(16 + k, n) - 0.5 for k in range(3)], rho0=0.8 + u(20, n) if density else None, rho00=0.7 + u(21, n) if density else None,
             phi00=u(23, nf) - 0.5, r=50.0 + 400.0 * u(4, n))
    fU = orc.flux_div(n, lo, up, d["lam"], d["Sf"], d["U0"] if not density else [d["rho0"] * x for x in d["U0"]], want_div=False)
    phi0 = fU + 0.05 * (u(22, nf) - 0.5)
    phi0[::5] = 0.0
    phi0[2::7] = fU[2::7]
    d["phi0"] = phi0
    return d


def prep_ddt_backward(pkg, orc, mesh):
    from test_backward_ddt import coeffs, ddt_corr
    q = _ldu(pkg, mesh)
    q["c"], q["rdt"], q["ref"] = coeffs(0.004, 0.01), 1.0 / 0.004, {}
    for tag in ("plain", "rho"):
        d = q[tag] = _ddt_corr_inputs(pkg, orc, q, tag == "rho")
        ref, k, _ = ddt_corr(orc, q["n"], q["lo"], q["up"], q["rdt"], q["c"], d["lam"], d["Sf"], d["U0"], d["U00"], d["rho0"], d["rho00"], d["phi0"], d["phi00"])
        assert np.any(k == 0.0) and np.any(k == 1.0) and np.any((k > 0.05) & (k < 0.95))
        q["ref"][tag] = ref
    return q


def run_ddt_backward(env, q):
    A, got = env.assembly(q), {}
    for tag in ("plain", "rho"):
        d, out = q[tag], env.N(q["nf"])
        A.ddt_phi_corr_backward(q["rdt"], q["c"], env.dev(d["lam"]), env.devs(d["Sf"]), env.devs(d["U0"]), env.devs(d["U00"]),
                                None if d["rho0"] is None else env.dev(d["rho0"]), None if d["rho00"] is None else env.dev(d["rho00"]),
                                env.dev(d["phi0"]), env.dev(d["phi00"]), out)
        got[tag] = env.host(out)
    return got


def prep_ddt_local(pkg, orc, mesh):
    from test_local_ddt import ddt_corr
    q = _ldu(pkg, mesh)
    d = q["d"] = _ddt_corr_inputs(pkg, orc, q, False)
    ref, k = ddt_corr(orc, q["n"], q["lo"], q["up"], d["r"], d["lam"], d["Sf"], d["U0"], d["phi0"])
    assert np.any(k == 0.0) and np.any(k == 1.0) and np.any((k > 0.05) & (k < 0.95))
    q["ref"] = dict(out=ref)
    return q


def run_ddt_local(env, q):
    d, out = q["d"], env.N(q["nf"])
    env.assembly(q).ddt_phi_corr_local(env.dev(d["r"]), env.dev(d["lam"]), env.devs(d["Sf"]), env.devs(d["U0"]), env.dev(d["phi0"]), out)
    return dict(out=env.host(out))


# -- the non-orthogonal corrections and dev(T(grad)): the oracle and the restatements of tests/test_limited_sngrad.py, test_div_dev_tgrad.py
def prep_sngrad(pkg, orc, mesh):
    u = pkg.synthetic.splitmix_uniform
    M = _geometry(pkg, mesh)
    n, nI = M["n"], M["nI"]
    q = dict(n=n, nf=nI, lo=M["lo"], up=M["up"], M=M, g=[(u(12, n, start=k * n) - 0.5) * 128 for k in range(3)], gms=M["G"]["magSf"][:nI] * (1.0 + 0.3 * u(4, nI)))
    q["ref"] = dict(flux=orc.sngrad_correction_flux(M["lo"], M["up"], M["corr"], M["G"]["weights"], q["g"], q["gms"]))
    return q


def run_sngrad(env, q):
    M, flux = q["M"], env.N(q["nf"])
    env.assembly(q).sngrad_correction_flux(env.devs(M["corr"]), env.dev(M["G"]["weights"]), env.devs(q["g"]), env.dev(q["gms"]), flux)
    return dict(flux=env.host(flux))


def prep_sngrad_limited(n_comp, k=0.33):
    def prep(pkg, orc, mesh):
        from test_limited_sngrad import limited_flux
        u = pkg.synthetic.splitmix_uniform
        M = _geometry(pkg, mesh)
        n, nI, G = M["n"], M["nI"], M["G"]
        q = dict(n=n, nf=nI, lo=M["lo"], up=M["up"], M=M, k=k, vf=[u(11, n, start=j * n) - 0.5 for j in range(n_comp)],
                 g=[(u(12, n, start=i * n) - 0.5) * 128 for i in range(3 * n_comp)], gms=G["magSf"][:nI] * (1.0 + 0.3 * u(4, nI)))
        out, lim = limited_flux(orc, M["lo"], M["up"], k, M["corr"], G["weights"], G["delta"], q["vf"], q["g"], q["gms"])
        assert np.any(lim < 1.0) and np.any(lim == 1.0)                     # both branches of the min
        q["ref"] = dict(_named("flux", out), limiter=lim)
        return q
    return prep


def run_sngrad_limited(env, q):
    M, G = q["M"], q["M"]["G"]
    out, lim = [env.N(q["nf"]) for _ in q["vf"]], env.N(q["nf"])
    env.assembly(q).sngrad_limited_correction_flux(q["k"], env.devs(M["corr"]), env.dev(G["weights"]), env.dev(G["delta"]), env.devs(q["vf"]), env.devs(q["g"]),
                                                   env.dev(q["gms"]), out, lim)
    return dict(env.hosts("flux", out), limiter=env.host(lim))


def prep_dev_tgrad(kind):
    def prep(pkg, orc, mesh):
        from test_div_dev_tgrad import internal
        u = pkg.synthetic.splitmix_uniform
        M = _geometry(pkg, mesh)
        n = M["n"]
        q = dict(n=n, nf=M["nI"], lo=M["lo"], up=M["up"], M=M, kind=kind, g=[(u(21, n, start=i * n) - 0.5) * 128 for i in range(9)], visc=0.5 + u(22, n))
        face, div = internal(orc, M, kind, q["visc"], q["g"], M["G"]["V"])
        q["ref"] = dict(_named("face", face), **_named("div", div))
        return q
    return prep


def run_dev_tgrad(env, q):
    G, nI = q["M"]["G"], q["nf"]
    face, div = [env.N(nI) for _ in range(3)], [env.N(q["n"]) for _ in range(3)]
    env.assembly(q).div_dev_tgrad(q["kind"], env.dev(G["weights"]), [env.dev(G["Sf"][:nI, k]) for k in range(3)], env.dev(q["visc"]), env.devs(q["g"]), face, div,
                                  env.dev(G["V"]))
    return dict(env.hosts("face", face), **env.hosts("div", div))


# -- the limited schemes and linearUpwind: the oracle and the restatements of tests/test_limited_schemes.py, tests/test_linear_upwind.py
def _limited_mesh(pkg, mesh):
    from conftest import random_graph_case
    from test_limited_schemes import _fields, _graded_box
    if mesh == "box":
        case, Cc = _graded_box(pkg, (13, 11, 9))
    else:
        case = random_graph_case(pkg, 600, extra=3.0, seed=13)
        Cc = [pkg.synthetic.splitmix_uniform(90 + k, case.n_cells) for k in range(3)]
    q = dict(n=case.n_cells, nf=case.n_faces, lo=case.lower_addr, up=case.upper_addr, Cc=Cc)
    q["flux"], q["cdw"], q["phi"], q["grad"] = _fields(pkg, q["n"], q["nf"], 300)
    return q


def prep_limited_linear(pkg, orc, mesh):
    q = _limited_mesh(pkg, mesh)
    w, lim = orc.limited_linear_weights(q["lo"], q["up"], 0.33, q["cdw"], q["flux"], q["phi"][0], q["grad"][:3], q["Cc"])
    q["ref"] = dict(w=w, limiter=lim)
    return q


def run_limited_linear(env, q):
    w, lim = env.N(q["nf"]), env.N(q["nf"])
    env.assembly(q).limited_linear_weights(0.33, env.dev(q["cdw"]), env.dev(q["flux"]), env.dev(q["phi"][0]), env.devs(q["grad"][:3]), env.devs(q["Cc"]), w, lim)
    return dict(w=env.host(w), limiter=env.host(lim))


def prep_limited(scheme, kind, vec, bounds, k):
    def prep(pkg, orc, mesh):
        from test_limited_schemes import restate_internal
        q = _limited_mesh(pkg, mesh)
        q.update(scheme=scheme, phi=q["phi"][:3] if vec else q["phi"][:1], grad=q["grad"] if vec else q["grad"][:3])
        w, lim = restate_internal(kind, vec, bounds, k, q["lo"], q["up"], q["cdw"], q["flux"], q["phi"], q["grad"], q["Cc"])
        q["ref"] = dict(w=w, limiter=lim)
        return q
    return prep


def run_limited(env, q):
    w, lim = env.N(q["nf"]), env.N(q["nf"])
    env.assembly(q).limited_weights(env.eng.limiter(q["scheme"]), env.dev(q["cdw"]), env.dev(q["flux"]), env.devs(q["phi"]), env.devs(q["grad"]), env.devs(q["Cc"]), w, lim)
    return dict(w=env.host(w), limiter=env.host(lim))


def prep_linear_upwind(n_rhs, scale):
    def prep(pkg, orc, mesh):
        from test_linear_upwind import _grads, _mesh, restate_internal
        n, lo, up, C, cf = _mesh(pkg, mesh)
        nf = lo.shape[0]
        q = dict(n=n, nf=nf, lo=lo, up=up, C=C, cf=cf, scale=scale, flux=signed_flux(pkg.synthetic.splitmix_uniform(7, nf)), g=_grads(pkg, n, n_rhs, 60 + n_rhs))
        q["ref"] = _named("t", restate_internal(lo, up, q["flux"], cf, C, q["g"], scale))
        return q
    return prep


def run_linear_upwind(env, q):
    out = [env.N(q["nf"]) for _ in q["g"]]
    env.assembly(q).linear_upwind_correction(env.dev(q["flux"]), env.devs(q["cf"]), env.devs(q["C"]), [env.devs(gr) for gr in q["g"]], out, scale=q["scale"])
    return env.hosts("t", out)


# -- fvMatrix::setValues: the oracle.  A third of the cells is set so that the label kernel strides under every forced grid -- that needs
#    more than 11*256 labels, so the meshes are the larger two of assembly_support.shape_case (13 547 and 9 000 cells), not the 13x11x9 box
def prep_set_values(upstream):
    def prep(pkg, orc, mesh):
        u = pkg.synthetic.splitmix_uniform
        case = shape_case(pkg, mesh, symmetric=False)
        n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
        n_set, m = n // 3, 500
        assert n_set > GRIDS[-1] * 256
        q = dict(n=n, nf=nf, lo=lo, up=up, case=case, upstream=upstream, cells=np.argsort(u(81, n), kind="stable")[:n_set].astype(np.int32), vals=u(82, n_set) - 0.5,
                 psi=u(83, n), fc=(u(84, m) * n).astype(np.int32), ic=u(85, m) - 0.5, bc=u(86, m) - 0.5)
        sv = orc.set_values(n, lo, up, q["cells"], q["vals"], q["psi"], case.diag, case.source, case.upper, case.lower, [q["fc"]], [q["ic"]], [q["bc"]], upstream=upstream)
        assert np.any(sv["icoeffs"][0] == 0.0) and np.any(sv["icoeffs"][0] != 0.0)
        q["ref"] = dict(psi=sv["psi"], source=sv["source"], upper=sv["upper"], lower=sv["lower"], ic=sv["icoeffs"][0], bc=sv["bcoeffs"][0])
        return q
    return prep


def run_set_values(env, q):
    import torch
    case, dev = q["case"], env.dev
    psi, src, upper, lower, ic, bc = dev(q["psi"]), dev(case.source), env.N(q["nf"]), env.N(q["nf"]), dev(q["ic"]), dev(q["bc"])
    patch = env.eng.Patch(env.ctx, q["n"], q["fc"])
    env.assembly(q).set_values(torch.from_numpy(q["cells"]).to("cuda:0"), dev(q["vals"]), psi, dev(case.diag), src, dev(case.upper), dev(case.lower), upper, lower,
                               [patch], [ic], [bc], upstream=q["upstream"])
    return dict(psi=env.host(psi), source=env.host(src), upper=env.host(upper), lower=env.host(lower), ic=env.host(ic), bc=env.host(bc))


# -- the unique-cell patch kernels: the oracle (np.maximum.at for the maximum, as tests/test_local_ddt.py co_cells).  3 000 unique cells of the
#    31x23x19 box with 1 to 5 faces each, the faces in a seeded order: 12 blocks at one thread per cell, so that a grid of 11 still strides
def patch_faces(pkg, n, n_unique, seed):
    u = pkg.synthetic.splitmix_uniform
    cells = np.argsort(u(seed, n), kind="stable")[:n_unique]
    fc = np.repeat(cells, 1 + np.arange(n_unique) % 5)
    return fc[np.argsort(u(seed + 1, fc.shape[0]), kind="stable")].astype(np.int32)


def prep_patch(op, fn):
    def prep(pkg, orc, mesh):
        u = pkg.synthetic.splitmix_uniform
        n = 31 * 23 * 19
        fc = patch_faces(pkg, n, 3000, 91)
        m = fc.shape[0]
        assert m == 9000 and np.unique(fc).shape[0] == 3000 > GRIDS[-1] * 256 and np.bincount(np.bincount(fc))[1:].tolist() == [600] * 5
        q = dict(n=n, fc=fc, op=op, fn=fn, pf=u(93, m) - 0.5, q=u(94, m), intf=u(95, n) - 0.5)
        if op == "add":
            ref = orc.patch_add(fc, q["pf"], q["intf"], fn)
        elif op == "add_product":
            ref = orc.patch_add_product(fc, q["pf"], q["q"], q["intf"], fn)
        else:
            ref = q["intf"].copy()
            np.maximum.at(ref, fc, q["pf"])
            assert 0.2 * 3000 < np.sum(ref != q["intf"]) < 3000
        q["ref"] = dict(intf=ref)
        return q
    return prep


def run_patch(env, q):
    patch, intf = env.eng.Patch(env.ctx, q["n"], q["fc"]), env.dev(q["intf"])
    if q["op"] == "add":
        patch.add(env.dev(q["pf"]), intf, q["fn"])
    elif q["op"] == "add_product":
        patch.add_product(env.dev(q["pf"]), env.dev(q["q"]), intf, q["fn"])
    else:
        patch.max(env.dev(q["pf"]), intf)
    return dict(intf=env.host(intf))


# entry -> (meshes, prepare, run, it has an XCD-aware form)
BOTH = ("box", "graph")
ENTRIES = {
    "face_interpolate": (BOTH, prep_face_interpolate, run_face_interpolate, True),
    "fvc_div/weights": (BOTH, prep_fvc_div(True), run_fvc_div(True), True),
    "fvc_div/upwind": (BOTH, prep_fvc_div(False), run_fvc_div(False), True),
    "sngrad_correction_flux": (BOTH, prep_sngrad, run_sngrad, True),
    "sngrad_limited_correction_flux/scalar": (BOTH, prep_sngrad_limited(1), run_sngrad_limited, True),
    "sngrad_limited_correction_flux/vector": (BOTH, prep_sngrad_limited(3), run_sngrad_limited, True),
    "flux_div": (BOTH, prep_flux_div, run_flux_div, True),
    "ddt_phi_corr": (BOTH, prep_ddt_phi_corr, run_ddt_phi_corr, True),
    "ddt_phi_corr_backward": (BOTH, prep_ddt_backward, run_ddt_backward, True),
    "ddt_phi_corr_local": (BOTH, prep_ddt_local, run_ddt_local, True),
    "limited_linear_weights": (BOTH, prep_limited_linear, run_limited_linear, True),
    "limited_weights/vanLeer": (BOTH, prep_limited("vanLeer", "vanLeer", False, None, None), run_limited, True),
    "limited_weights/limitedCubicV": (BOTH, prep_limited("limitedCubicV 0.33", "limitedCubic", True, None, 0.33), run_limited, True),
    "limited_weights/limitedVanLeer": (BOTH, prep_limited("limitedVanLeer -0.2 0.3", "vanLeer", False, (-0.2, 0.3), None), run_limited, True),
    "linear_upwind_correction/1": (BOTH, prep_linear_upwind(1, 1.0), run_linear_upwind, True),
    "linear_upwind_correction/4": (BOTH, prep_linear_upwind(4, 0.25), run_linear_upwind, True),
    "div_dev_tgrad/dev": (BOTH, prep_dev_tgrad("dev"), run_dev_tgrad, True),
    "div_dev_tgrad/dev2": (BOTH, prep_dev_tgrad("dev2"), run_dev_tgrad, True),
    "set_values/fvMatrix": (BOTH, prep_set_values(False), run_set_values, True),
    "set_values/upstream": (BOTH, prep_set_values(True), run_set_values, True),
    "patch_add/0": (("box",), prep_patch("add", 0), run_patch, False),
    "patch_add/1": (("box",), prep_patch("add", 1), run_patch, False),
    "patch_add/2": (("box",), prep_patch("add", 2), run_patch, False),
    "patch_add_product/0": (("box",), prep_patch("add_product", 0), run_patch, False),
    "patch_add_product/1": (("box",), prep_patch("add_product", 1), run_patch, False),
    "patch_max": (("box",), prep_patch("max", None), run_patch, False),
}
CASES = [(entry, mesh) for entry, spec in ENTRIES.items() for mesh in spec[0]]
_PREPARED, _DEFAULT = {}, {}          # (entry, mesh) -> inputs and reference; (entry, mesh, tables) -> the default grid's results: computed once


def assert_results(got, q, what, base=None):
    assert sorted(got) == sorted(q["ref"]), what
    for key, ref in q["ref"].items():
        assert not np.isnan(ref).any(), (what, key)
        assert not np.isnan(got[key]).any(), (what, key, "an output kept its NaN prefill", int(np.isnan(got[key]).sum()))
        assert same(got[key], ref), (what, key, "against the reference", int(np.sum(got[key] != ref)))
        if base is not None:
            assert same(got[key], base[key]), (what, key, "against the default grid")


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("entry,mesh", CASES, ids=[f"{entry.replace('/', '.')}-{mesh}" for entry, mesh in CASES])
def test_entry_under_a_forced_grid(pkg, orc, monkeypatch, entry, mesh, grid):
    _, prepare, run, xcd_form = ENTRIES[entry]
    if (entry, mesh) not in _PREPARED:
        _PREPARED[entry, mesh] = prepare(pkg, orc, mesh)
    q = _PREPARED[entry, mesh]
    for tables in (("default", "noxcd") if xcd_form else ("default",)):
        if (entry, mesh, tables) not in _DEFAULT:
            base = run(Env(pkg, monkeypatch, None, tables), q)
            assert_results(base, q, (entry, mesh, tables, "default grid"))
            _DEFAULT[entry, mesh, tables] = base
        got = run(Env(pkg, monkeypatch, grid, tables), q)                  # a second context: the switch is read when a context is created
        assert_results(got, q, (entry, mesh, tables, grid), _DEFAULT[entry, mesh, tables])


# ---- natural sizes past the shipped cap --------------------------------------------------------------------------------------------------
FACE_BOX = (129, 127, 44)       # 720 852 cells, 2 134 909 internal faces


def face_sample(pkg, nf):
    """where a wrong stride or chunk shows: both ends, both sides of the cap, both sides of every XCD run of chunks (multiples of
    512*1024), and seeded faces anywhere"""
    edge = CAP * 256
    parts = [np.arange(512), np.arange(nf - 637, nf), np.arange(edge - 256, edge + 256)]
    parts += [np.arange(m - 256, m + 256) for m in range(512 * 1024, nf, 512 * 1024)]
    parts.append((pkg.synthetic.splitmix_uniform(97, 4096) * nf).astype(np.int64))
    return np.unique(np.concatenate(parts))


@pytest.fixture(scope="module")
def face_box(pkg):
    import torch
    case = pkg.synthetic.box_case(*FACE_BOX)
    n, nf = case.n_cells, case.n_faces
    assert (n, nf) == (720852, 2134909) and grid_for(nf) == CAP
    os.environ.pop("MI_FACE_GRID", None)                                   # the shipped cap
    eng, ctx, dev, host, N = gpu_env(pkg, fill=NAN)
    q = dict(n=n, nf=nf, lo=case.lower_addr, up=case.upper_addr, eng=eng, ctx=ctx, dev=dev, host=host, N=N)
    q["A"] = eng.Assembly(eng.Addressing(ctx, n, q["lo"], q["up"]))
    yield q
    del q["A"]
    torch.cuda.empty_cache()


def whole(got, ref, what):
    """the whole array: the reference is vectorised and takes a second or two at this size"""
    assert got.shape == ref.shape and not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert same(got, ref), (what, int(np.sum(got != ref)), np.nonzero(got != ref)[0][:4])


@pytest.mark.gpu
def test_fvc_div_past_the_cap(pkg, orc, face_box):
    """k_face_conv_flux, grid-stride: the second trip covers the faces 2 097 152 .. 2 134 908"""
    b, u = face_box, pkg.synthetic.splitmix_uniform
    n, nf, lo, up, dev = b["n"], b["nf"], b["lo"], b["up"], b["dev"]
    phi, w, cellf, vol = u(10, nf) - 0.5, u(9, nf), u(12, n), 0.5 + u(11, n)
    for wts in (w, None):
        face, div = b["N"](nf), b["N"](n)
        b["A"].fvc_div(dev(phi), None if wts is None else dev(wts), dev(cellf), dev(vol), face, div)
        ref = phi * orc.face_interpolate(lo, up, orc.upwind_weights(phi) if wts is None else wts, cellf)
        whole(b["host"](face), ref, ("face", wts is None))
        whole(b["host"](div), orc.surface_integrate(n, lo, up, ref, vol), ("div", wts is None))


@pytest.mark.gpu
def test_ddt_phi_corr_local_and_backward_past_the_cap(pkg, orc, face_box):
    """k_ddt_phi_corr_local (grid-stride) and k_ddt_phi_corr_backward (block_chunk: chunks of 512, 4 170 busy blocks of 8 192, the last
    one partial)"""
    from test_backward_ddt import coeffs, ddt_corr as backward_corr
    from test_local_ddt import ddt_corr as local_corr
    b = face_box
    n, nf, lo, up, dev = b["n"], b["nf"], b["lo"], b["up"], b["dev"]
    d = _ddt_corr_inputs(pkg, orc, b, True)
    c, rdt = coeffs(0.004, 0.01), 1.0 / 0.004
    out = b["N"](nf)
    b["A"].ddt_phi_corr_backward(rdt, c, dev(d["lam"]), [dev(x) for x in d["Sf"]], [dev(x) for x in d["U0"]], [dev(x) for x in d["U00"]], dev(d["rho0"]),
                                 dev(d["rho00"]), dev(d["phi0"]), dev(d["phi00"]), out)
    ref, k, _ = backward_corr(orc, n, lo, up, rdt, c, d["lam"], d["Sf"], d["U0"], d["U00"], d["rho0"], d["rho00"], d["phi0"], d["phi00"])
    assert np.any(k == 0.0) and np.any(k == 1.0)
    whole(b["host"](out), ref, "backward")
    out = b["N"](nf)
    b["A"].ddt_phi_corr_local(dev(d["r"]), dev(d["lam"]), [dev(x) for x in d["Sf"]], [dev(x) for x in d["U0"]], dev(d["phi0"]), out)
    whole(b["host"](out), local_corr(orc, n, lo, up, d["r"], d["lam"], d["Sf"], d["U0"], d["phi0"])[0], "local")


@pytest.mark.gpu
def test_div_dev_tgrad_past_the_cap(pkg, orc, face_box):
    """k_face_dev_tgrad_flux<MI_DEV>, block_chunk"""
    from test_div_dev_tgrad import internal
    b, u = face_box, pkg.synthetic.splitmix_uniform
    n, nf, dev = b["n"], b["nf"], b["dev"]
    G = dict(weights=0.2 + 0.6 * u(70, nf), Sf=np.stack([u(72 + k, nf) - 0.5 for k in range(3)], axis=1), V=0.5 + u(76, n))
    g, visc = [(u(21, n, start=i * n) - 0.5) * 128 for i in range(9)], 0.5 + u(22, n)
    face, div = [b["N"](nf) for _ in range(3)], [b["N"](n) for _ in range(3)]
    b["A"].div_dev_tgrad("dev", dev(G["weights"]), [dev(G["Sf"][:, k]) for k in range(3)], dev(visc), [dev(x) for x in g], face, div, dev(G["V"]))
    rface, rdiv = internal(orc, dict(n=n, nI=nf, lo=b["lo"], up=b["up"], G=G), "dev", visc, g, G["V"])
    for j in range(3):
        whole(b["host"](face[j]), rface[j], ("face", j))
        whole(b["host"](div[j]), rdiv[j], ("div", j))


@pytest.mark.gpu
def test_sngrad_limited_flux_past_the_cap(pkg, orc, face_box):
    """k_sngrad_limited_flux<3>, grid-stride.  The restatement's vector magnitude is exact rational arithmetic, face by face (5.5 s per
    100 000 faces: two minutes for all of them), so it is compared on face_sample, 7 288 faces; no face keeps its NaN prefill"""
    from test_limited_sngrad import limited_flux
    b, u = face_box, pkg.synthetic.splitmix_uniform
    n, nf, lo, up, dev = b["n"], b["nf"], b["lo"], b["up"], b["dev"]
    cv, lam, delta, gms = [0.3 * (u(77 + k, nf) - 0.5) for k in range(3)], 0.2 + 0.6 * u(70, nf), 1.0 + u(71, nf), 0.5 + u(75, nf)
    vf, g = [u(11, n, start=j * n) - 0.5 for j in range(3)], [(u(12, n, start=i * n) - 0.5) * 128 for i in range(9)]
    out, lim = [b["N"](nf) for _ in range(3)], b["N"](nf)
    b["A"].sngrad_limited_correction_flux(0.33, [dev(x) for x in cv], dev(lam), dev(delta), [dev(x) for x in vf], [dev(x) for x in g], dev(gms), out, lim)
    s = face_sample(pkg, nf)
    assert s[0] == 0 and s[-1] == nf - 1 and {CAP * 256 - 1, CAP * 256}.issubset(s.tolist())
    ref, rlim = limited_flux(orc, lo[s], up[s], 0.33, [x[s] for x in cv], lam[s], delta[s], vf, g, gms[s])
    assert np.any(rlim < 1.0) and np.any(rlim == 1.0)
    for j, t in enumerate(out + [lim]):
        got = b["host"](t)
        assert not np.isnan(got).any(), (j, int(np.isnan(got).sum()))
        assert same(got[s], ref[j] if j < 3 else rlim), j


CELL_BOX = (130, 130, 130)      # 2 197 000 cells


@pytest.fixture(scope="module")
def cell_box(pkg):
    import torch
    case = pkg.synthetic.box_case(*CELL_BOX, symmetric=False)
    assert case.n_cells == 2197000
    os.environ.pop("MI_FACE_GRID", None)
    eng, ctx, dev, host, N = gpu_env(pkg, fill=NAN)
    q = dict(case=case, eng=eng, ctx=ctx, dev=dev, host=host, N=N, A=eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)))
    yield q
    del q["A"]
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("upstream", [False, True])
def test_set_values_past_the_cap(pkg, orc, cell_box, upstream):
    """2 097 152 + 300 distinct labels in a seeded order: without a loop in k_set_values_cells the last 300 are dropped -- their psi and
    source keep their values and their neighbours' coefficients and sources are those of free cells"""
    import torch
    b, u = cell_box, pkg.synthetic.splitmix_uniform
    case, dev, host = b["case"], b["dev"], b["host"]
    n, nf, n_set = case.n_cells, case.n_faces, CAP * 256 + 300
    cells = np.argsort(u(81, n), kind="stable")[:n_set].astype(np.int32)
    vals, psi0 = u(82, n_set) - 0.5, u(83, n)
    psi, src, upper, lower = dev(psi0), dev(case.source), b["N"](nf), b["N"](nf)
    b["A"].set_values(torch.from_numpy(cells).to("cuda:0"), dev(vals), psi, dev(case.diag), src, dev(case.upper), dev(case.lower), upper, lower, upstream=upstream)
    sv = orc.set_values(n, case.lower_addr, case.upper_addr, cells, vals, psi0, case.diag, case.source, case.upper, case.lower, upstream=upstream)
    for key, t in (("psi", psi), ("source", src), ("upper", upper), ("lower", lower)):
        whole(host(t), sv[key], key)


@pytest.mark.gpu
def test_patch_kernels_past_the_cap(pkg, orc):
    """k_patch_add<0>, k_patch_add<0, true> and k_patch_max over 2 100 000 unique cells (2 150 000 faces: 50 000 cells hold two)"""
    u = pkg.synthetic.splitmix_uniform
    os.environ.pop("MI_FACE_GRID", None)
    eng, ctx, dev, host, _ = gpu_env(pkg)
    n, nu, m = 2197000, 2100000, 2150000
    cells = np.argsort(u(91, n), kind="stable")[:nu]
    fc = np.concatenate([cells, cells[::42]])
    fc = fc[np.argsort(u(92, m), kind="stable")].astype(np.int32)
    assert fc.shape[0] == m and grid_for(nu) == CAP and nu > CAP * 256
    pf, qq, start = u(93, m) - 0.5, u(94, m), u(95, n) - 0.5
    patch = eng.Patch(ctx, n, fc)
    intf = dev(start); patch.add(dev(pf), intf, 0)
    whole(host(intf), orc.patch_add(fc, pf, start, 0), "add")
    intf = dev(start); patch.add_product(dev(pf), dev(qq), intf, 0)
    whole(host(intf), orc.patch_add_product(fc, pf, qq, start, 0), "add_product")
    intf = dev(start); patch.max(dev(pf), intf)
    ref = start.copy()
    np.maximum.at(ref, fc, pf)
    assert 0.3 * nu < np.sum(ref != start) < nu
    whole(host(intf), ref, "max")
