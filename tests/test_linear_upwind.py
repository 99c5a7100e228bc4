"""`Gauss linearUpwind grad(U)` / `Gauss LUST grad(U)`: the explicit correction that gaussConvectionScheme::fvmDiv adds to the div
matrix (gaussConvectionScheme.C:109-112; linearUpwind.C:33-62; LUST.H:104-126).  An independent restatement of the reference's
functors (CPU), then the engine's face pass, patch pass, LUST weights and the fused assembly against it and against the engine's own
unfused sequence, bit for bit (gpu)."""
import numpy as np
import pytest

from assembly_support import (ROW_MODES, bits, box_centres, dot_contracted, gpu_env, lust_weights, same, set_row_blocks, set_row_tables, shape_case,
                              shaped_addressing, signed_flux)


def restate_internal(lo, up, flux, cf, C, grads, scale):
    """faceFlux*(scale*correction) on the internal faces: c = owner if faceFlux > 0 (strict) else neighbour,
    corr = (Cf - C[c]) & grad_r[c]; two stored fields (scale*corr, then the product)"""
    lo, up, flux = lo.tolist(), up.tolist(), flux.tolist()
    cf = [x.tolist() for x in cf]; C = [x.tolist() for x in C]; grads = [[x.tolist() for x in g] for g in grads]
    out = [np.empty(len(flux)) for _ in grads]
    for f, fl in enumerate(flux):
        c = lo[f] if fl > 0 else up[f]
        dx, dy, dz = cf[0][f] - C[0][c], cf[1][f] - C[1][c], cf[2][f] - C[2][c]
        for r, g in enumerate(grads):
            out[r][f] = fl * (scale * dot_contracted(dx, dy, dz, g[0][c], g[1][c], g[2][c]))
    return out


def restate_patch(fc, pflux, pcf, C, pd, grads, nbr, scale):
    """the coupled-patch functor the reference runs: faceFlux > 0: (pCf - C[o]) & grad[o]; else ((pCf - C[o]) - pd) & gradNbr[i]"""
    out = [np.empty(len(pflux)) for _ in grads]
    for i, fl in enumerate(pflux.tolist()):
        o = int(fc[i])
        dx, dy, dz = pcf[0][i] - C[0][o], pcf[1][i] - C[1][o], pcf[2][i] - C[2][o]
        for r in range(len(grads)):
            if fl > 0:
                g = [grads[r][k][o] for k in range(3)]
            else:
                g = [nbr[r][k][i] for k in range(3)]
            e = (dx, dy, dz) if fl > 0 else (dx - pd[0][i], dy - pd[1][i], dz - pd[2][i])
            out[r][i] = fl * (scale * dot_contracted(*e, *g))
    return out


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_restatement_reconstructs_the_face_value_of_a_linear_field(pkg):
    """phi_upwind + correction = phi(Cf) exactly for a linear field with its exact gradient -- what the correction is for -- and the
    upwind cell of the correction is the neighbour at a zero flux (strict >), while the weights take the owner there (>=)"""
    syn = pkg.synthetic
    dims = (6, 5, 4)
    case = syn.box_case(*dims)
    lo, up = case.lower_addr, case.upper_addr
    C = box_centres(dims)
    cf = [0.5 * (x[lo] + x[up]) for x in C]
    a, b = np.array([0.75, -1.25, 0.5]), 0.3
    phi = lambda X: a[0] * X[0] + a[1] * X[1] + a[2] * X[2] + b
    grad = [np.full(case.n_cells, a[k]) for k in range(3)]
    flux = signed_flux(syn.splitmix_uniform(3, case.n_faces))
    assert np.any(flux > 0) and np.any(flux < 0) and np.any(flux == 0)
    unit = np.where(flux > 0, 1.0, -1.0)                   # the same upwind side as flux, |flux| = 1: t = +-corr exactly
    corr = restate_internal(lo, up, unit, cf, C, [grad], 1.0)[0] * unit
    t = restate_internal(lo, up, flux, cf, C, [grad], 1.0)[0]
    up_cell = np.where(flux > 0, lo, up)
    assert np.max(np.abs(phi(C)[up_cell] + corr - phi(cf))) < 1e-14
    # the zero-flux faces take the neighbour: their correction is (Cf - C[N]) & a, not (Cf - C[P]) & a
    z = flux == 0
    d_nei = sum((cf[k] - C[k][up]) * a[k] for k in range(3))
    assert np.allclose(corr[z], d_nei[z], rtol=0, atol=1e-15) and np.all(np.abs(d_nei[z]) > 1e-3)
    assert np.all(np.abs(t[z]) == 0.0)
    # LUST: a quarter of the correction; the weights blend linear and upwind (pos(): >= 0, the owner at a zero flux)
    cq = restate_internal(lo, up, np.ones(case.n_faces), cf, C, [grad], 0.25)[0]
    assert np.array_equal(cq, 0.25 * restate_internal(lo, up, np.ones(case.n_faces), cf, C, [grad], 1.0)[0])
    w = lust_weights(np.full(case.n_faces, 0.5), flux)
    assert np.all(w[flux >= 0] == 0.625) and np.all(w[flux < 0] == 0.375)


def test_library_exports_the_correction_entry_points(pkg):
    lib = pkg.engine.lib()
    for name in ("mi_linear_upwind_correction", "mi_patch_linear_upwind_correction", "mi_lust_weights", "mi_fvm_assemble_corrected"):
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS


def test_mirror_exports_the_corrected_convection(pkg):
    """foam/miFoam: fvc::linearUpwindCorrectionFlux (scalar, vector), LUSTWeights, fvm::assemble with the correction (scalar, vector)"""
    import os
    import subprocess
    so = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "libmiFoam.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", so], capture_output=True, text=True, check=True).stdout
    assert syms.count("Foam::fvc::linearUpwindCorrectionFlux(") == 2
    assert "Foam::LUSTWeights(" in syms
    assert sum("Foam::fvm::assemble(" in line and "linearUpwindCorrection" in line for line in syms.splitlines()) == 2


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _mesh(pkg, name):
    """-> (n, lo, up, C, Cf): the box, the skewed mesh, the random graph (seeded centres)"""
    syn = pkg.synthetic
    if name == "box":
        dims = (13, 11, 9)
        case = syn.box_case(*dims)
        C = box_centres(dims)
        return case.n_cells, case.lower_addr, case.upper_addr, C, [0.5 * (x[case.lower_addr] + x[case.upper_addr]) for x in C]
    if name == "skewed":
        from test_assembly import skewed_mesh
        M = skewed_mesh((9, 8, 7))
        G, nI = M["G"], M["nI"]
        return M["n"], M["lo"], M["up"], [np.ascontiguousarray(G["C"][:, k]) for k in range(3)], [np.ascontiguousarray(G["Cf"][:nI, k]) for k in range(3)]
    from conftest import random_graph_case
    case = random_graph_case(pkg, 1500, extra=2.5, seed=11)
    u = syn.splitmix_uniform
    return case.n_cells, case.lower_addr, case.upper_addr, [u(40 + k, case.n_cells) for k in range(3)], [u(50 + k, case.n_faces) for k in range(3)]


def _grads(pkg, n, n_rhs, seed):
    u = pkg.synthetic.splitmix_uniform
    return [[4.0 * (u(seed + 3 * r + k, n) - 0.5) for k in range(3)] for r in range(n_rhs)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "skewed", "graph", "skewed_noxcd"])
def test_face_pass_and_lust_weights_against_the_restatement(pkg, monkeypatch, name):
    if name.endswith("_noxcd"):   # the plain blockIdx.x mapping of the face pass
        set_row_tables(monkeypatch, "noxcd"); name = name[:-len("_noxcd")]
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    n, lo, up, C, cf = _mesh(pkg, name)
    nf = lo.shape[0]
    addr = eng.Addressing(ctx, n, lo, up)
    A = eng.Assembly(addr)
    flux = signed_flux(syn.splitmix_uniform(7, nf))
    fd, Cd, cfd = dev(flux), [dev(x) for x in C], [dev(x) for x in cf]
    for n_rhs, scale in ((1, 1.0), (3, 1.0), (4, 0.25), (3, 0.25)):
        g = _grads(pkg, n, n_rhs, 60 + n_rhs)
        out = [E(nf) for _ in range(n_rhs)]
        A.linear_upwind_correction(fd, cfd, Cd, [[dev(x) for x in gr] for gr in g], out, scale=scale)
        ref = restate_internal(lo, up, flux, cf, C, g, scale)
        for r in range(n_rhs):
            assert same(host(out[r]), ref[r]), (n_rhs, scale, r)
    # LUST weights
    cdw = 0.3 + 0.4 * syn.splitmix_uniform(8, nf)
    w = E(nf)
    A.lust_weights(dev(cdw), fd, w)
    assert same(host(w), lust_weights(cdw, flux))


@pytest.mark.gpu
def test_unfused_sequence_and_the_cyclic_patch(pkg, orc):
    """face pass -> mi_surface_integrate(t, V) -> source -= V*ivf against the oracle's surfaceIntegrate and the rounded product; then a
    cyclic channel: the patch pass with patchNeighbourField gradients, the patch faces added before the division by V -- and the fused
    call refusing that addressing"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    dims = (12, 7, 6)
    case = syn.box_case(*dims)
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    C = box_centres(dims); cf = [0.5 * (x[lo] + x[up]) for x in C]
    V = 0.5 + u(1, n); src = u(2, n) - 0.5
    flux = signed_flux(u(3, nf))
    g = _grads(pkg, n, 3, 70)
    Cd, cfd, gd, Vd = [dev(x) for x in C], [dev(x) for x in cf], [[dev(x) for x in gr] for gr in g], dev(V)
    addr = eng.Addressing(ctx, n, lo, up)
    A = eng.Assembly(addr)
    t = [E(nf) for _ in range(3)]
    A.linear_upwind_correction(dev(flux), cfd, Cd, gd, t)
    rt = restate_internal(lo, up, flux, cf, C, g, 1.0)
    for r in range(3):
        ivf = E(n); A.surface_integrate(t[r], Vd, ivf)
        rivf = orc.surface_integrate(n, lo, up, rt[r], V)
        assert same(host(ivf), rivf)
        s = dev(src); A.submul(Vd, ivf, s)
        assert same(host(s), src - V * rivf)

    # the cyclic channel: x-min <-> x-max
    cyc = syn.add_cyclic_x(case)
    fcs = [i.face_cells for i in cyc.interfaces]
    nbrs = [cyc.interfaces[i.nbr_patch].face_cells for i in cyc.interfaces]
    caddr = eng.Addressing(ctx, n, lo, up, fcs, nbrs)
    assert caddr.n_ext > 0
    mat = eng.Matrix(caddr)
    CA = eng.Assembly(caddr)
    h = 1.0 / dims[0]
    npf = [len(f) for f in fcs]
    pflux = [signed_flux(u(80 + p, m)) for p, m in enumerate(npf)]
    pcf = [[np.full(npf[p], 0.0 if p == 0 else 1.0), C[1][fcs[p]], C[2][fcs[p]]] for p in range(2)]   # the x = 0 / x = 1 planes
    pd = [[np.full(npf[p], (-h if p == 0 else h) if k == 0 else 0.0) for k in range(3)] for p in range(2)]
    # patchNeighbourField of every gradient component through the engine (the partner patch's cells), concatenated by patch
    nbr_all = [[E(sum(npf)) for _ in range(3)] for _ in range(3)]
    for r in range(3):
        for k in range(3):
            mat.patch_neighbour_field(gd[r][k], nbr_all[r][k])
    nbr_h = [[host(x) for x in row] for row in nbr_all]
    off = [0, npf[0]]
    for r in range(3):
        for k in range(3):
            assert same(nbr_h[r][k], np.concatenate([g[r][k][q] for q in nbrs]))
    ivf = [E(n) for _ in range(3)]
    for r in range(3):
        CA.surface_integrate(t[r], None, ivf[r])
    rivf = [orc.surface_integrate(n, lo, up, rt[r], None) for r in range(3)]
    for p in range(2):
        P = eng.Patch(ctx, n, fcs[p])
        pt = [E(npf[p]) for _ in range(3)]
        nb = [[nbr_all[r][k][off[p]:off[p] + npf[p]].contiguous() for k in range(3)] for r in range(3)]
        P.linear_upwind_correction(dev(pflux[p]), [dev(x) for x in pcf[p]], Cd, [dev(x) for x in pd[p]], gd, nb, pt)
        nbh = [[x[off[p]:off[p] + npf[p]] for x in row] for row in nbr_h]
        rpt = restate_patch(fcs[p], pflux[p], pcf[p], C, pd[p], g, nbh, 1.0)
        for r in range(3):
            assert same(host(pt[r]), rpt[r]), (p, r)
            P.add(pt[r], ivf[r], 0)
            rivf[r] = orc.patch_add(fcs[p], rpt[r], rivf[r], 0)
        P.close()
    for r in range(3):
        eng._chk(eng.lib().mi_vec_div(ctx.h, n, eng._ptr(ivf[r]), eng._ptr(Vd), eng._ptr(ivf[r])))
        s = dev(src); CA.submul(Vd, ivf[r], s)
        assert same(host(s), src - V * (rivf[r] / V)), r
    # the fused pass refuses coupled addressing: those faces are added before the division by V
    up_o, lo_o, dg = E(nf), E(nf), E(n)
    with pytest.raises(eng.MiError, match="coupled patches.*unfused"):
        CA.assemble(up_o, dg, lower_out=lo_o, sources_out=[E(n)], ddt=dict(vol=Vd), div=dict(flux=dev(flux), correction=dict(cf=cfd, c=Cd, grad=gd[:1])))


def _fused_vs_unfused(pkg, eng, ctx, addr, n, nf, q, cfg, dev, host, E):
    """mi_fvm_assemble_corrected against (a) mi_fvm_assemble for the coefficients and (b) the unfused source sequence:
    [ddt source | 0] -> correction face pass -> surfaceIntegrate(t, V) -> source -= V*ivf -> the explicit terms"""
    import torch
    A = eng.Assembly(addr)
    n_rhs, scale = cfg["n_rhs"], cfg["scale"]
    flux, vol = dev(q["flux"]), dev(q["vol"])
    w = None
    if scale != 1.0:
        w = E(nf); A.lust_weights(dev(q["cdw"]), flux, w)
    grads = [[dev(x) for x in gr] for gr in q["grad"][:n_rhs]]
    corr = dict(scale=scale, cf=[dev(x) for x in q["cf"]], c=[dev(x) for x in q["C"]], grad=grads)
    ddt = dict(vol=vol)
    if cfg["ddt"]:
        ddt.update(r_delta_t=q["rdt"], rho=dev(q["rho"]), rho_old=dev(q["rho0"]), psi_old=[dev(x) for x in q["psi0"][:n_rhs]])
    lap = dict(delta_coeffs=dev(q["delta"]), gamma_magsf=dev(q["gamma"])) if cfg["lap"] else None
    sp = (dev(q["sp"]), -1.0) if cfg["sp"] else None
    su = [(1.0, [dev(x) for x in q["su"][:n_rhs]]), (-1.0, [dev(x) for x in q["su2"][:n_rhs]])] if cfg["su"] else []
    outs = {}
    for tag, div in (("plain", dict(flux=flux, weights=w)), ("corr", dict(flux=flux, weights=w, correction=corr))):
        o = dict(lower=E(nf), upper=E(nf), diag=E(n), mag=E(n), src=[E(n) for _ in range(n_rhs)])
        A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=ddt, div=div, laplacian=lap, sp=sp, su=su, sum_mag_out=o["mag"])
        outs[tag] = o
    for k in ("lower", "upper", "diag", "mag"):
        assert same(host(outs["corr"][k]), host(outs["plain"][k])), k
    t = [E(nf) for _ in range(n_rhs)]
    A.linear_upwind_correction(flux, corr["cf"], corr["c"], grads, t, scale=scale)
    got = []
    for r in range(n_rhs):
        if cfg["ddt"]:
            s, dd = E(n), E(n)
            A.fvm_ddt_euler_rho(q["rdt"], dev(q["rho"]), dev(q["rho0"]), vol, dev(q["psi0"][r]), dd, s)
        else:
            s = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        ivf = E(n); A.surface_integrate(t[r], vol, ivf)
        A.submul(vol, ivf, s)
        if cfg["su"]:
            A.fvm_su(vol, dev(q["su"][r]), s)                                 # + su: source -= V*su
            p = vol * dev(q["su2"][r]); s.add_(p)                             # == su2: source += V*su2
        got.append(host(s))
        assert same(host(outs["corr"]["src"][r]), got[r]), (cfg, r)
    return got


def _fused_inputs(pkg, n, nf):
    u = pkg.synthetic.splitmix_uniform
    q = dict(flux=signed_flux(u(110, nf)), vol=0.5 + u(111, n), cdw=0.3 + 0.4 * u(140, nf), delta=1.0 + u(107, nf), gamma=0.5 + u(108, nf),
             rho=0.8 + u(135, n), rho0=0.7 + u(136, n), rdt=1.0 / 3e-4, sp=u(153, n),
             psi0=[u(131 + k, n) - 0.5 for k in range(4)], su=[u(154 + k, n) - 0.5 for k in range(4)], su2=[u(158 + k, n) - 0.5 for k in range(4)],
             C=[u(144 + k, n) for k in range(3)], cf=[u(147 + k, nf) for k in range(3)])
    q["grad"] = _grads(pkg, n, 4, 200)
    q["grad"][3] = [np.zeros(n) for _ in range(3)]          # a zero correction: t = +-0 -> ivf = +-0 -> the no-ddt source stays +0.0
    return q


CONFIGS = [
    dict(n_rhs=3, scale=1.0, ddt=True, lap=True, sp=True, su=True),       # momentum: linearUpwind with everything
    dict(n_rhs=4, scale=0.25, ddt=False, lap=True, sp=False, su=False),   # LUST, no ddt: 0.0 - V*ivf, the signed zero
    dict(n_rhs=1, scale=1.0, ddt=True, lap=False, sp=False, su=True),     # scalar, no diffusion
    dict(n_rhs=3, scale=0.25, ddt=False, lap=False, sp=True, su=True),    # LUST, no ddt, explicit terms after the correction
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ROW_MODES)
@pytest.mark.parametrize("name", ["box", "graph"])
def test_fused_correction_equals_the_unfused_sequence_bit_for_bit(pkg, monkeypatch, name, mode):
    set_row_blocks(monkeypatch, mode)
    eng, ctx, dev, host, E = gpu_env(pkg)
    case, addr = shaped_addressing(eng, ctx, pkg.synthetic, shape_case(pkg, name), mode)
    n, nf = case.n_cells, case.n_faces
    q = _fused_inputs(pkg, n, nf)
    for cfg in CONFIGS:
        got = _fused_vs_unfused(pkg, eng, ctx, addr, n, nf, q, cfg, dev, host, E)
        if cfg["n_rhs"] == 4 and not cfg["ddt"] and not cfg["su"]:
            assert np.all(bits(got[3]) == 0)                                # +0.0 everywhere, no -0.0
            assert np.any(got[0] != 0)


@pytest.mark.gpu
def test_fused_correction_argument_errors(pkg):
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    case = syn.box_case(9, 8, 7, symmetric=False)
    n, nf = case.n_cells, case.n_faces
    q = _fused_inputs(pkg, n, nf)
    addr = eng.Addressing(ctx, n, case.lower_addr, case.upper_addr)
    A = eng.Assembly(addr)
    flux, vol = dev(q["flux"]), dev(q["vol"])
    cf, C = [dev(x) for x in q["cf"]], [dev(x) for x in q["C"]]
    grads = [[dev(x) for x in gr] for gr in q["grad"][:3]]
    corr = dict(cf=cf, c=C, grad=grads)
    lo_o, up_o, dg, src = E(nf), E(nf), E(n), [E(n) for _ in range(3)]
    call = lambda **kw: A.assemble(kw.get("up", up_o), dg, lower_out=kw.get("lo", lo_o), sources_out=kw.get("src", src), ddt=dict(vol=vol),
                                   div=kw.get("div", dict(flux=flux, correction=kw.get("corr", corr))), laplacian=kw.get("lap"))
    call()                                                                  # valid
    lap = dict(delta_coeffs=dev(q["delta"]), gamma_magsf=dev(q["gamma"]))
    with pytest.raises(eng.MiError, match="without a convection term"):
        A.assemble(up_o, dg, lower_out=lo_o, sources_out=src, ddt=dict(vol=vol), laplacian=lap, div=dict(flux=None, correction=corr))
    with pytest.raises(eng.MiError, match="missing"):
        call(corr=dict(cf=cf, c=[C[0], None, C[2]], grad=grads))
    with pytest.raises(eng.MiError, match="missing"):
        call(corr=dict(cf=cf, c=C, grad=[grads[0], [grads[1][0], None, grads[1][2]], grads[2]]))
    with pytest.raises(eng.MiError, match="right-hand sides"):
        call(src=[])                                                        # a correction without a right-hand side
    with pytest.raises(eng.MiError, match="aligned"):
        big = E(nf + 1)
        call(corr=dict(cf=[big[1:], cf[1], cf[2]], c=C, grad=grads))
    with pytest.raises(eng.MiError, match="alias"):
        call(src=[src[0], grads[1][1], src[2]])                             # a source written over a gradient another block reads
    with pytest.raises(eng.MiError, match="alias"):
        call(up=cf[0])
    # the unfused face pass: the same refusals
    t = [E(nf) for _ in range(3)]
    with pytest.raises(eng.MiError, match="faceFlux"):
        A.linear_upwind_correction(None, cf, C, grads, t)
    with pytest.raises(eng.MiError, match="missing"):
        A.linear_upwind_correction(flux, [cf[0], None, cf[2]], C, grads, t)
    with pytest.raises(eng.MiError, match="aligned"):
        big = E(nf + 1)
        A.linear_upwind_correction(big[1:], cf, C, grads, t)
    with pytest.raises(eng.MiError, match="alias"):
        A.linear_upwind_correction(flux, cf, C, grads, [t[0], C[1], t[2]])
    with pytest.raises(eng.MiError, match="alias"):
        A.linear_upwind_correction(flux, cf, C, grads, [t[0], flux, t[2]])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_correction_at_the_bench_size(pkg):
    """216^3 (the bench case), three components, ddt + linearUpwind + laplacian: fused against unfused, bit for bit (on the device)"""
    import torch
    eng = pkg.engine
    syn = pkg.synthetic
    ctx = eng.Context(0, torch.cuda.current_stream().cuda_stream)
    case = syn.box_case(216, 216, 216)
    n, nf = case.n_cells, case.n_faces
    addr = eng.Addressing(ctx, n, case.lower_addr, case.upper_addr)
    A = eng.Assembly(addr)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device="cuda:0", generator=gen) * (b - a) + a
    E = lambda m: torch.empty(m, dtype=torch.float64, device="cuda:0")
    flux, vol = R(nf, -0.5, 0.5), R(n, 0.5, 1.5)
    flux[::7] = 0.0
    cf, C = [R(nf) for _ in range(3)], [R(n) for _ in range(3)]
    grads = [[R(n, -2.0, 2.0) for _ in range(3)] for _ in range(3)]
    psi0 = [R(n, -0.5, 0.5) for _ in range(3)]
    delta, gamma = R(nf, 1.0, 2.0), R(nf, 0.5, 1.5)
    ddt = dict(vol=vol, r_delta_t=1.0 / 3e-4, psi_old=psi0)
    lap = dict(delta_coeffs=delta, gamma_magsf=gamma)
    corr = dict(cf=cf, c=C, grad=grads)
    lo_o, up_o, dg, src = E(nf), E(nf), E(n), [E(n) for _ in range(3)]
    A.assemble(up_o, dg, lower_out=lo_o, sources_out=src, ddt=ddt, div=dict(flux=flux, correction=corr), laplacian=lap)
    lo_p, up_p, dg_p, src_p = E(nf), E(nf), E(n), [E(n) for _ in range(3)]
    A.assemble(up_p, dg_p, lower_out=lo_p, sources_out=src_p, ddt=dict(vol=vol, r_delta_t=1.0 / 3e-4, psi_old=psi0), div=dict(flux=flux), laplacian=lap)
    bitsq = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert bitsq(lo_o, lo_p) and bitsq(up_o, up_p) and bitsq(dg, dg_p)
    t = [E(nf) for _ in range(3)]
    A.linear_upwind_correction(flux, cf, C, grads, t)
    ivf = E(n)
    for r in range(3):
        A.surface_integrate(t[r], vol, ivf)
        s = src_p[r].clone()                    # the ddt source (no su terms): the correction follows it
        A.submul(vol, ivf, s)
        assert bitsq(src[r], s), r
        assert not bitsq(src[r], src_p[r])
    torch.cuda.synchronize()
