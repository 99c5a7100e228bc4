"""`ddtSchemes { default backward; }`: fvm::ddt, fvc::ddt, fvc::ddtCorr and the fused assembly with the backward time derivative
(backwardDdtScheme.C:57-69, 196-355, 456-607, 724-765, 868-950; ddtScheme.C:139-174; static mesh).

The expected values are a numpy restatement of the reference's field expressions written here: numpy evaluates one operator per pass
and rounds each, exactly as the reference's gpuField operators do, so every comparison with the engine is bit for bit.  CPU: the host
scalars through the C ABI, exactness for a quadratic in time, the order of accuracy.  GPU: the two streaming kernels, the ddtCorr face
pass, mi_fvm_assemble_backward against the engine's own unfused sequence and against the restatement in every block shape of the row
pass, the Euler path on the same inputs, a six-step time loop with changing step sizes, and scalarTransportFoam with `default backward`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from assembly_support import SHAPES, VARIANTS, FusedCase, gpu_env

GREAT = 1e15


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def coeffs(dt, dt0=None):
    """backwardDdtScheme.C:472-479 in the reference's order; dt0 None: fewer than two old times, deltaT0 = GREAT (:57-69)"""
    dt0 = GREAT if dt0 is None else dt0
    coefft = 1 + dt / (dt + dt0)
    coefft00 = dt * dt / (dt0 * (dt + dt0))
    coefft0 = coefft + coefft00
    return (coefft, coefft0, coefft00)


def fvm_ddt(rdt, c, V, p0, p00, rho_value=1.0, rho=None, rho0=None, rho00=None):
    """-> (diag, source) of fvmDdt (:456-607), constant density or density field"""
    if rho is None:
        return ((c[0] * rdt) * rho_value) * V, ((rdt * V) * rho_value) * ((c[1] * p0) - (c[2] * p00))
    return ((c[0] * rdt) * rho) * V, (rdt * V) * (((c[1] * rho0) * p0) - ((c[2] * rho00) * p00))


def fvc_ddt(rdt, c, f, f0, f00, rho_value=None, rho=None, rho0=None, rho00=None):
    """fvcDdt (:196-207 no density, :268-280 constant, :343-355 field)"""
    if rho is not None:
        return rdt * ((((c[0] * rho) * f) - ((c[1] * rho0) * f0)) + ((c[2] * rho00) * f00))
    bracket = ((c[0] * f) - (c[1] * f0)) + (c[2] * f00)
    return rdt * bracket if rho_value is None else (rdt * rho_value) * bracket


def ddt_corr(orc, n, lo, up, rdt, c, lam, Sf, U0, U00, rho0, rho00, phi0, phi00):
    """fvcDdtPhiCorr on the internal faces (:724-765, :868-950 first branch) -> (out, coupling coefficient, flux(U0 or rho0*U0)); the two
    fluxes are the oracle's pinned flux_face"""
    X0 = U0 if rho0 is None else [rho0 * u for u in U0]
    X00 = U00 if rho00 is None else [rho00 * u for u in U00]
    W = [(c[1] * a) - (c[2] * b) for a, b in zip(X0, X00)]
    fU = orc.flux_div(n, lo, up, lam, Sf, X0, want_div=False)
    fW = orc.flux_div(n, lo, up, lam, Sf, W, want_div=False)
    k = 1 - np.minimum(np.abs(phi0 - fU) / (np.abs(phi0) + 1e-15), 1.0)
    return (k * rdt) * (((c[1] * phi0) - (c[2] * phi00)) - fW), k, fU


COEFF_SETS = [("first", 5e-3, None), ("equal", 0.01, 0.01), ("unequal", 0.004, 0.01)]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_backward_coeffs_through_the_c_abi(pkg):
    """mi_ddt_backward_coeffs (host only) against the four-line restatement, bit for bit; its two refusals"""
    eng = pkg.engine
    lib = eng.lib()
    for _, dt, dt0 in COEFF_SETS:
        assert eng.ddt_backward_coeffs(dt, dt0) == coeffs(dt, dt0), (dt, dt0)
    assert eng.ddt_backward_coeffs(0.01, 0.01) == (1.5, 2.0, 0.5)
    assert eng.ddt_backward_coeffs(5e-3) == (1.0, 1.0, 2.5e-35)            # coefft00 is not zero: the old-old field is always read
    out = (C.c_double * 3)()
    call = lambda dt, dt0, n_old: lib.mi_ddt_backward_coeffs(C.c_double(dt), C.c_double(dt0), C.c_int32(n_old), out)
    assert call(0.004, 0.01, 2) == 0 and tuple(out) == coeffs(0.004, 0.01)
    assert call(0.004, 0.0, 1) == 0 and tuple(out) == coeffs(0.004)         # fewer than two old times: deltaT0 is not read
    assert call(0.004, -1.0, 0) == 0 and tuple(out) == coeffs(0.004)
    assert call(0.0, 0.01, 2) != 0 and call(-0.01, 0.01, 2) != 0            # MI_ERR_ARG: delta_t <= 0
    assert call(0.01, 0.0, 2) != 0 and call(0.01, -0.01, 3) != 0            # MI_ERR_ARG: delta_t0 <= 0 with two old times
    with pytest.raises(eng.MiError):
        eng.ddt_backward_coeffs(0.01, 0.0)


def test_restated_fvc_ddt_is_exact_for_a_quadratic_in_time():
    f = lambda t: 0.3 + 1.7 * t - 2.1 * t * t
    t0, d0, d1 = 0.2, 0.01, 0.004
    t2 = t0 + d0 + d1
    got = fvc_ddt(1.0 / d1, coeffs(d1, d0), np.array([f(t2)]), np.array([f(t0 + d0)]), np.array([f(t0)]))[0]
    assert abs(got - (1.7 - 4.2 * t2)) < 1e-12


def test_restated_fvm_ddt_is_second_order_and_euler_first():
    """dT/dt = -2 T, T(0) = 1, one cell of volume 0.37, Sp as V*k on the diagonal, to t = 1 with a GREAT first step"""
    V, k = np.array([0.37]), 2.0

    def error(steps, backward):
        dt = 1.0 / steps
        T0 = T00 = np.array([1.0])
        for s in range(steps):
            if backward:
                d, src = fvm_ddt(1.0 / dt, coeffs(dt, None if s == 0 else dt), V, T0, T00)
            else:
                d, src = (1.0 / dt) * V, ((1.0 / dt) * T0) * V
            T = src / (d + V * k)
            T00, T0 = T0, T
        return abs(T0[0] - np.exp(-2.0))

    eb = [error(s, True) for s in (20, 40, 80, 160)]
    ee = [error(s, False) for s in (20, 40, 80, 160)]
    for a, b in zip(eb, eb[1:]):
        assert 3.8 <= a / b <= 4.4, eb
    for a, b in zip(ee, ee[1:]):
        assert 1.9 <= a / b <= 2.1, ee


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 1027, 31 * 23 * 19, 1050625, 5243907])
def test_streaming_kernels_against_the_restatement(pkg, n):
    """mi_fvm_ddt_backward / mi_fvc_ddt_backward: the three density forms x the three coefficient sets; sizes with an odd tail and an unpaired
    element of the double2 loop"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    u = pkg.synthetic.splitmix_uniform
    syn = pkg.synthetic
    case = syn.box_case(2, 2, 2)
    asm = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
    V, p, p0, p00 = 0.5 + u(1, n), u(2, n) - 0.5, u(3, n) - 0.5, u(4, n) - 0.5
    rho, rho0, rho00 = 0.9 + u(5, n), 0.8 + u(6, n), 0.7 + u(7, n)
    d, s, o = E(n), E(n), E(n)
    for _, dt, dt0 in COEFF_SETS:
        c, rdt = coeffs(dt, dt0), 1.0 / dt
        assert eng.ddt_backward_coeffs(dt, dt0) == c
        for form in ("none", "constant", "field"):
            kw = dict(constant=dict(rho_value=1.3), field=dict(rho=rho, rho0=rho0, rho00=rho00)).get(form, {})
            ekw = dict(constant=dict(rho_value=1.3), field=dict(rho=dev(rho), rho_old=dev(rho0), rho_old_old=dev(rho00))).get(form, {})
            asm.fvm_ddt_backward(rdt, c, dev(V), dev(p0), dev(p00), d, s, **ekw)
            rd, rs = fvm_ddt(rdt, c, V, p0, p00, **kw)
            assert np.array_equal(host(d), rd) and np.array_equal(host(s), rs), (form, dt, dt0)
            asm.fvc_ddt_backward(rdt, c, dev(p), dev(p0), dev(p00), o, **ekw)
            assert np.array_equal(host(o), fvc_ddt(rdt, c, p, p0, p00, **kw)), (form, dt, dt0)
    if n != 1027:
        return
    # refusals: an output among the inputs, the two outputs the same array, a missing old-old field, one density array of three
    c, rdt = coeffs(0.01, 0.01), 100.0
    Vd, p0d, p00d, rd_ = dev(V), dev(p0), dev(p00), dev(rho)
    for bad in (lambda: asm.fvm_ddt_backward(rdt, c, Vd, p0d, p00d, p0d, s), lambda: asm.fvm_ddt_backward(rdt, c, Vd, p0d, p00d, d, Vd),
                lambda: asm.fvm_ddt_backward(rdt, c, Vd, p0d, p00d, d, d), lambda: asm.fvm_ddt_backward(rdt, c, Vd, p0d, None, d, s),
                lambda: asm.fvm_ddt_backward(rdt, c, Vd, p0d, p00d, d, s, rho=rd_, rho_old=rd_), lambda: asm.fvc_ddt_backward(rdt, c, p0d, p0d, p00d, p00d),
                lambda: asm.fvc_ddt_backward(rdt, c, p0d, p0d, None, o), lambda: asm.fvc_ddt_backward(rdt, c, p0d, p0d, p00d, o, rho_old_old=rd_)):
        with pytest.raises(eng.MiError):
            bad()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "graph"])
def test_ddt_corr_against_the_restatement(pkg, orc, name):
    """mi_ddt_phi_corr_backward with and without density; faces with phi0 == 0.0 (coefficient 0) and faces whose phi0 equals flux(U0) bit for
    bit (coefficient 1)"""
    from conftest import random_graph_case
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    case = syn.box_case(13, 11, 9) if name == "box" else random_graph_case(pkg, 9000, extra=3.0, seed=5)
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    asm = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    lam = 0.001 + 0.998 * u(9, nf)
    assert np.all((lam > 0) & (lam < 1))
    Sf = [u(10 + k, nf) - 0.5 for k in range(3)]
    U0, U00 = [u(13 + k, n) - 0.5 for k in range(3)], [u(16 + k, n) - 0.5 for k in range(3)]
    rho0, rho00 = 0.8 + u(20, n), 0.7 + u(21, n)
    phi00 = u(23, nf) - 0.5
    out = E(nf)
    for r0, r00 in ((None, None), (rho0, rho00)):
        fU = orc.flux_div(n, lo, up, lam, Sf, U0 if r0 is None else [r0 * x for x in U0], want_div=False)
        phi0 = fU + 0.05 * (u(22, nf) - 0.5)          # near flux(U0): coefficients spread over (0, 1)
        phi0[::5] = 0.0
        phi0[2::7] = fU[2::7]
        for _, dt, dt0 in COEFF_SETS:
            c, rdt = coeffs(dt, dt0), 1.0 / dt
            ref, k, _ = ddt_corr(orc, n, lo, up, rdt, c, lam, Sf, U0, U00, r0, r00, phi0, phi00)
            one = np.zeros(nf, bool); one[2::7] = True
            zero = np.zeros(nf, bool); zero[::5] = True; zero &= ~one          # (the second assignment above wins where both hit)
            assert np.all(k[zero & (fU != 0)] == 0.0) and np.all(k[one] == 1.0) and np.any((k > 0.05) & (k < 0.95))
            asm.ddt_phi_corr_backward(rdt, c, dev(lam), [dev(x) for x in Sf], [dev(x) for x in U0], [dev(x) for x in U00],
                                      None if r0 is None else dev(r0), None if r00 is None else dev(r00), dev(phi0), dev(phi00), out)
            assert np.array_equal(host(out), ref), (r0 is None, dt, dt0)
    p0 = dev(phi0)
    for bad in (lambda: asm.ddt_phi_corr_backward(rdt, c, dev(lam), [dev(x) for x in Sf], [dev(x) for x in U0], [dev(x) for x in U00], dev(rho0), None, p0, dev(phi00), out),
                lambda: asm.ddt_phi_corr_backward(rdt, c, dev(lam), [dev(x) for x in Sf], [dev(x) for x in U0], [dev(x) for x in U00], None, None, p0, None, out),
                lambda: asm.ddt_phi_corr_backward(rdt, c, dev(lam), [dev(x) for x in Sf], [dev(x) for x in U0], [dev(x) for x in U00], None, None, p0, dev(phi00), p0)):
        with pytest.raises(eng.MiError):
            bad()


# ---- the fused assembly ----------------------------------------------------------------------------------------------------------
def backward_ddt_call(V, rdt, c):
    """the ddt_call of assembly_support.unfused_sequence for the backward scheme on the fields of the variant V"""
    return lambda r, dd, ds: V.case.A.fvm_ddt_backward(rdt, c, V.case.vol, V.psi_old[r], V.psi_old_old[r], dd, ds, rho_old_old=V.rho_old_old, **V.rho)


def backward_arg(V, c):
    """the `backward` key of Assembly.assemble's ddt argument on the fields of the variant V"""
    back = dict(coeffs=c, psi_old_old=V.psi_old_old)
    if V.rho_old_old is not None:
        back["rho_old_old"] = V.rho_old_old
    return back


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,tables", SHAPES)
def test_fused_backward_assembly_bit_for_bit(pkg, orc, monkeypatch, name, mode, tables):
    """mi_fvm_assemble_backward against (a) the engine's own unfused sequence -- mi_fvm_ddt_backward, mi_fvm_div, mi_fvm_laplacian, mi_fvm_su /
    Sp, the mi_vec_axpby combinations, in the order of tests/assembly_support.py::unfused_sequence -- and (b) the restatement (the corrected
    variants take the correction's face field from the engine's own face pass, which tests/test_linear_upwind.py pins); and on the same
    inputs the Euler call, which takes no `backward` key, against its unfused sequence."""
    F = FusedCase(pkg, orc, monkeypatch, name, mode, tables)
    eng, dev, host, E, A, addr, q = F.eng, F.dev, F.host, F.E, F.A, F.addr, F.q
    n, nf, vol, flux, lap = F.n, F.nf, F.vol, F.flux, F.lap
    dt, dt0 = 0.004, 0.01
    c, rdt = coeffs(dt, dt0), 1.0 / dt
    for v in VARIANTS:
        if v["corr"] and name != "box":
            continue
        V = F.variant(v)
        rkw = dict(rho=q["rho"], rho0=q["rho0"], rho00=q["rho00"]) if v["field"] else dict(rho_value=1.2)
        ddt = dict(V.ddt, r_delta_t=rdt)
        got = V.fused(dict(ddt, backward=backward_arg(V, c)))
        seq = V.unfused(backward_ddt_call(V, rdt, c))
        V.assert_same(got, seq, "backward")
        V.assert_restated(got, seq, lambda r: fvm_ddt(rdt, c, q["vol"], q["psi0"][r], q["psi00"][r], **rkw))
        # Euler untouched: the same call without the `backward` key
        eul = V.fused(ddt)
        V.assert_same(eul, V.unfused(V.euler(rdt)), "euler")
        for r in range(V.R):
            assert not np.array_equal(host(eul["src"][r]), host(got["src"][r]))
    # refusals of the backward entry point
    R = 1
    ddt = dict(r_delta_t=rdt, vol=vol, psi_old=[dev(q["psi0"][0])])
    p00 = dev(q["psi00"][0])
    o = dict(lower=E(nf), upper=E(nf), diag=E(n), src=[E(n)])
    call = lambda d: A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=d, div=dict(flux=flux), laplacian=lap)
    call(dict(ddt, backward=dict(coeffs=c, psi_old_old=[p00])))
    for bad in (dict(vol=vol, backward=dict(coeffs=c, psi_old_old=[p00])),                                   # terms->ddt == 0
                dict(ddt, backward=dict(coeffs=c, psi_old_old=[None])),                                      # a missing old-old field
                dict(ddt, backward=dict(coeffs=c, psi_old_old=[p00], rho_old_old=dev(q["rho00"]))),          # rho_old_old without rho
                dict(ddt, rho=dev(q["rho"]), rho_old=dev(q["rho0"]), backward=dict(coeffs=c, psi_old_old=[p00]))):   # rho without rho_old_old
        with pytest.raises(eng.MiError):
            call(bad)
    with pytest.raises(eng.MiError):                                                                         # a coefficient output aliasing an input
        A.assemble(flux, o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=dict(ddt, backward=dict(coeffs=c, psi_old_old=[p00])), div=dict(flux=flux))
    lib = eng.lib()
    t = eng.FvmTerms()
    assert lib.mi_fvm_assemble_backward(addr.h, C.byref(t), None, None, None, None, None, None, None) != 0   # bw NULL


# ---- the statements of scalarTransportFoam walked with the restatement ----------------------------------------------------------------
class BackwardDdt:
    """the time scheme object of tests/transport_walk.py::walk: fvm::ddt(T) by the restatement; the old-old field is kept from step to step
    (the first step: the old field, with GREAT as the previous step size)"""

    def start_step(self, step, dts, Told):
        self.Too = Told.copy() if step == 0 else self.Told
        self.Told, self.rdt = Told, 1.0 / dts[step]
        self.c = coeffs(dts[step], None if step == 0 else dts[step - 1])

    def assemble(self, V, non_orth, rep):
        return fvm_ddt(self.rdt, self.c, V, self.Told, self.Too)

    def state(self):
        return {}


def walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme, corrected, n_non_orth, backward=True):
    """tests/transport_walk.py::walk with the ddt line by the restatement (backward False: Euler) and one step size per step"""
    import transport_walk
    w = transport_walk.walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme, "corrected" if corrected else None, n_non_orth,
                            ddt=BackwardDdt() if backward else None)
    return w.lines, w.T, w.mesh


def _close(g, r):
    """the bars of tests/test_scalartransportfoam.py for one solver line (initial, final residual, iterations)"""
    return g[2] == r[2] and abs(g[0] - r[0]) <= 1e-7 * max(r[0], 1e-12) + 1e-14 and abs(g[1] - r[1]) <= 1e-6 * max(r[0], 1e-12) + 1e-14


@pytest.mark.gpu
def test_time_loop_with_changing_step_sizes(pkg, orc):
    """six steps of ddt(T) + div(phi,T) - laplacian(DT,T) through Python: fused assembly, PBiCG + DILU, against the same statements walked
    with the restatement and the oracle's PBiCG"""
    import torch
    from test_polymesh import make_box_mesh
    eng, ctx, dev, host, E = gpu_env(pkg)
    DT, dts = 0.01, [0.01, 0.01, 0.004, 0.008, 0.008, 0.01]
    pts, faces, owner, neighbour, patches = make_box_mesh((12, 8, 6), seed=None)
    cnt_in = [pt[2] for pt in patches if pt[0] == "inlet"][0]
    tin = 1.0 + 0.5 * np.sin(np.arange(cnt_in))
    n = int(owner.max()) + 1
    ref_lines, Tref, M = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, np.zeros(n), DT, dts, "linear", False, 0)
    _, Teuler, _ = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, np.zeros(n), DT, dts, "linear", False, 0, backward=False)
    G, nI, lo, up = M["G"], M["nI"], M["lo"], M["up"]
    addr = eng.Addressing(ctx, n, lo, up)
    A, mat = eng.Assembly(addr), eng.Matrix(addr)
    V, lam, phi = dev(G["V"]), dev(G["weights"]), dev(M["phi"])
    lap = dict(delta_coeffs=dev(G["delta"]), gamma_magsf=dev(DT * G["magSf"][:nI]))
    uL, dL = orc.fvm_laplacian(n, lo, up, G["delta"], DT * G["magSf"][:nI])
    lB, uB, dB = orc.fvm_div(n, lo, up, G["weights"], M["phi"])
    patch = [(eng.Patch(ctx, n, q["fc"]), dev(q["ic"]), dev(q["bc"])) for q in M["P"]]
    T = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    lower, upper, diag, src = E(nI), E(nI), E(n), E(n)
    Too = None
    for step, dt in enumerate(dts):
        Told = T.clone()
        if step == 0:
            Too = Told.clone()
        c = eng.ddt_backward_coeffs(dt, None if step == 0 else dts[step - 1])
        assert c == coeffs(dt, None if step == 0 else dts[step - 1])
        A.assemble(upper, diag, lower_out=lower, sources_out=[src], ddt=dict(r_delta_t=1.0 / dt, vol=V, psi_old=[Told], backward=dict(coeffs=c, psi_old_old=[Too])),
                   div=dict(flux=phi, weights=lam), laplacian=lap)
        dD, sD = fvm_ddt(1.0 / dt, c, G["V"], host(Told), host(Too))          # the restatement on the fields this step starts from
        assert np.array_equal(host(lower), lB - uL) and np.array_equal(host(upper), uB - uL), step
        assert np.array_equal(host(diag), (dD + dB) - dL) and np.array_equal(host(src), sD), step
        for p, ic, bc in patch:
            p.add(ic, diag, 0); p.add(bc, src, 0)
        mat.set_coeffs(diag, upper, lower)
        perf = mat.pbicg(T, src, "DILU", tolerance=1e-10, relTol=0.0)
        r = ref_lines[step]
        assert _close((perf["initialResidual"], perf["finalResidual"], perf["nIterations"]), r[2:]), (step, perf, r)
        Too = Told
    Tg = host(T)
    assert np.max(np.abs(Tg - Tref)) <= 1e-8 * np.max(np.abs(Tref))
    assert np.max(np.abs(Tref - Teuler)) > 1e-5 * np.max(np.abs(Tref))          # the scheme is not a no-op
    assert 0.05 < np.max(Tref) < 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("dims, n_steps, scheme, corrected, n_non_orth", [((12, 8, 6), 4, "upwind", False, 0), ((12, 9, 7), 3, "linear", True, 2)])
def test_scalarTransportFoam_with_the_backward_scheme(pkg, orc, tmp_path, dims, n_steps, scheme, corrected, n_non_orth):
    """the application with `ddtSchemes { default backward; }`: T.oldTime().oldTime() kept, GREAT on the first step, deltaT0 = deltaT
    afterwards; every solver line and the written T against the walk, with the comparisons of tests/test_scalartransportfoam.py"""
    from test_polymesh import PKG, read_vol_field
    from transport_walk import assert_solver_lines, rewrite_schemes, solver_lines
    from test_scalartransportfoam import write_channel
    DT, delta_t = 0.01, 0.01
    case_dir = str(tmp_path / "channel")
    pts, faces, owner, neighbour, patches, tin, T0 = write_channel(case_dir, dims, DT, delta_t, n_steps, scheme, corrected, n_non_orth)
    rewrite_schemes(case_dir, ("ddtSchemes { default Euler; }", "ddtSchemes { default backward; }"))
    ref, Tref, _ = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, [delta_t] * n_steps, scheme, corrected, n_non_orth)
    _, Teuler, _ = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, [delta_t] * n_steps, scheme, corrected, n_non_orth, backward=False)
    out = subprocess.run([os.path.join(PKG, "scalarTransportFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout[-1500:]
    got = solver_lines(out.stdout)
    assert len(got) == len(ref) == n_steps * (n_non_orth + 1)
    assert_solver_lines(got, ref)
    f = read_vol_field(os.path.join(case_dir, f"{n_steps * delta_t:.10g}", "T"))
    assert f["header"]["class"] == "volScalarField" and np.max(np.abs(f["internalField"] - Tref)) <= 1e-8 * np.max(np.abs(Tref))
    assert 0.05 < np.max(Tref) < 2.0 and np.min(Tref) > -0.2
    bf = dict(f["boundaryField"])
    assert bf["inlet"]["type"] == "fixedValue" and np.array_equal(bf["inlet"]["value"], tin) and bf["outlet"] == {"type": "zeroGradient"}
    assert np.max(np.abs(Teuler - Tref)) > 1e-5 * np.max(np.abs(Tref))          # not the Euler result
