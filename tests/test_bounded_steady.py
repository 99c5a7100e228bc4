"""`div(phi,U) bounded Gauss <scheme>` and `ddtSchemes { default steadyState; }` (boundedConvectionScheme.C:69-92, steadyStateDdtScheme.C):
fvmDiv = scheme.fvmDiv(flux, vf) - fvm::Sp(divPhi, vf), divPhi = fvc::surfaceIntegrate(faceFlux) with the boundary faces; a steady matrix has no
time part at all.

The expected values are a numpy restatement, one rounding per operator (tests/test_backward_ddt.py says why that is the reference's
rounding); every comparison with the engine is bit for bit.  CPU: where the bounded diagonal differs from the plain one.  GPU:
mi_fvm_assemble_local with div_flux_dev -- alone (Euler), with the local time derivative, and steady -- against the engine's own unfused
sequence and against the restatement, in every block shape of the row pass."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from assembly_support import SHAPES, VARIANTS, FusedCase, gpu_env

SENTINEL = -7.25


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def bounded_diag(div_diag, V, div_phi):
    """the convection matrix's diagonal after `- fvm::Sp(divPhi, vf)`: V*divPhi rounded first (fvmSup.C:118), then subtracted
    (lduMatrixOperations.C:319-322)"""
    return div_diag - (V * div_phi)


def wall_box(pkg, orc, nx=6, ny=5, nz=4):
    """a uniform box, uniform velocity (1, 0, 0): inlet at x = 0, a NO-SLIP WALL at x = 1 (flux 0 where the outlet would be), slip sides.
    -> n, lo, up, V, phi (internal faces), divPhi = surfaceIntegrate(phi, boundary faces included)/V"""
    case = pkg.synthetic.box_case(nx, ny, nz)
    n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
    h = 1.0 / nx
    V = np.full(n, h * h * h)
    phi = np.where(up - lo == 1, h * h, 0.0)
    ivf = orc.surface_integrate(n, lo, up, phi)
    inlet = np.arange(n)[np.arange(n) % nx == 0]
    np.add.at(ivf, inlet, -(h * h))                                 # the inlet's faces: Sf points outwards; the wall's and the sides' add 0.0
    return n, lo, up, V, phi, ivf / V


def test_restated_bounded_diag_differs_exactly_where_the_flux_does_not_balance(pkg, orc):
    n, lo, up, V, phi, div_phi = wall_box(pkg, orc)
    nx = 6
    at_wall = np.arange(n) % nx == nx - 1
    assert np.all(div_phi[~at_wall] == 0.0) and np.all(div_phi[at_wall] < 0.0)        # what flows in does not flow out
    for w in (orc.upwind_weights(phi), np.full(phi.shape[0], 0.5)):
        _, _, dB = orc.fvm_div(n, lo, up, w, phi)
        d = bounded_diag(dB, V, div_phi)
        assert np.array_equal(d != dB, div_phi != 0.0)
        assert np.all(d[at_wall] > dB[at_wall])                                       # bounded: the missing outflow goes onto the diagonal
        assert np.array_equal(d[~at_wall], dB[~at_wall])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def unfused_bounded(V, ddt_call, div_phi):
    """assembly_support.unfused_sequence with `diag_div -= V*divPhi` inserted after mi_fvm_div -- the engine's own scheme-by-scheme calls"""
    c = V.case
    A, E, vol, lap, div, sp, su, R = c.A, c.E, c.vol, c.lap, V.div, V.sp, V.su, V.R
    n, nf = c.n, c.nf
    corr = div.get("correction")
    cl, cu, cd, lu, ld, dd, ds = E(nf), E(nf), E(n), E(nf), E(n), E(n), [E(n) for _ in range(R)]
    t = [E(nf) for _ in range(R)]
    flux, wts = div["flux"], div.get("weights")
    if wts is None:
        wts = E(nf); A.upwind_weights(flux, wts)
    A.fvm_div(wts, flux, cl, cu, cd)
    p = vol * div_phi; cd.sub_(p)                                   # - fvm::Sp(divPhi, vf)
    if corr:
        A.linear_upwind_correction(flux, corr["cf"], corr["c"], corr["grad"], t)
    A.fvm_laplacian(lap["delta_coeffs"], lap["gamma_magsf"], lu, ld)
    for r in range(R):
        ddt_call(r, dd, ds[r])
        if corr:
            ivf = E(n); A.surface_integrate(t[r], vol, ivf); A.submul(vol, ivf, ds[r])
        if su:
            A.fvm_su(vol, su[0][1][r], ds[r])
            p = vol * su[1][1][r]; ds[r].add_(p)
    A.axpby(1.0, cl, -1.0, lu, cl); A.axpby(1.0, cu, -1.0, lu, cu)
    A.axpby(1.0, dd, 1.0, cd, dd)
    A.axpby(1.0, dd, -1.0, ld, dd)
    if sp is not None:
        p = vol * sp[0]; dd.sub_(p)
    return dict(lower=cl, upper=cu, diag=dd, src=ds, t=t)


def assert_restated_bounded(V, got, seq, restated_ddt, div_phi):
    """assembly_support.FusedVariant.assert_restated with the bounded diagonal; restated_ddt(r) -> (diag, source), zeros for steadyState (the
    empty matrix the convection matrix is added to)"""
    c, v, q, orc, host = V.case, V.v, V.case.q, V.case.orc, V.case.host
    n, lo, up = c.n, c.lo, c.up
    wh = orc.upwind_weights(q["flux"]) if v["div"] is None else q["w"]
    lB, uB, dB = orc.fvm_div(n, lo, up, wh, q["flux"])
    dB = bounded_diag(dB, q["vol"], div_phi)
    lower, upper = lB - c.uL, uB - c.uL
    for r in range(V.R):
        dD, s = restated_ddt(r)
        if v["corr"]:
            s = s - q["vol"] * orc.surface_integrate(n, lo, up, host(seq["t"][r]), q["vol"])
        if v["extras"]:
            s = s - q["vol"] * q["su"][r]
            s = s + q["vol"] * q["su2"][r]
        assert np.array_equal(host(got["src"][r]), s), (V.tag, r)
    diag = (dD + dB) - c.dL
    if v["extras"]:
        diag = diag - q["vol"] * q["sp"]
    assert np.array_equal(host(got["diag"]), diag) and np.array_equal(host(got["upper"]), upper) and np.array_equal(host(got["lower"]), lower), V.tag
    assert np.array_equal(host(got["mag"]), orc.row_face_op(2, n, lo, up, lower, upper, np.zeros(n))), V.tag


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,tables", SHAPES)
def test_fused_bounded_and_steady_assembly_bit_for_bit(pkg, orc, monkeypatch, name, mode, tables):
    """mi_fvm_assemble_local with div_flux_dev: bounded alone (the Euler time derivative), bounded with the local time derivative, and steadyState +
    bounded (no time derivative) -- each against the engine's own unfused sequence and against the restatement; a divPhi of zeros gives
    mi_fvm_assemble's bits; the variant without a convection term checks the refusal"""
    from test_local_ddt import fvm_ddt as local_fvm_ddt
    F = FusedCase(pkg, orc, monkeypatch, name, mode, tables)
    eng, dev, host, A, q = F.eng, F.dev, F.host, F.A, F.q
    n, nf, vol = F.n, F.nf, F.vol
    u = pkg.synthetic.splitmix_uniform
    dph = orc.surface_integrate(n, F.lo, F.up, q["flux"], q["vol"])                   # the internal faces' part of a real divPhi
    dph[::9] = 0.0
    assert np.sum(dph != 0.0) > n // 2
    rh, rdt = 50.0 + 400.0 * u(181, n), 250.0
    div_phi, zeros, r = dev(dph), dev(np.zeros(n)), dev(rh)
    _, _, _, _, S = gpu_env(pkg, fill=SENTINEL)
    for v in VARIANTS:
        if v["corr"] and name != "box":
            continue
        V = F.variant(v)
        if V.div is None:                                                             # bounded needs a convection term: refused, nothing launched
            o = dict(upper=S(nf), diag=S(n), src=[S(n)])
            with pytest.raises(eng.MiError, match="without a convection term"):
                A.assemble(o["upper"], o["diag"], sources_out=o["src"], ddt=dict(V.ddt, r_delta_t=rdt), div=dict(flux=None, bounded=div_phi), laplacian=F.lap,
                           sp=V.sp, su=V.su)
            assert all(np.all(host(x) == SENTINEL) for x in (o["upper"], o["diag"], o["src"][0]))
            continue
        rkw = dict(rho=q["rho"], rho0=q["rho0"]) if v["field"] else dict(rho_value=1.2)
        rho_of = (lambda: q["rho"]) if v["field"] else (lambda: 1.2)
        euler = lambda k: ((rdt * rho_of()) * q["vol"], ((rdt * (q["rho0"] if v["field"] else 1.2)) * q["psi0"][k]) * q["vol"])
        steady_call = lambda k, dd, ds: (dd.zero_(), ds.zero_())
        fused = lambda ddt, b: (V.div.__setitem__("bounded", b), V.fused(ddt), V.div.pop("bounded"))[1]
        plain = V.fused(dict(V.ddt, r_delta_t=rdt))
        cases = [("bounded", dict(V.ddt, r_delta_t=rdt), V.euler(rdt), euler),
                 ("local + bounded", dict(V.ddt, local=dict(r_delta_t=r)), lambda k, dd, ds: A.fvm_ddt_local(r, vol, V.psi_old[k], dd, ds, **V.rho),
                  lambda k: local_fvm_ddt(rh, q["vol"], q["psi0"][k], **rkw)),
                 ("steady + bounded", dict(vol=vol), steady_call, lambda k: (np.zeros(n), np.zeros(n)))]
        for what, ddt, ddt_call, restated in cases:
            got = fused(ddt, div_phi)
            seq = unfused_bounded(V, ddt_call, div_phi)
            V.assert_same(got, seq, what)
            assert_restated_bounded(V, got, seq, restated, dph)
            if what == "bounded":
                changed = host(got["diag"]) != host(plain["diag"])
                assert np.array_equal(changed, dph != 0.0) and np.array_equal(host(got["upper"]), host(plain["upper"]))
        same = fused(dict(V.ddt, r_delta_t=rdt), zeros)                               # divPhi == 0: the plain scheme, bit for bit
        V.assert_same(same, plain, "divPhi 0")
        assert np.array_equal(host(same["mag"]), host(plain["mag"]))
    # refusals: divPhi among the outputs -- nothing launched
    V = F.variant(VARIANTS[1])
    o = dict(lower=S(nf), upper=S(nf), diag=S(n), src=[S(n)])
    for bad in (o["diag"], o["src"][0]):
        with pytest.raises(eng.MiError, match="must not be an output"):
            A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=dict(V.ddt, r_delta_t=rdt), div=dict(V.div, bounded=bad),
                       laplacian=F.lap)
    for x in (o["lower"], o["upper"], o["diag"], o["src"][0]):
        assert np.all(host(x) == SENTINEL)


# ---- scalarTransportFoam: steadyState, CoEuler and the bounded schemes -------------------------------------------------------------------
def channel_fields(pkg, orc, pts, faces, owner, neighbour, patches):
    """what the schemes read on the channel of tests/transport_walk.py::walk, formed as the walk forms its own: phi on the internal faces and per
    patch (fc, phi_b, deltaCoeffs_b, magSf_b); deltaCoeffs = 1/|delta|, on a patch the patch-normal delta nHat (nHat & (Cf - Cn)) (fvPatch.C:147-191)"""
    from test_polymesh import geometry
    G = geometry(pts, faces, owner, neighbour)
    n, nI = int(owner.max()) + 1, len(neighbour)
    lo, up = owner[:nI].astype(np.int32), neighbour.astype(np.int32)
    Sf = [np.ascontiguousarray(G["Sf"][:nI, k]) for k in range(3)]
    u0 = np.array([1.0, 0.2, 0.0])
    phi = orc.flux_div(n, lo, up, G["weights"], Sf, [np.full(n, u0[k]) for k in range(3)], want_div=False)
    dc = 1.0 / np.linalg.norm(G["C"][up] - G["C"][lo], axis=1)
    P = []
    for name, _, cnt, start in patches:
        fc = owner[start:start + cnt].astype(np.int32)
        sfb, msb = G["Sf"][start:start + cnt], G["magSf"][start:start + cnt]
        ub = np.tile(u0, (cnt, 1)) if name in ("inlet", "outlet") else np.zeros((cnt, 3))
        nhat = sfb / msb[:, None]
        nd = np.sum(nhat * (G["Cf"][start:start + cnt] - G["C"][fc]), axis=1)
        P.append(dict(fc=fc, phi=ub[:, 0] * sfb[:, 0] + ub[:, 1] * sfb[:, 1] + ub[:, 2] * sfb[:, 2], dc=1.0 / np.linalg.norm(nhat * nd[:, None], axis=1), magSf=msb))
    div_phi = orc.surface_integrate(n, lo, up, phi)
    for q in P:
        div_phi = orc.patch_add(q["fc"], q["phi"], div_phi, 0)
    return SimpleNamespace(n=n, lo=lo, up=up, V=G["V"], phi=phi, dc=dc, magSf=G["magSf"][:nI], P=P, div_phi=div_phi / G["V"])


class LocalDdt:
    """steadyState (max_co None) or CoEuler as the time scheme object of tests/transport_walk.py::walk, with or without the bounded convection
    scheme.  What assemble returns stands where fvm::ddt(T) stands in the walk's sum, so the bounded scheme's -V*divPhi rides on it: the
    reference subtracts it from the convection matrix's diagonal first -- another order of the same roundings, far inside the application bars"""

    def __init__(self, F, bounded, max_co=None):
        self.F, self.bounded, self.max_co = F, bounded, max_co

    def start_step(self, step, dts, Told):
        self.Told, self.dt = Told, dts[step]

    def r_delta_t(self):
        from test_local_ddt import co_cells, co_face
        F = self.F
        x = co_face(F.dc, F.phi, F.magSf, self.dt, self.max_co)
        return co_cells(F.n, F.lo, F.up, x, [(q["fc"], co_face(q["dc"], q["phi"], q["magSf"], self.dt, self.max_co)) for q in F.P])

    def assemble(self, V, non_orth, rep):
        from test_local_ddt import fvm_ddt
        dD, sD = (np.zeros(self.F.n), np.zeros(self.F.n)) if self.max_co is None else fvm_ddt(self.r_delta_t(), V, self.Told)
        return (dD - V * self.F.div_phi if self.bounded else dD), sD

    def state(self):
        return {}


# (tag, mesh, steps, deltaT, DT, ddt entry, bounded, convection scheme, corrected Laplacian, non-orthogonal correctors).  A steady run is one
# "time step" (a second one would start from the converged field, at a residual near the tolerance).  The steady central-differencing case takes
# DT = 0.05: the cell Peclet number |U| h / DT = (1/12)/0.05 is then below 2, where a steady central scheme is a sound discretisation.  CoEuler
# takes deltaT = 0.05: the Courant number of the x faces, 1 * 0.05 * 12 = 0.6, exceeds maxCo = 0.5, so the local step is at work.
APP_CASES = [("steady_upwind", (12, 8, 6), 1, 0.01, 0.01, "steadyState", True, "upwind", False, 0),
             ("steady_linear_corrected", (12, 9, 7), 1, 0.01, 0.05, "steadyState", True, "linear", True, 2),
             ("coeuler_upwind", (12, 8, 6), 4, 0.05, 0.01, "CoEuler phi rho 0.5", False, "upwind", False, 0)]
TOL = 1e-10


def run_walk(pkg, orc, mesh, tin, T0, DT, dts, scheme, corrected, n_non_orth, ddt):
    import transport_walk
    pts, faces, owner, neighbour, patches = mesh
    return transport_walk.walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme, "corrected" if corrected else None, n_non_orth, ddt=ddt)


@pytest.mark.gpu
@pytest.mark.parametrize("tag, dims, n_steps, delta_t, DT, ddt_entry, bounded, scheme, corrected, n_non_orth", APP_CASES)
def test_scalarTransportFoam_steady_bounded_and_co_euler(pkg, orc, tmp_path, tag, dims, n_steps, delta_t, DT, ddt_entry, bounded, scheme, corrected, n_non_orth):
    """the application with `default steadyState` + `bounded Gauss ...` and with `default CoEuler phi rho 0.5`: every solver line and the written T
    against the walk of the same statements with the restatement; on the walk: the result is not the Euler run's, the bounded result not the
    plain scheme's, and no residual lies within a factor of two of the solver tolerance (an iteration count cannot flip on the last bit)"""
    from test_polymesh import PKG, read_vol_field
    from transport_walk import assert_solver_lines, rewrite_schemes, solver_lines
    from test_scalartransportfoam import write_channel
    case_dir = str(tmp_path / "channel")
    pts, faces, owner, neighbour, patches, tin, T0 = write_channel(case_dir, dims, DT, delta_t, n_steps, scheme, corrected, n_non_orth)
    mesh = (pts, faces, owner, neighbour, patches)
    rewrite_schemes(case_dir, ("ddtSchemes { default Euler; }", "ddtSchemes { default " + ddt_entry + "; }"))
    if bounded:
        rewrite_schemes(case_dir, ("div(phi,T) Gauss", "div(phi,T) bounded Gauss"))
    F = channel_fields(pkg, orc, *mesh)
    max_co = float(ddt_entry.split()[-1]) if ddt_entry.startswith("CoEuler") else None
    dts = [delta_t] * n_steps
    w = run_walk(pkg, orc, mesh, tin, T0, DT, dts, scheme, corrected, n_non_orth, LocalDdt(F, bounded, max_co))
    ref, Tref = w.lines, w.T
    scale = np.max(np.abs(Tref))
    Teuler = run_walk(pkg, orc, mesh, tin, T0, DT, dts, scheme, corrected, n_non_orth, None).T
    assert np.max(np.abs(Tref - Teuler)) > 1e-5 * scale
    if bounded:
        Tplain = run_walk(pkg, orc, mesh, tin, T0, DT, dts, scheme, corrected, n_non_orth, LocalDdt(F, False, max_co)).T
        assert np.max(np.abs(Tref - Tplain)) > 1e-5 * scale and np.any(F.div_phi != 0.0)
    if max_co is not None:
        r = LocalDdt(F, False, max_co); r.start_step(0, dts, T0)
        assert np.any(r.r_delta_t() > 1.0 / delta_t)                      # the local step is at work
    for line in ref:
        for res in line[2:4]:
            assert not (TOL / 2 <= res <= 2 * TOL), line
        assert line[4] < 1000, line
    out = subprocess.run([os.path.join(PKG, "scalarTransportFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout[-1500:]
    got = solver_lines(out.stdout)
    assert len(got) == len(ref) == n_steps * (n_non_orth + 1)
    assert_solver_lines(got, ref)
    f = read_vol_field(os.path.join(case_dir, f"{n_steps * delta_t:.10g}", "T"))
    assert f["header"]["class"] == "volScalarField" and np.max(np.abs(f["internalField"] - Tref)) <= 1e-8 * scale
    assert 0.05 < np.max(Tref) < 2.0


@pytest.mark.gpu
def test_scalarTransportFoam_refuses_co_euler_without_max_co(pkg, tmp_path):
    from test_polymesh import PKG
    from transport_walk import rewrite_schemes
    from test_scalartransportfoam import write_channel
    case_dir = str(tmp_path / "channel")
    write_channel(case_dir, (12, 8, 6), 0.01, 0.01, 1, "upwind", False, 0)
    rewrite_schemes(case_dir, ("ddtSchemes { default Euler; }", "ddtSchemes { default CoEuler phi rho; }"))
    out = subprocess.run([os.path.join(PKG, "scalarTransportFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "CoEuler" in out.stderr + out.stdout and "maxCo" in out.stderr + out.stdout, out.stderr + out.stdout[-800:]
