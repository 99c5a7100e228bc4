"""The streaming (one element in, one element out) entries of the assembly at every size class of their double2 loop, bit for bit against
the restatements the schemes' own tests use: the oracle's sweeps, lust_weights / co_face of assembly_support, the local-time-step
expressions of tests/test_local_ddt.py, plain numpy for the quotient.  Each entry states its formula once per element; what can go wrong
is the element it is applied to -- the second of a pair, the unpaired last one of an odd chunk, the pairs of an unrolled body -- so the
sizes (STREAM_SIZES) walk those cases and the inputs differ from element to element."""
import ctypes as C

import numpy as np
import pytest

from assembly_support import STREAM_SIZES, co_face, gpu_env, lust_weights, same, signed_flux
from test_local_ddt import fvc_ddt as local_fvc_ddt, fvm_ddt as local_fvm_ddt


@pytest.mark.gpu
@pytest.mark.parametrize("n", STREAM_SIZES)
def test_streaming_entries_bit_for_bit(pkg, orc, n):
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    case = syn.box_case(2, 2, 2)
    asm = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
    V, p0, x, y = 0.5 + u(1, n), u(2, n) - 0.5, u(3, n) - 0.5, 0.25 + u(4, n)
    rho, rho0 = 0.9 + u(5, n), 0.8 + u(6, n)
    diag0, src0 = 1.0 + u(7, n), u(8, n) - 0.5
    susp = signed_flux(u(9, n))                                      # both signs and exact zeros: max(susp, 0) and min(susp, 0) both taken
    Vd, p0d, xd, yd, rhod, rho0d = dev(V), dev(p0), dev(x), dev(y), dev(rho), dev(rho0)
    d, s, o = E(n), E(n), E(n)
    # fvm::ddt, Euler: constant density and density field
    asm.fvm_ddt_euler(250.0, 1.3, Vd, p0d, d, s)
    rd, rs = orc.fvm_ddt_euler(250.0, 1.3, V, p0)
    assert same(host(d), rd) and same(host(s), rs)
    asm.fvm_ddt_euler_rho(250.0, rhod, rho0d, Vd, p0d, d, s)
    rd, rs = orc.fvm_ddt_euler_rho(250.0, rho, rho0, V, p0)
    assert same(host(d), rd) and same(host(s), rs)
    # fvm::Su, fvm::Sp (field and value), fvm::SuSp: in place
    s = dev(src0); asm.fvm_su(Vd, xd, s)
    assert same(host(s), orc.fvm_su(V, x, src0))
    d = dev(diag0); asm.fvm_sp(Vd, xd, d)
    assert same(host(d), orc.fvm_sp(V, x, diag0))
    d = dev(diag0); asm.fvm_sp(Vd, 0.375, d)
    assert same(host(d), orc.fvm_sp(V, 0.375, diag0))
    d, s = dev(diag0), dev(src0); asm.fvm_susp(Vd, dev(susp), p0d, d, s)
    rd, rs = orc.fvm_susp(V, susp, p0, diag0, src0)
    assert same(host(d), rd) and same(host(s), rs)
    # the vector helpers: inout -= x*y; a*x + b*y out of place and onto either input; x / y out of place and onto x
    s = dev(src0); asm.submul(xd, yd, s)
    assert same(host(s), orc.submul(x, y, src0))
    want = orc.axpby(1.5, x, -0.75, y)
    asm.axpby(1.5, xd, -0.75, yd, o)
    assert same(host(o), want)
    t = dev(x); asm.axpby(1.5, t, -0.75, yd, t)
    assert same(host(t), want)
    t = dev(y); asm.axpby(1.5, xd, -0.75, t, t)
    assert same(host(t), want)
    vec_div = lambda a, b, out: eng._chk(eng.lib().mi_vec_div(ctx.h, C.c_int64(n), eng._ptr(a), eng._ptr(b), eng._ptr(out)))
    vec_div(xd, yd, o)
    assert same(host(o), x / y)
    t = dev(x); vec_div(t, yd, t)
    assert same(host(t), x / y)
    # the weight passes: a flux of both signs with +0.0 and -0.0 (pos(0) = pos(-0) = 1)
    flux, cdw = signed_flux(u(10, n)), 0.3 + 0.4 * u(11, n)
    assert np.any(flux == 0.0) and (n < 4 or np.any(np.signbit(flux) & (flux == 0.0)))
    fd = dev(flux)
    asm.upwind_weights(fd, o)
    assert same(host(o), orc.upwind_weights(flux))
    asm.lust_weights(dev(cdw), fd, o)
    assert same(host(o), lust_weights(cdw, flux))
    # CoEuler's face rDeltaT, volumetric and mass flux: both branches of the max
    dc, mag_sf, phi, rho_f = 1.0 + u(30, n), 0.5 + u(31, n), 60.0 * signed_flux(u(32, n)), 0.7 + u(33, n)
    dcd, md, pd = dev(dc), dev(mag_sf), dev(phi)
    for rf in (None, rho_f):
        asm.co_face_r_delta_t(dcd, md, pd, 0.02, 0.5, o, rho_face=None if rf is None else dev(rf))
        want = co_face(dc, phi, mag_sf, 0.02, 0.5, rho_f=rf)
        assert same(host(o), want) and (n < 1000 or 0.2 * n < np.sum(want > 50.0) < 0.8 * n)
    # fvm::ddt / fvc::ddt with a cell field rDeltaT (localEuler, CoEuler): no density, constant density, density field
    r = 50.0 + 400.0 * u(12, n)
    rD = dev(r)
    d, s = E(n), E(n)
    for form in ("none", "constant", "field"):
        kw = dict(constant=dict(rho_value=1.3), field=dict(rho=rho, rho0=rho0)).get(form, {})
        ekw = dict(constant=dict(rho_value=1.3), field=dict(rho=rhod, rho_old=rho0d)).get(form, {})
        asm.fvm_ddt_local(rD, Vd, p0d, d, s, **ekw)
        rd, rs = local_fvm_ddt(r, V, p0, **kw)
        assert same(host(d), rd) and same(host(s), rs), form
        asm.fvc_ddt_local(rD, xd, p0d, o, **ekw)
        assert same(host(o), local_fvc_ddt(r, x, p0, **kw)), form
