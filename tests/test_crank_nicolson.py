"""`ddtSchemes { default CrankNicolson <oc>; }`: the ddt0 state, fvm::ddt, fvc::ddt and the fused assembly with the CrankNicolson time
derivative (CrankNicolsonDdtScheme.H:165-180, CrankNicolsonDdtScheme.C:186-267, 417-426, 507-516, 603-616, 755-1003; static mesh).

The expected values are a numpy restatement of the reference's field expressions written here: numpy evaluates one operator per pass and
rounds each (tests/test_backward_ddt.py explains why that is the reference's rounding), so every comparison with the engine is bit for bit.
CPU: the parser, the state sequence through the C ABI, the order of accuracy and the Euler limit of the restatement, the exports.  GPU: the
three streaming kernels, mi_fvm_assemble_cn against the engine's own unfused sequence and against the restatement in every block shape of
the row pass (with the Euler and backward calls on the same inputs), a six-step time loop with changing step sizes and a repeated assembly,
scalarTransportFoam with `default CrankNicolson 0.9`, and the mirror's fvc::ddt / fvc::ddtCorr from a small program of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_backward_ddt as bw
from assembly_support import SHAPES, VARIANTS, FusedCase, gpu_env
from test_backward_ddt import _close


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def off(oc, x):
    """offCentre_ (.C:250-267)"""
    return oc * x if oc < 1.0 else x


class State:
    """the DDt0Field's two time indices and the host scalars (.C:109-181, 186-247)"""

    def __init__(self, oc, time_index):
        self.oc, self.start, self.index = oc, time_index, time_index

    def scalars(self, time_index):
        coef = 1.0 + self.oc if time_index - self.start > 0 else 1.0
        coef0 = 1.0 + self.oc if time_index - self.start > 1 else 1.0
        return coef, coef0

    def step(self, time_index, dt, dt0):
        coef, coef0 = self.scalars(time_index)
        evaluate = self.index != time_index
        if evaluate:
            self.index = time_index
        return coef / dt, coef0 / dt0, evaluate


def ddt0_update(rdt0, oc, p0, p00, d, rho_value=None, rho0=None, rho00=None):
    """the ddt0 assignment of fvcDdt / fvmDdt (:417-418 no density, :507-508 constant, :603-607 field)"""
    if rho0 is not None:
        return (rdt0 * ((rho0 * p0) - (rho00 * p00))) - off(oc, d)
    c = rdt0 if rho_value is None else rdt0 * rho_value
    return (c * (p0 - p00)) - off(oc, d)


def fvm_ddt(rdt, oc, V, p0, d, rho_value=None, rho=None, rho0=None):
    """-> (diag, source) of fvmDdt (:755-832 no density, :837-913 constant, :919-1003 field); d: ddt0, already updated"""
    if rho is not None:
        return (rdt * rho) * V, (((rdt * rho0) * p0) + off(oc, d)) * V
    c = rdt if rho_value is None else rdt * rho_value
    return c * V, ((c * p0) + off(oc, d)) * V


def fvc_ddt(rdt, oc, f, f0, d, rho_value=None, rho=None, rho0=None):
    """fvcDdt (:426 no density, :516 constant, :615-616 field)"""
    if rho is not None:
        return (rdt * ((rho * f) - (rho0 * f0))) - off(oc, d)
    c = rdt if rho_value is None else rdt * rho_value
    return (c * (f - f0)) - off(oc, d)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_parser(pkg):
    eng = pkg.engine
    for text, oc in (("CrankNicolson 0.9", 0.9), ("CrankNicolson 1", 1.0), ("CrankNicolson 0", 0.0), ("  CrankNicolson\t0.5 ", 0.5)):
        assert eng.ddt_cn_parse(text) == oc, text
    for text, token in (("CrankNicolson", "CrankNicolson"), ("CrankNicolson 1.5", "1.5"), ("CrankNicolson -0.1", "-0.1"), ("CrankNicolson nan", "nan"),
                        ("CrankNicolson one", "one"), ("CrankNicolson 0.9 1", "'1'"), ("Euler", "Euler"), ("backward", "backward"), ("", "empty")):
        with pytest.raises(eng.MiError) as e:
            eng.ddt_cn_parse(text)
        assert token in str(e.value), (text, str(e.value))
    for text in ("CrankNicolson 1.5", "CrankNicolson -0.1"):
        with pytest.raises(eng.MiError, match="should be >= 0 and <= 1"):
            eng.ddt_cn_parse(text)
    oc = C.c_double()
    assert eng.lib().mi_ddt_cn_parse(None, C.byref(oc)) != 0 and eng.lib().mi_ddt_cn_parse(b"CrankNicolson 1", None) != 0


def test_state_sequence_through_the_c_abi(pkg):
    """mi_ddt_cn_begin / mi_ddt_cn_step: Euler on the step of first use, coef0 one step behind coef, evaluate once per time index"""
    eng = pkg.engine
    oc, dts = 0.9, [0.01, 0.01, 0.004, 0.008]
    want = [(1.0, 1.0, False), (1.9, 1.0, True), (1.9, 1.9, True), (1.9, 1.9, True)]
    for first in (1, 5):
        cn, ref = eng.CrankNicolson(oc, first), State(oc, first)
        assert cn.oc == oc and cn.state.start_time_index == first and cn.state.ddt0_time_index == first
        for k, dt in enumerate(dts):
            dt0 = dts[k - 1] if k else dts[0]
            assert (*ref.scalars(first + k), want[k][2]) == want[k]
            got = cn.step(first + k, dt, dt0)
            assert got == (want[k][0] / dt, want[k][1] / dt0, want[k][2]), (first, k, got)
            assert got == ref.step(first + k, dt, dt0)
            assert cn.state.ddt0_time_index == first + k and cn.state.start_time_index == first
            again = cn.step(first + k, dt, dt0)                       # non-orthogonal correctors: the same scalars, no second update
            assert again == (got[0], got[1], False), (first, k, again)
    cn = eng.CrankNicolson(oc, 1)
    for bad in (lambda: cn.step(1, 0.0, 0.01), lambda: cn.step(1, -0.01, 0.01), lambda: cn.step(2, 0.01, 0.0), lambda: cn.step(2, 0.01, -1.0),
                lambda: eng.CrankNicolson(1.5, 1), lambda: eng.CrankNicolson(-0.1, 1), lambda: eng.CrankNicolson(float("nan"), 1)):
        with pytest.raises(eng.MiError):
            bad()
    assert cn.state.ddt0_time_index == 1                              # a refused step leaves the state alone
    assert cn.step(1, 0.01, 0.0) == (100.0, 0.0, False)               # delta_t0 is read only when evaluate is set
    assert cn.step(1, 0.01, -1.0)[2] is False
    assert cn.step(2, 0.01, 0.01) == (1.9 / 0.01, 1.0 / 0.01, True)


def _decay_error(steps, oc):
    """dT/dt = -2 T, T(0) = 1, one cell of volume 0.37, Sp as V*k on the diagonal, to t = 1: the set-up of
    tests/test_backward_ddt.py::test_restated_fvm_ddt_is_second_order_and_euler_first, with the ddt0 state carried along"""
    V, k = np.array([0.37]), 2.0
    dt = 1.0 / steps
    T0 = T00 = np.array([1.0])
    st, d0 = State(oc, 1), np.zeros(1)
    pairs = []
    for s in range(1, steps + 1):
        rdt, rdt0, evaluate = st.step(s, dt, dt)
        if evaluate:
            d0 = ddt0_update(rdt0, oc, T0, T00, d0)
        d, src = fvm_ddt(rdt, oc, V, T0, d0)
        pairs.append((d, src, (1.0 / dt) * V, ((1.0 / dt) * T0) * V))
        T = src / (d + V * k)
        T00, T0 = T0, T
    return abs(T0[0] - np.exp(-2.0)), pairs


def test_restatement_is_second_order_at_oc_1_and_euler_at_oc_0():
    e = [_decay_error(s, 1.0)[0] for s in (20, 40, 80, 160)]
    for a, b in zip(e, e[1:]):
        assert 3.8 <= a / b <= 4.1, e
    for d, src, de, se in _decay_error(40, 0.0)[1]:
        assert np.array_equal(d, de) and np.array_equal(src, se)


def test_exports(pkg):
    from test_polymesh import PKG
    eng = pkg.engine
    names = ["mi_ddt_cn_parse", "mi_ddt_cn_begin", "mi_ddt_cn_step", "mi_ddt_cn_update", "mi_fvm_ddt_cn", "mi_fvc_ddt_cn", "mi_fvm_assemble_cn"]
    for name in names:
        assert name in eng.SYMBOLS and hasattr(eng.lib(), name), name
    out = subprocess.run(["nm", "-D", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    assert "Foam::fv::CrankNicolsonDdtScheme::New(" in out and "Foam::fv::CrankNicolsonDdtScheme::assemble(" in out
    assert "Foam::fvm::ddt(Foam::fvScalarMatrix&, Foam::fv::CrankNicolsonDdtScheme&" in out
    assert "Foam::fvc::ddt(Foam::gpuList<double>&, Foam::fv::CrankNicolsonDdtScheme&" in out
    assert "Foam::fvc::ddtCorr(Foam::gpuList<double>&, Foam::lduAddressing const&, Foam::fv::CrankNicolsonDdtScheme&" in out
    assert "Foam::fv::CrankNicolsonDdtScheme::evaluate(" in out and "Foam::fv::CrankNicolsonDdtScheme::rDtCoef(" in out


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
OCS = [1.0, 0.9, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 1027, 31 * 23 * 19, 1050625, 5243907])
def test_streaming_kernels_against_the_restatement(pkg, n):
    """mi_ddt_cn_update (one and three fields, in place) / mi_fvm_ddt_cn / mi_fvc_ddt_cn: the three density forms x three off-centring
    coefficients; sizes with an odd tail and an unpaired element of the double2 loop"""
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg)
    u = pkg.synthetic.splitmix_uniform
    case = pkg.synthetic.box_case(2, 2, 2)
    asm = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
    V, p = 0.5 + u(1, n), u(2, n) - 0.5
    p0, p00, d0 = [u(3 + k, n) - 0.5 for k in range(3)], [u(6 + k, n) - 0.5 for k in range(3)], [40.0 * (u(9 + k, n) - 0.5) for k in range(3)]
    rho, rho0, rho00 = 0.9 + u(15, n), 0.8 + u(16, n), 0.7 + u(17, n)
    d, s, o = E(n), E(n), E(n)
    rdt, rdt0 = 1.9 / 0.004, 1.9 / 0.01
    for oc in OCS:
        for form in ("none", "constant", "field"):
            kw = dict(constant=dict(rho_value=1.3), field=dict(rho=rho, rho0=rho0)).get(form, {})
            ukw = dict(constant=dict(rho_value=1.3), field=dict(rho0=rho0, rho00=rho00)).get(form, {})
            ekw = dict(constant=dict(rho_value=1.3), field=dict(rho=dev(rho), rho_old=dev(rho0))).get(form, {})
            eukw = dict(constant=dict(rho_value=1.3), field=dict(rho_old=dev(rho0), rho_old_old=dev(rho00))).get(form, {})
            for k in (1, 3):
                io = [dev(x) for x in d0[:k]]
                asm.ddt_cn_update(rdt0, oc, [dev(x) for x in p0[:k]], [dev(x) for x in p00[:k]], io, **eukw)
                for j in range(k):
                    assert np.array_equal(host(io[j]), ddt0_update(rdt0, oc, p0[j], p00[j], d0[j], **ukw)), (form, oc, k, j)
            asm.fvm_ddt_cn(rdt, oc, dev(V), dev(p0[0]), dev(d0[0]), d, s, **ekw)
            rd, rs = fvm_ddt(rdt, oc, V, p0[0], d0[0], **kw)
            assert np.array_equal(host(d), rd) and np.array_equal(host(s), rs), (form, oc)
            asm.fvc_ddt_cn(rdt, oc, dev(p), dev(p0[0]), dev(d0[0]), o, **ekw)
            assert np.array_equal(host(o), fvc_ddt(rdt, oc, p, p0[0], d0[0], **kw)), (form, oc)
    if n != 1027:
        return
    # refusals: a missing array, an unaligned array, an output among the inputs or twice, one density array of two, oc outside [0, 1]
    Vd, pd, p0d, p00d, dd, rd_ = dev(V), dev(p), dev(p0[0]), dev(p00[0]), dev(d0[0]), dev(rho)
    odd = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")[1:]
    assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    for bad in (lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, None, d, s), lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, None, s),
                lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, odd, s), lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, odd, dd, d, s),
                lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, p0d, s), lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, d, dd),
                lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, d, d), lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, d, s, rho=rd_),
                lambda: asm.fvm_ddt_cn(rdt, 0.9, Vd, p0d, dd, d, s, rho_old=rd_), lambda: asm.fvm_ddt_cn(rdt, 1.5, Vd, p0d, dd, d, s),
                lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, p0d, dd, dd), lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, p0d, dd, pd),
                lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, p0d, None, o), lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, None, dd, o),
                lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, p0d, dd, odd), lambda: asm.fvc_ddt_cn(rdt, 0.9, pd, p0d, dd, o, rho_old=rd_),
                lambda: asm.fvc_ddt_cn(rdt, -0.1, pd, p0d, dd, o),
                lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [p00d], [p0d]), lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [p00d], [None]),
                lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [None], [dd]), lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [p00d], [odd]),
                lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d, p0d], [p00d, p00d], [dd, dd]), lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [p00d], [dd], rho_old=rd_),
                lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d], [p00d], [dd], rho_old_old=rd_), lambda: asm.ddt_cn_update(rdt0, 2.0, [p0d], [p00d], [dd]),
                lambda: asm.ddt_cn_update(rdt0, 0.9, [p0d] * 5, [p00d] * 5, [E(n) for _ in range(5)]), lambda: asm.ddt_cn_update(rdt0, 0.9, [], [], [])):
        with pytest.raises(eng.MiError):
            bad()
    assert np.array_equal(host(dd), d0[0])                            # no refused call wrote


# ---- the fused assembly ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,tables", SHAPES)
def test_fused_cn_assembly_bit_for_bit(pkg, orc, monkeypatch, name, mode, tables):
    """mi_fvm_assemble_cn against (a) the engine's own unfused sequence -- mi_fvm_ddt_cn, mi_fvm_div, mi_fvm_laplacian, mi_fvm_su / Sp, the
    mi_vec_axpby combinations, in the order of tests/assembly_support.py::unfused_sequence -- and (b) the restatement; and on the same inputs
    the Euler call (no `crank_nicolson` key) and the backward call against their own unfused sequences."""
    F = FusedCase(pkg, orc, monkeypatch, name, mode, tables)
    eng, dev, host, E, A, addr, q = F.eng, F.dev, F.host, F.E, F.A, F.addr, F.q
    n, nf, vol, flux, lap = F.n, F.nf, F.vol, F.flux, F.lap
    u = pkg.synthetic.splitmix_uniform
    ddt0 = [40.0 * (u(181 + k, n) - 0.5) for k in range(3)]
    rdt, rdt_e = 1.9 / 0.004, 1.0 / 0.004                                  # rDtCoef of the CN call; Euler's and backward's rDeltaT
    cb = bw.coeffs(0.004, 0.01)
    for vi, v in enumerate(VARIANTS):
        if v["corr"] and name != "box":
            continue
        oc = OCS[vi % 3]                                                    # 1.0, 0.9, 0.0, 1.0, 0.9 over the five variants
        V = F.variant(v)
        cn = dict(oc=oc, ddt0=[dev(x) for x in ddt0[:V.R]])
        rkw = dict(rho=q["rho"], rho0=q["rho0"]) if v["field"] else dict(rho_value=1.2)
        got = V.fused(dict(V.ddt, r_delta_t=rdt, crank_nicolson=cn))
        seq = V.unfused(lambda r, dd, ds: A.fvm_ddt_cn(rdt, oc, vol, V.psi_old[r], cn["ddt0"][r], dd, ds, **V.rho))
        V.assert_same(got, seq, "cn")
        for r in range(V.R):
            assert np.array_equal(host(cn["ddt0"][r]), ddt0[r])                 # an input only
        V.assert_restated(got, seq, lambda r: fvm_ddt(rdt, oc, q["vol"], q["psi0"][r], ddt0[r], **rkw))
        # Euler and backward untouched: the same call without the `crank_nicolson` key, and with the `backward` key
        eul = V.fused(dict(V.ddt, r_delta_t=rdt_e))
        V.assert_same(eul, V.unfused(V.euler(rdt_e)), "euler")
        bwd = V.fused(dict(V.ddt, r_delta_t=rdt_e, backward=bw.backward_arg(V, cb)))
        V.assert_same(bwd, V.unfused(bw.backward_ddt_call(V, rdt_e, cb)), "backward")
        for r in range(V.R):
            assert not np.array_equal(host(eul["src"][r]), host(got["src"][r])) and not np.array_equal(host(bwd["src"][r]), host(got["src"][r]))
    # refusals of the CrankNicolson entry point
    ddt = dict(r_delta_t=rdt, vol=vol, psi_old=[dev(q["psi0"][0])])
    d0, p00 = dev(ddt0[0]), dev(q["psi00"][0])
    o = dict(lower=E(nf), upper=E(nf), diag=E(n), src=[E(n)])
    call = lambda d: A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=d, div=dict(flux=flux), laplacian=lap)
    call(dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[d0])))
    for bad in (dict(vol=vol, crank_nicolson=dict(oc=0.9, ddt0=[d0])),                                       # terms->ddt == 0
                dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[None])),                                         # a missing ddt0 array
                dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[o["src"][0]])),                                  # a ddt0 array among the outputs
                dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[o["diag"]])),
                dict(ddt, crank_nicolson=dict(oc=1.5, ddt0=[d0])),                                           # oc outside [0, 1]
                dict(ddt, rho=dev(q["rho"]), crank_nicolson=dict(oc=0.9, ddt0=[d0])),                        # rho without rho_old (mi_fvm_assemble's)
                dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[d0]), backward=dict(coeffs=cb, psi_old_old=[p00]))):   # both schemes
        with pytest.raises(eng.MiError):
            call(bad)
    with pytest.raises(eng.MiError):                                                                         # a coefficient output aliasing an input
        A.assemble(flux, o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[d0])), div=dict(flux=flux))
    with pytest.raises(eng.MiError):                                                                         # no face term at all
        A.assemble(o["upper"], o["diag"], sources_out=o["src"], ddt=dict(ddt, crank_nicolson=dict(oc=0.9, ddt0=[d0])))
    t = eng.FvmTerms()
    assert eng.lib().mi_fvm_assemble_cn(addr.h, C.byref(t), None, None, None, None, None, None, None) != 0   # cn NULL


# ---- the statements of scalarTransportFoam walked with the restatement ----------------------------------------------------------------
class CrankNicolsonDdt:
    """the time scheme object of tests/transport_walk.py::walk: fvm::ddt(T) by the restatement and its state -- the old-old field, the ddt0 field
    created zero at the first step's time index and updated once per step, by the step's first assembly only"""

    def __init__(self, oc):
        self.oc, self.st = oc, State(oc, 1)

    def start_step(self, step, dts, Told):
        if step == 0:
            self.d0 = np.zeros(len(Told))
        self.Too = Told.copy() if step == 0 else self.Told
        self.Told, self.step, self.dt, self.dt0 = Told, step, dts[step], dts[step - 1] if step else dts[step]

    def assemble(self, V, non_orth, rep):
        rdt, rdt0, evaluate = self.st.step(self.step + 1, self.dt, self.dt0)
        assert evaluate == (self.step > 0 and non_orth == 0 and rep == 0)
        if evaluate:
            self.d0 = ddt0_update(rdt0, self.oc, self.Told, self.Too, self.d0)
        return fvm_ddt(rdt, self.oc, V, self.Told, self.d0)

    def state(self):
        return dict(ddt0=self.d0.copy())


def walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme, corrected, n_non_orth, oc=None, repeat_at=()):
    """tests/transport_walk.py::walk with the ddt line by the restatement and its state, one step size per step.  oc None: Euler.  repeat_at:
    steps whose first assembly is formed twice (the second must see the same ddt0).  -> solver lines, T, mesh data, per step the assembled
    system and ddt0"""
    import transport_walk
    w = transport_walk.walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme, "corrected" if corrected else None, n_non_orth,
                            ddt=None if oc is None else CrankNicolsonDdt(oc), repeat_at=repeat_at)
    return w.lines, w.T, w.mesh, w.systems


@pytest.fixture(scope="module")
def loop_case(pkg, orc):
    """the 12 x 8 x 6 box of the time loop and its Euler walk, computed once"""
    from test_polymesh import make_box_mesh
    mesh = make_box_mesh((12, 8, 6), seed=None)
    cnt_in = [pt[2] for pt in mesh[4] if pt[0] == "inlet"][0]
    tin = 1.0 + 0.5 * np.sin(np.arange(cnt_in))
    n = int(mesh[2].max()) + 1
    dts = [0.01, 0.01, 0.004, 0.008, 0.008, 0.01]
    euler = walk(pkg, orc, *mesh, tin, np.zeros(n), 0.01, dts, "linear", False, 0)
    return dict(mesh=mesh, tin=tin, n=n, dts=dts, DT=0.01, euler=euler)


@pytest.mark.gpu
@pytest.mark.parametrize("oc", [0.9, 1.0, 0.0])
def test_time_loop_with_changing_step_sizes(pkg, orc, loop_case, oc):
    """six steps of ddt(T) + div(phi,T) - laplacian(DT,T) through Python: the state object, the evaluate-once update, the fused assembly,
    PBiCG + DILU, against the same statements walked with the restatement and the oracle's PBiCG; steps 2 and 4 assemble twice.  oc 0: the
    assembled arrays are the Euler assembly's."""
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg)
    L = loop_case
    DT, dts, n = L["DT"], L["dts"], L["n"]
    repeat_at = (2, 4)
    ref_lines, Tref, M, systems = walk(pkg, orc, *L["mesh"], L["tin"], np.zeros(n), DT, dts, "linear", False, 0, oc=oc, repeat_at=repeat_at)
    elines, Teuler, _, esystems = L["euler"]
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
    ref, d0 = State(oc, 1), np.zeros(n)                                    # the restated state, on the fields each step starts from
    el, eu, ed, es = E(nI), E(nI), E(n), E(n)
    cn, ddt0 = eng.CrankNicolson(oc, 1), torch.zeros(n, dtype=torch.float64, device="cuda:0")      # created zero at the first step's time index
    Too = None
    for step, dt in enumerate(dts):
        Told = T.clone()
        if step == 0:
            Too = Told.clone()
        for rep in range(2 if step in repeat_at else 1):
            rdt, rdt0, evaluate = cn.step(step + 1, dt, dts[step - 1] if step else dt)
            assert evaluate == (step > 0 and rep == 0), (step, rep)
            assert (rdt, rdt0, evaluate) == ref.step(step + 1, dt, dts[step - 1] if step else dt)
            if evaluate:
                A.ddt_cn_update(rdt0, oc, [Told], [Too], [ddt0])
                d0 = ddt0_update(rdt0, oc, host(Told), host(Too), d0)
            A.assemble(upper, diag, lower_out=lower, sources_out=[src], ddt=dict(r_delta_t=rdt, vol=V, psi_old=[Told], crank_nicolson=dict(oc=oc, ddt0=[ddt0])),
                       div=dict(flux=phi, weights=lam), laplacian=lap)
            dD, sD = fvm_ddt(rdt, oc, G["V"], host(Told), d0)
            assert np.array_equal(host(ddt0), d0), (step, rep)                  # the second assembly of a step sees an unchanged ddt0
            assert np.array_equal(host(lower), lB - uL) and np.array_equal(host(upper), uB - uL), (step, rep)
            assert np.array_equal(host(diag), (dD + dB) - dL) and np.array_equal(host(src), sD), (step, rep)
        if oc == 0.0:
            A.assemble(eu, ed, lower_out=el, sources_out=[es], ddt=dict(r_delta_t=1.0 / dt, vol=V, psi_old=[Told]), div=dict(flux=phi, weights=lam), laplacian=lap)
            for got, e in ((lower, el), (upper, eu), (diag, ed), (src, es)):
                assert np.array_equal(host(got), host(e)), step
        for p, ic, bc in patch:
            p.add(ic, diag, 0); p.add(bc, src, 0)
        mat.set_coeffs(diag, upper, lower)
        perf = mat.pbicg(T, src, "DILU", tolerance=1e-10, relTol=0.0)
        r = ref_lines[step]
        assert _close((perf["initialResidual"], perf["finalResidual"], perf["nIterations"]), r[2:]), (step, perf, r)
        Too = Told
    Tg = host(T)
    assert np.max(np.abs(Tg - Tref)) <= 1e-8 * np.max(np.abs(Tref))
    assert 0.05 < np.max(Tref) < 2.0
    if oc == 0.0:
        assert np.max(np.abs(Tref - Teuler)) <= 1e-8 * np.max(np.abs(Tref))      # the Euler walk: the same arrays every step
    else:
        assert np.max(np.abs(Tref - Teuler)) > 1e-5 * np.max(np.abs(Tref))       # the scheme is not a no-op
        assert np.any(systems[2]["ddt0"] != 0.0) and not np.any(systems[0]["ddt0"] != 0.0)


def _channel(tmp_path, dims, n_steps, scheme, corrected, n_non_orth, ddt_entry):
    from test_scalartransportfoam import write_channel
    from transport_walk import rewrite_schemes
    case_dir = str(tmp_path / "channel")
    made = write_channel(case_dir, dims, 0.01, 0.01, n_steps, scheme, corrected, n_non_orth)
    rewrite_schemes(case_dir, ("ddtSchemes { default Euler; }", "ddtSchemes { default %s; }" % ddt_entry))
    return case_dir, made


@pytest.mark.gpu
@pytest.mark.parametrize("dims, n_steps, scheme, corrected, n_non_orth", [((12, 8, 6), 4, "upwind", False, 0), ((12, 9, 7), 3, "linear", True, 2)])
def test_scalarTransportFoam_with_the_crank_nicolson_scheme(pkg, orc, tmp_path, dims, n_steps, scheme, corrected, n_non_orth):
    """the application with `ddtSchemes { default CrankNicolson 0.9; }`: T.oldTime().oldTime() kept, ddt0(T) owned by the scheme object and
    updated by the first corrector's assembly only; every solver line and the written T against the walk, with the comparisons of
    tests/test_backward_ddt.py::test_scalarTransportFoam_with_the_backward_scheme"""
    from test_polymesh import PKG, read_vol_field
    from transport_walk import assert_solver_lines, solver_lines
    DT, delta_t = 0.01, 0.01
    case_dir, (pts, faces, owner, neighbour, patches, tin, T0) = _channel(tmp_path, dims, n_steps, scheme, corrected, n_non_orth, "CrankNicolson 0.9")
    ref, Tref, _, _ = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, [delta_t] * n_steps, scheme, corrected, n_non_orth, oc=0.9)
    _, Teuler, _, _ = walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, [delta_t] * n_steps, scheme, corrected, n_non_orth)
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


@pytest.mark.gpu
def test_scalarTransportFoam_refuses_crank_nicolson_without_a_coefficient(pkg, tmp_path):
    from test_polymesh import PKG
    case_dir, _ = _channel(tmp_path, (12, 8, 6), 1, "upwind", False, 0, "CrankNicolson")
    out = subprocess.run([os.path.join(PKG, "scalarTransportFoam"), case_dir], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "CrankNicolson" in out.stderr + out.stdout and "coefficient" in out.stderr + out.stdout, out.stderr + out.stdout[-800:]


MIRROR_PROGRAM = r'''
#include "miFoam.H"
#include <cstdio>
using namespace Foam;
// three time steps of fvc::ddt(T) (twice per step) and fvc::ddtCorr(U, phi) through fv::CrankNicolsonDdtScheme; every double printed as %a
static std::vector<double> field(int s, int n, int salt) { std::vector<double> v(n); for (int i = 0; i < n; ++i) v[i] = ((i * 7 + s * 13 + salt) % 11) / 8.0 - 0.5 + s * 0.125; return v; }
static void print(const char* tag, int s, const scalargpuField& f) { std::printf("%s %d", tag, s); for (double x : f.asHost()) std::printf(" %a", x); std::printf("\n"); }
int main()
{
    try {
        const int n = 7; const double oc = 0.9, dts[3] = {0.01, 0.004, 0.008};
        fv::CrankNicolsonDdtScheme cn = fv::CrankNicolsonDdtScheme::New("CrankNicolson 0.9");
        labelList lo(n - 1), up(n - 1); for (int i = 0; i < n - 1; ++i) { lo[i] = i; up[i] = i + 1; }
        lduAddressing addr(n, lo, up);
        scalargpuField w(field(0, n - 1, 3)), phiOld(field(1, n - 1, 5)), out(n), again(n), corr(n - 1), corrE(n - 1);
        vectorgpuField Sf(n - 1), Uold(n);
        for (int d = 0; d < 3; ++d) { Sf.component(d) = field(2, n - 1, d); Uold.component(d) = field(3, n, d); }
        const word name = fv::CrankNicolsonDdtScheme::ddt0Name("T");
        for (int s = 1; s <= 3; ++s) {
            cn.setTime(s, dts[s - 1], s > 1 ? dts[s - 2] : dts[0]);
            const scalargpuField vf(field(s, n, 0)), vf0(field(s - 1, n, 0)), vf00(field(s > 1 ? s - 2 : 0, n, 0));
            fvc::ddt(out, cn, name, vf, vf0, vf00);
            print("ddt", s, out); print("ddt0", s, cn.ddt0(name));
            fvc::ddt(again, cn, name, vf, vf0, vf00);                       // the same time step: ddt0 is not updated again
            print("again", s, again); print("ddt0again", s, cn.ddt0(name));
            const word nameU = fv::CrankNicolsonDdtScheme::ddt0Name("U");
            std::printf("rDtCoef %d %a\n", s, cn.rDtCoef(nameU, n, 3));
            fvc::ddtCorr(corr, addr, cn, nameU, w, Sf, Uold, phiOld);
            fvc::ddtCorr(corrE, addr, (s > 1 ? 1.0 + oc : 1.0) / dts[s - 1], w, Sf, Uold, phiOld);   // Euler's call with rDtCoef
            std::printf("ddtCorr %d %d\n", s, (int)(corr.asHost() == corrE.asHost()));
            for (direction d = 0; d < 3; ++d) for (double x : cn.ddt0(nameU, d).asHost()) if (x != 0.0) std::printf("ddt0(U) touched\n");
        }
        const scalargpuField a(field(1, n, 0)); const scalargpuField* p[1] = {&a};
        for (int bad : {0, 5}) { try { cn.evaluate("ddt0(X)", 1.0, p, p, bad); std::printf("accepted %d\n", bad); } catch (const error&) { std::printf("refused %d\n", bad); } }
    } catch (const std::exception& e) { std::printf("FAILED %s\n", e.what()); return 1; }
    return 0;
}
'''


@pytest.mark.gpu
def test_mirror_fvc_ddt_and_ddt_corr_through_the_scheme_object(pkg, tmp_path):
    """the mirror's fv::CrankNicolsonDdtScheme from a small program of its own: fvc::ddt over three steps with changing step sizes against
    the restatement bit for bit, twice per step (one update per step); fvc::ddtCorr is Euler's call with rDtCoef of ddt0(U), which it neither
    reads nor updates; a component count outside 1..4 is refused"""
    from test_polymesh import PKG
    src, exe = tmp_path / "cn.C", tmp_path / "cn"
    src.write_text(MIRROR_PROGRAM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "foam"), "-I", os.path.join(os.path.dirname(PKG), "include"), str(src), "-o", str(exe),
                    "-L" + PKG, "-lmiFoam", "-lrapidcfd_amd", "-Wl,-rpath," + PKG], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] in ("ddt", "ddt0", "again", "ddt0again", "rDtCoef"):
            got[(w[0], int(w[1]))] = np.array([float.fromhex(x) for x in w[2:]])
    n, oc, dts = 7, 0.9, [0.01, 0.004, 0.008]
    field = lambda s: np.array([((i * 7 + s * 13) % 11) / 8.0 - 0.5 + s * 0.125 for i in range(n)])
    st, d0 = State(oc, 1), np.zeros(n)
    for s in (1, 2, 3):
        rdt, rdt0, evaluate = st.step(s, dts[s - 1], dts[s - 2] if s > 1 else dts[0])
        if evaluate:
            d0 = ddt0_update(rdt0, oc, field(s - 1), field(s - 2 if s > 1 else 0), d0)
        want = fvc_ddt(rdt, oc, field(s), field(s - 1), d0)
        for a, b in (("ddt", "ddt0"), ("again", "ddt0again")):
            assert np.array_equal(got[(a, s)], want) and np.array_equal(got[(b, s)], d0), (a, s)
        assert got[("rDtCoef", s)][0] == rdt, s
        assert f"ddtCorr {s} 1" in out.stdout, out.stdout
    assert np.any(d0 != 0.0) and "touched" not in out.stdout
    assert "refused 0" in out.stdout and "refused 5" in out.stdout and "accepted" not in out.stdout
