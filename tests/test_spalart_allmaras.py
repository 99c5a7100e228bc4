"""The Spalart-Allmaras block on the device (RAS, DES, DDES, IDDES and nutUSpaldingWallFunction): mi_sa_coeffs_init, mi_sa_terms, mi_sa_nut and
mi_sa_nut_spalding_wall, bit for bit against the restatement of tests/spalart_support.py continued from the device's pow / tanh / exp values,
each of which is held to numpy's on the same argument."""
import os
import re

import numpy as np
import pytest

import spalart_support as S
from assembly_support import bits, gpu_env, same, set_face_grid
from turbulence_support import ALL_MESHES, BIG, boundary_cells, mesh, wall_mask, wall_tables

EXPORTS = ("mi_sa_coeffs_init", "mi_sa_terms", "mi_sa_nut", "mi_sa_nut_spalding_wall")
NAN = float("nan")
SEED = {"box": 7000, "edge_257": 7100, "isolated": 7200, BIG: 7300}
VARIANTS = [(kind, ash) for kind in S.KINDS for ash in (True, False)]
_CACHE, _REST = {}, {}


def same_n(a, b):
    """bit for bit, signed zeros included; a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def _case(pkg, name):
    """the mesh and its inputs, computed once and left unchanged"""
    if name not in _CACHE:
        L = mesh(pkg, name)
        Ke = pkg.engine.sa_coeffs()                               # the library's coefficients, shown equal to S.coeffs() by test_coefficients
        K = {m: getattr(Ke, m) for m in S.MODEL + S.WALL + S.DERIVED}
        assert K == S.coeffs()
        _CACHE[name] = dict(L=L, F=S.inputs(pkg.synthetic, L, SEED[name]), K=K)
    return _CACHE[name]


def _restated(pkg, name, kind, ash, nu_key="nu", cont=None):
    """the restatement of one variant, once per (mesh, kind, Ashford, nu, the library values it continues from)"""
    key = (name, kind, ash, nu_key, None if cont is None else tuple(sorted((k, np.asarray(v).tobytes()) for k, v in cont.items())))
    if key not in _REST:
        c = _case(pkg, name)
        _REST[key] = S.restate_terms(c["K"], kind, ash, c["F"], nu=c["F"][nu_key], cont=cont)
    return _REST[key]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    lib = pkg.engine.lib()
    header = open(os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "..", "include", "mi_ldu.h")).read()
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in pkg.engine.SYMBOLS
    for word in ("SpalartAllmaras", "SpalartAllmarasDDES", "SpalartAllmarasIDDES", "nutUSpalding", "mi_sa_coeffs", "DESIGN 3.5t"):
        assert word in header, word
    assert pkg.engine.SA_KINDS == dict(RAS=0, DES=1, DDES=2, IDDES=3)
    for k, v in pkg.engine.SA_KINDS.items():
        assert re.search(r"#define MI_SA_%s %d\b" % (k, v), header)


def test_coefficients(pkg):
    """the defaults are the reference's, the derived members the literal host formulas in the reference's operand order; regrouped, Cw1 is
    another number, psiCoeff and Cv1_3 are not on the defaults (stated here, not assumed); a member that is not finite or not above zero is
    refused"""
    eng = pkg.engine
    K, W = eng.sa_coeffs(), S.coeffs()
    assert tuple(getattr(K, m) for m in S.MODEL) == S.MODEL_DEFAULTS == (0.66666, 0.41, 0.1355, 0.622, 0.3, 2.0, 7.1, 5.0, 0.65, 0.07, 0.424, 3.55, 1.63)
    assert (K.wallKappa, K.E) == S.WALL_DEFAULTS == (0.41, 9.8)
    assert eng.SA_MODEL == S.MODEL and eng.SA_WALL == S.WALL and eng.SA_DERIVED == S.DERIVED
    for m in S.DERIVED:
        assert getattr(K, m) == W[m], m
    assert K.Cw1 == 0.1355 / (0.41 * 0.41) + (1.0 + 0.622) / 0.66666 and K.psiCoeff == 0.1355 / ((K.Cw1 * (0.41 * 0.41)) * 0.424)
    assert K.invE == 1 / 9.8 and K.sqrt2 == 2.0 ** 0.5 and K.Cv1_3 == 7.1 * (7.1 * 7.1) and K.Cw3_6 == 64.0 and K.onePlusCw3_6 == 65.0
    given = dict(sigmaNut=0.7, kappa=0.4, Cb1=0.14, Cb2=0.6, Cw2=0.31, Cw3=2.1, Cv1=7.0, Cv2=4.9, CDES=0.6, ck=0.08, fwStar=0.4, cl=3.5, ct=1.6, wallKappa=0.4187,
                 E=9.793)
    K2, W2 = eng.sa_coeffs(**given), S.coeffs(**given)
    for m in S.MODEL + S.WALL + S.DERIVED:
        assert getattr(K2, m) == W2[m], m
    # regroupings of the host-formed products on the defaults: Cw1 over a common denominator is another number; Cb1/((Cw1*sqr(kappa))*fwStar)
    # and pow3(Cv1) happen to survive their regroupings on these values, which is why they are formed once and not left to the expression
    k2 = 0.41 * 0.41
    assert K.Cw1 != (0.1355 * 0.66666 + (1.0 + 0.622) * k2) / (k2 * 0.66666)
    assert K.psiCoeff == 0.1355 / (K.Cw1 * (k2 * 0.424)) and K.Cv1_3 == (7.1 * 7.1) * 7.1
    for name in S.MODEL + S.WALL:
        for bad in (0.0, -1.0, NAN, float("inf")):
            with pytest.raises(eng.MiError, match="above zero"):
                eng.sa_coeffs(**{name: bad})
    with pytest.raises(TypeError):
        eng.sa_coeffs(Cw1=3.0)


@pytest.mark.parametrize("name", ALL_MESHES)
def test_restatement_equals_the_literal_loops_and_the_inputs_reach_every_arm(pkg, name):
    """both restatements agree bit for bit for every kind, with and without the Ashford correction, nu a number and a cell array; every arm
    that positive inputs can reach is taken on both sides: by at least 5 % of the cells of the 1 200-cell box, by at least one cell elsewhere.
    Arms that positive inputs cannot reach: the ROOTVSMALL of r and rd decides only where max(S, SMALL)*sqr(kappa*d) < 1e-134, that is
    d < 1e-59 (shown on hand-made cells in test_each_stated_rounding_changes_a_compared_bit); the outer max(., SMALL) of the DDES and IDDES
    dTilda needs y < 1e-15; max(0.0, ut) of the wall functor needs a negative Newton iterate, which ends the loop first (ut > ROOTVSMALL)."""
    c = _case(pkg, name)
    F, K = c["F"], c["K"]
    share = 0.05 if name == BIG else 0.0
    for kind, ash in VARIANTS:
        for nu_key in ("nu", "nu_f"):
            R = _restated(pkg, name, kind, ash, nu_key)
            lit = S.literal_terms(K, kind, ash, F, {t: R[t] for t in S.TRANSCENDENTALS[kind]}, nu=F[nu_key])
            for key in S.OUTPUTS:
                assert same_n(lit[key], R[key]), (kind, ash, nu_key, key)
                assert np.all(np.isfinite(R[key])), (kind, ash, nu_key, key)
        R = _restated(pkg, name, kind, ash)
        arms = S.arms_of(kind, ash)
        for arm in arms:
            m = R[arm]
            if arm == "arm_fv1_small":      # max(SMALL, fv1) with fv1 == 0: the SMALL side is the nuTilda == 0 cells
                assert np.array_equal(m, F["nt"] == 0.0)
            lo = max(1, int(np.ceil(share * m.shape[0])))
            assert m.sum() >= lo and (~m).sum() >= lo, (name, kind, ash, arm, int(m.sum()), m.shape[0])
        for key in ("arm_fd_low", "arm_fd_high"):
            if key in R:
                assert not np.any(R["arm_fd_low"] & R["arm_fd_high"])
    # max(STilda, SMALL): without Ashford a negative fv2 makes STilda negative; with it STilda == 0 where nuTilda == 0 and gradU == 0
    Rn, Ra = _restated(pkg, name, "RAS", False), _restated(pkg, name, "RAS", True)
    assert np.any(Rn["stilda"] < 0) and np.any(Rn["fv2"] < 0) and np.all(Ra["fv2"] > 0)
    quiet = (F["nt"] == 0.0) & (F["grad"][1] == 0.0)
    assert np.any(quiet) and np.all(Ra["stilda"][quiet] == 0.0) and np.all(Ra["arm_st_small"][quiet])
    assert np.all(Ra["fv1"][F["nt"] == 0.0] == 0.0) and np.all(Ra["sp"][F["nt"] == 0.0] == 0.0)
    # mi_sa_nut's two forms agree where fv1 is the same array
    nut, fv1 = S.restate_nut(K, F["nt"], nu=F["nu"])
    assert same_n(fv1, Ra["fv1"]) and same_n(S.restate_nut(K, F["nt"], fv1=Ra["fv1"])[0], nut)


def _hand_made():
    """four cells at y = 1e-80 with nuTilda = 1e-170: max(STilda, SMALL)*sqr(kappa*y) is about 1e-170, far below ROOTVSMALL"""
    n = 4
    z = np.zeros(n)
    return dict(nt=np.full(n, 1e-170) * np.array([1.0, 2.0, 3.0, 4.0]), grad=[z.copy() for _ in range(9)], gnt=[z.copy() for _ in range(3)], y=np.full(n, 1e-80),
                nu=1e-5, delta=np.full(n, 1e-2), nusgs=np.full(n, 1e-5), hmax=np.full(n, 1e-2))


def test_each_stated_rounding_changes_a_compared_bit(pkg):
    """Undone one at a time on the 1 200-cell box, each stated rounding changes a compared bit: the contraction of magSqr(skew(gradU))
    (assumption 1 of 3.5t) and of magSqr(grad(nuTilda)); the RAS / LES forms of fv2, of chi/Cv2 and of fv3*sqrt(2.0)*mag; the host-formed
    Cb2/sigmaNut, Cb1/psiDen and (Cw1*fw)*nuTilda regrouped inside the expression; the equation's two additions against V*(a + b); the
    contracted wall functor (assumption 2).  The ROOTVSMALL of r changes nothing on positive inputs of ordinary size and changes r on the
    hand-made cells of _hand_made()."""
    c = _case(pkg, BIG)
    F, K, L = c["F"], c["K"], c["L"]
    differs = lambda kind, ash, alt, key: not same_n(S.restate_terms(K, kind, ash, F, alt=(alt,))[key], _restated(pkg, BIG, kind, ash)[key])
    for kind in ("RAS", "DES", "IDDES"):
        assert differs(kind, True, "skew_plain", "s") and differs(kind, True, "skew_plain", "su_prod")
    for kind, ash in VARIANTS:
        assert differs(kind, ash, "magsqr_plain", "su_grad"), (kind, ash)
        assert differs(kind, ash, "cb2_regroup", "su_grad") and differs(kind, ash, "cw1_regroup", "sp"), (kind, ash)
        assert not differs(kind, ash, "r_other", "sp"), (kind, ash)
    for kind in S.KINDS:
        assert differs(kind, True, "fv2_other", "stilda") and differs(kind, True, "chibycv2_other", "stilda"), kind
        assert not differs(kind, False, "fv2_other", "stilda")            # without Ashford both classes write the same fv2
    assert differs("RAS", True, "stilda_other", "stilda") and differs("DES", True, "stilda_other", "stilda")
    assert differs("IDDES", True, "psi_regroup", "dtilda")
    H = _hand_made()
    for kind in ("RAS", "DES"):
        a, b = S.restate_terms(K, kind, True, H), S.restate_terms(K, kind, True, H, alt=("r_other",))
        assert np.all(np.isfinite(a["sp"])) and not same_n(a["r"], b["r"]) and not same_n(a["sp"], b["sp"]), kind
    R = _restated(pkg, BIG, "RAS", True)
    d1, s1 = S.restate_sources(F["V"], F["diag"], F["source"], R["su_grad"], R["su_prod"], R["sp"])
    d2, s2 = S.restate_sources(F["V"], F["diag"], F["source"], R["su_grad"], R["su_prod"], R["sp"], summed=True)
    assert same_n(d1, d2) and not same_n(s1, s2)
    W = S.restate_wall(L, K, F["wall"])
    plain = S.restate_wall(L, K, F["wall"], ev=W["exp"], contracted=False)
    assert not same_n(plain["nut"], W["nut"])


@pytest.mark.parametrize("name", ALL_MESHES)
def test_wall_function_restated_twice(pkg, name):
    """the vectorised and the literal Newton loop agree bit for bit from the same exp values; no err comes within a relative 1e-9 of 0.01 and
    no ut within that of ROOTVSMALL, so a last-bit difference in exp cannot change an iteration count; iteration counts from 1 to the cap of
    10 occur (every count on the 1 200-cell box, the cap and at least five different counts on the others), and both the ut0 <= ROOTVSMALL arm (exactly 0: Uw == U[c]) and the kUu cap of 50 are reached"""
    c = _case(pkg, name)
    L, K, W = c["L"], c["K"], c["F"]["wall"]
    R = S.restate_wall(L, K, W)
    nut, iters = S.literal_wall(L, K, W, R["exp"])
    assert same_n(nut, R["nut"]) and np.array_equal(iters, R["iters"])
    wall = wall_mask(L)
    assert np.all(R["iters"][~wall] == -1) and same_n(R["nut"][~wall], W["bnutw"][~wall]) and np.all(np.isfinite(R["nut"])) and np.all(R["nut"][wall] >= 0)
    assert np.all(np.abs(R["errs"] / 0.01 - 1.0) > 1e-9) and np.all(np.abs(R["uts"] / S.ROOTVSMALL - 1.0) > 1e-9)
    counts = set(R["iters"][wall].tolist())
    assert np.any(R["zero"]) and np.all(R["mgu"][R["zero"]] == 0.0) and np.all(R["iters"][wall][R["zero"]] == 0) and np.all(R["nut"][wall][R["zero"]] == 0.0)
    assert np.any(R["capped"]) and not np.all(R["capped"])
    assert {0, 10} <= counts and len(counts) >= 5, sorted(counts)
    if name == BIG:
        assert counts == set(range(11)), sorted(counts)
    taken = np.sum(~np.isnan(R["exp"]), axis=1)
    assert np.array_equal(taken[wall], R["iters"][wall]) and np.all(taken[~wall] == 0)
    print(f"{name}: iteration counts {np.bincount(R['iters'][wall], minlength=11).tolist()}, kUu capped on {int(R['capped'].sum())} faces")


def test_host_side_refusals_need_no_device(pkg):
    """what the entries refuse before any device call: missing or broken coefficients, an unknown kind, a nu that is not above zero, DES kinds
    without delta, DDES and IDDES without nuSgs, IDDES without hmax, an optional output the kind does not form, a missing context or handle"""
    import ctypes as C
    eng = pkg.engine
    lib = eng.lib()
    null, one = C.c_void_p(0), C.c_int64(1)
    good, broken = eng.sa_coeffs(), eng.sa_coeffs()
    broken.Cw1 = NAN
    x = eng.SaCells()
    x.nu_value = 1e-5
    bad_nu = eng.SaCells()
    ctx = C.c_void_p(8)                      # never dereferenced: every call below is refused before the context is used
    has = lambda **kw: (lambda s: ([setattr(s, k, v) for k, v in kw.items()], s)[1])(eng.SaCells(nu_value=1e-5))
    d = C.c_double
    for call, why in ((lambda: lib.mi_sa_terms(null, one, None, 0, 1, C.byref(x)), "coefficients"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(broken), 0, 1, C.byref(x)), "above zero"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(good), 4, 1, C.byref(x)), "kind"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(good), -1, 1, C.byref(x)), "kind"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(good), 0, 1, None), "arrays are missing"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(good), 0, 1, C.byref(bad_nu)), "nu must be"),
                      (lambda: lib.mi_sa_terms(null, one, C.byref(good), 0, 1, C.byref(x)), "bad argument"),
                      (lambda: lib.mi_sa_terms(ctx, C.c_int64(-1), C.byref(good), 0, 1, C.byref(x)), "bad argument"),
                      (lambda: lib.mi_sa_terms(ctx, one, C.byref(good), 1, 1, C.byref(x)), "delta"),
                      (lambda: lib.mi_sa_terms(ctx, one, C.byref(good), 2, 1, C.byref(has(delta_dev=8))), "nuSgs"),
                      (lambda: lib.mi_sa_terms(ctx, one, C.byref(good), 3, 1, C.byref(has(delta_dev=8, nusgs_dev=8))), "hmax"),
                      (lambda: lib.mi_sa_terms(ctx, one, C.byref(good), 0, 1, C.byref(has(tanh_fd_out_dev_or_null=8))), "does not form"),
                      (lambda: lib.mi_sa_terms(ctx, one, C.byref(good), 2, 1, C.byref(has(delta_dev=8, nusgs_dev=8, exp_out_dev_or_null=8))), "does not form"),
                      (lambda: lib.mi_sa_nut(null, one, None, 1, null, null, null, d(1e-5), null, null), "coefficients"),
                      (lambda: lib.mi_sa_nut(null, one, C.byref(good), 1, null, null, null, d(0.0), null, null), "nu must be"),
                      (lambda: lib.mi_sa_nut(null, one, C.byref(good), 0, null, null, null, d(0.0), null, C.c_void_p(8)), "not an output"),
                      (lambda: lib.mi_sa_nut(null, one, C.byref(good), 1, null, null, null, d(1e-5), null, null), "bad argument"),
                      (lambda: lib.mi_sa_nut_spalding_wall(null, C.byref(good), None), "bad argument"),
                      (lambda: lib.mi_sa_coeffs_init(None, None, None), "bad argument")):
        assert call() != 0
        assert why in lib.mi_last_error().decode(), (why, lib.mi_last_error().decode())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _eq(got, want, tag):
    assert same_n(got, want), (tag, int(np.sum(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))) if got.shape == want.shape else "shape")


def _odd(dev, a):
    """the same values at an address that is 8 bytes past a 16-byte boundary: the one-cell-at-a-time form of the cell passes"""
    return dev(np.concatenate([[0.0], a]))[1:]


def _call_terms(A, K, kind, ash, f, nu, req, opt):
    A.sa_terms(K, kind, ash, f["nt"], f["grad"], f["gnt"], f["y"], nu, *req, delta=f["delta"], nusgs=f["nusgs"], hmax=f["hmax"], **opt)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_terms(pkg, monkeypatch, name, blocks):
    """mi_sa_terms for the four kinds, with and without the Ashford correction, nu a number and a cell array, with 16-byte aligned arrays (two
    cells per thread) and with arrays 8 bytes off (one by one), with and without the optional outputs, the launch grid at its default and forced
    to 1 and 3 workgroups, through a caller-order and an ordered addressing.  Every pow / tanh / exp value within its bar of numpy's on the same
    argument; everything else bit for bit against the restatement continued from the device's values; the same bits on every run"""
    import torch
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, F = c["L"], c["F"]
    n, K = L["n"], eng.sa_coeffs()
    worst = {}
    A = eng.Assembly(eng.Addressing(ctx, n, L["lo"], L["up"]))
    Ao = eng.Assembly(eng.Addressing(ctx, n, L["lo"], L["up"], ordered=True))
    for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
        f = {key: put(F[key]) for key in ("nt", "y", "delta", "nusgs", "hmax", "nu_f")}
        f["grad"], f["gnt"] = [put(x) for x in F["grad"]], [put(x) for x in F["gnt"]]
        for kind, ash in VARIANTS:
            for nu_key in ("nu", "nu_f"):
                tag = (name, blocks, "aligned" if put is dev else "8 bytes off", kind, ash, nu_key)
                nu = F["nu"] if nu_key == "nu" else f["nu_f"]
                names = ("s", "dtilda", "stilda") + S.TRANSCENDENTALS[kind]
                req, opt = [out(n) for _ in range(5)], {key: out(n) for key in names}
                _call_terms(A, K, kind, ash, f, nu, req, opt)
                got = {key: host(t) for key, t in opt.items()}
                got.update({key: host(t) for key, t in zip(S.OUTPUTS[:5], req)})
                R = _restated(pkg, name, kind, ash, nu_key, cont={t: got[t] for t in S.TRANSCENDENTALS[kind]})
                for t in S.TRANSCENDENTALS[kind]:
                    f_np = {"pow_fw": lambda x: np.power(x, 1.0 / 6.0), "exp": np.exp, "pow_hill_pos": lambda x: np.power(x, -11.09),
                            "pow_hill_neg": lambda x: np.power(x, -9.0), "pow_fl": lambda x: np.power(x, 10.0)}.get(t, np.tanh)
                    with np.errstate(all="ignore"):
                        ok, rel = S.within(got[t], f_np(R["arg_" + t]), S.BOUNDS[t])
                    worst[t] = max(worst.get(t, 0.0), rel)
                    assert ok, tag + (t, rel * 2.0 ** 52)
                for key in S.OUTPUTS:
                    _eq(got[key], R[key], tag + (key,))
                # without the optional outputs, and through the ordered addressing: the same bits
                req1 = [out(n) for _ in range(5)]
                _call_terms(Ao if nu_key == "nu" else A, K, kind, ash, f, nu, req1, {})
                for key, t in zip(S.OUTPUTS[:5], req1):
                    _eq(host(t), got[key], tag + (key, "without the optional outputs"))
    print(f"{name}: largest relative deviation of the device's library values from numpy in units of 2^-52: "
          + ", ".join(f"{t} {v * 2.0 ** 52:.2f}" for t, v in sorted(worst.items())))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_nut(pkg, monkeypatch, name, blocks):
    """mi_sa_nut with the stored fv1 (the RAS correct()) and with fv1 recomputed from nu a number and a cell array (updateSubGridScaleFields),
    aligned and 8 bytes off; the recomputed fv1 equals mi_sa_terms's"""
    set_face_grid(monkeypatch, blocks)
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    c = _case(pkg, name)
    L, F, Kh = c["L"], c["F"], c["K"]
    n, K = L["n"], eng.sa_coeffs()
    A = eng.Assembly(eng.Addressing(ctx, n, L["lo"], L["up"]))
    Ao = eng.Assembly(eng.Addressing(ctx, n, L["lo"], L["up"], ordered=True))
    for put, out in ((dev, E), (lambda a: _odd(dev, a), lambda m: E(m + 1)[1:])):
        nt = put(F["nt"])
        for nu_key in ("nu", "nu_f"):
            want, fv1 = S.restate_nut(Kh, F["nt"], nu=F[nu_key])
            assert same_n(fv1, _restated(pkg, name, "RAS", True, nu_key)["fv1"])
            o, o1, fo = out(n), out(n), out(n)
            A.sa_nut(K, nt, o, nu=F["nu"] if nu_key == "nu" else put(F["nu_f"]), fv1_out=fo)
            _eq(host(o), want, (name, blocks, nu_key, "recomputed")); _eq(host(fo), fv1, (name, blocks, nu_key, "fv1"))
            A.sa_nut(K, nt, o1, nu=F["nu"] if nu_key == "nu" else put(F["nu_f"]))
            _eq(host(o1), want, (name, blocks, nu_key, "recomputed, fv1 not returned"))
            o2, o3 = out(n), out(n)
            A.sa_nut(K, nt, o2, fv1=put(fv1))
            _eq(host(o2), want, (name, blocks, nu_key, "stored"))
            Ao.sa_nut(K, nt, o3, fv1=put(fv1))
            _eq(host(o3), want, (name, blocks, nu_key, "stored, ordered addressing"))
            o4 = out(n)
            Ao.sa_nut(K, nt, o4, nu=F["nu"] if nu_key == "nu" else put(F["nu_f"]))
            _eq(host(o4), want, (name, blocks, nu_key, "recomputed, ordered addressing"))


def _wall_layouts(eng, ctx, L):
    for tag, ordered in (("caller", False), ("ordered", True)):
        addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"], ordered=ordered)
        B = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(L["patches"]))
        yield tag, addr, B, eng.KEpsilon(addr, B, [w for _, w in L["patches"]])


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 1, 3])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_spalding_wall(pkg, monkeypatch, name, blocks):
    """mi_sa_nut_spalding_wall on every layout (the box layouts with corner cells on several wall patches, the graph layouts with shared cells,
    `big` with more wall faces than one workgroup): every exp value within EXP_BOUND of numpy's on the same argument; the iteration counts and
    nut bit for bit against the loop replayed from the device's exp values; faces off the walls and steps not taken are not written"""
    import torch
    set_face_grid(monkeypatch, blocks)
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, name)
    L, Kh, W = c["L"], c["K"], c["F"]["wall"]
    K = eng.sa_coeffs()
    nb = boundary_cells(L).shape[0]
    wall = wall_mask(L)
    ref = S.restate_wall(L, Kh, W)
    worst = 0.0
    for tag, addr, B, H in _wall_layouts(eng, ctx, L):
        A = eng.Assembly(addr)
        for put in (dev, lambda a: _odd(dev, a)):
            u, uw = [put(x) for x in W["U"]], [put(x) for x in W["Uw"]]
            bdc, by, bnuw = put(W["bdc"]), put(W["by"]), put(W["bnuw"])
            nut, ev = put(W["bnutw"]), E(10 * nb)
            it = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
            A.sa_nut_spalding_wall(H, K, u, uw, bdc, by, bnuw, nut, ev, it)
            evh, ith = host(ev).reshape(nb, 10), host(it)
            written = evh != fill
            assert np.array_equal(written.sum(axis=1)[wall], ith[wall]) and not np.any(written[~wall]) and np.all(ith[~wall] == -1), (name, tag)
            assert np.all(written == (np.arange(10)[None, :] < np.maximum(ith, 0)[:, None]))
            R = S.restate_wall(L, Kh, W, ev=np.where(written, evh, np.nan))
            assert np.array_equal(R["iters"], ith), (name, tag, blocks)
            assert np.array_equal(ith, ref["iters"]), "the exp values' last bits do not change an iteration count (the asserted margins)"
            with np.errstate(all="ignore"):                      # on the SAME argument: kUu of the loop replayed from the device's values
                ok, rel = S.within(evh[written], np.exp(R["arg"][written]), S.EXP_BOUND)
            worst = max(worst, rel)
            assert ok, (name, tag, rel * 2.0 ** 52)
            _eq(host(nut), R["nut"], (name, tag, blocks, "nut"))
            nut1 = put(W["bnutw"])
            A.sa_nut_spalding_wall(H, K, u, uw, bdc, by, bnuw, nut1)
            _eq(host(nut1), R["nut"], (name, tag, blocks, "nut without the optional outputs"))
        H.close(); B.close()
    print(f"{name}: largest relative deviation of the device's exp from numpy in units of 2^-52: {worst * 2.0 ** 52:.2f}")
    torch.cuda.synchronize()


def _sa_channel_walk(pkg, orc, kind, ordered, ash=True):
    """The constructor's viscosity line and three correct() steps of one model on the 6 x 5 x 4 channel (a fixed-value inlet, a zero-gradient
    outlet, four walls with nutUSpaldingWallFunction), driven through the Python binding: grad(nuTilda) from mi_gauss_grad with its boundary
    values each step, mi_sa_terms on the cells AND on the patch-ordered boundary arrays, mi_face_interpolate(dnu), ONE mi_fvm_assemble with
    sp > 0 and the two sources su_grad, su_prod with sign < 0, mi_relax, the boundary coefficients, PBiCG, bound, mi_sa_nut (the stored fv1
    for RAS, recomputed for the LES classes) on cells and boundary faces, then the wall pass, which reads a wall face's earlier value.  Every
    intermediate up to what the solver is handed equals the restatement bit for bit; the restatement continues from the engine's solution
    and from the device's library values.  The assembled diagonal and source are also held to diagL + V*sp and
    (sourceL + V*su_grad) + V*su_prod directly, and the summed form V*(su_grad + su_prod) is shown to differ -> the states"""
    import torch
    from turbulence_support import patch_coeffs
    eng, ctx, dev, host, E = gpu_env(pkg, fill=NAN)
    M, St = S.channel(pkg)
    L, n, nf, nb = M["L"], M["n"], M["nf"], M["nb"]
    K, wall = eng.sa_coeffs(), wall_mask(L)
    nu, rdt = M["nu"], 1.0 / M["dt"]
    fcs = [fc for fc, _ in L["patches"]]
    addr = eng.Addressing(ctx, n, M["lo"], M["up"], ordered=ordered)
    A = eng.Assembly(addr)
    Bd = eng.GradBoundary(addr, fcs, ["fixesValue" if kd == "inlet" else "other" for kd in M["kinds"]])
    H = eng.KEpsilon(addr, Bd, [kd == "wall" for kd in M["kinds"]])
    patches = [eng.Patch(ctx, n, fc) for fc in fcs]
    cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
    g = {key: dev(M[key]) for key in ("V", "magSf", "dc", "lam", "bms", "bdc", "by", "phi", "bnuw", "y", "delta", "bdelta", "hmax", "bhmax")}
    Sf, bSf = [dev(x) for x in M["Sf"]], [dev(x) for x in M["bSf"]]
    AV = eng.Average(addr, Bd, g["magSf"], g["bms"])
    U, Uw, grad, bgrad = [dev(x) for x in M["U"]], [dev(x) for x in M["Uw"]], [dev(x) for x in M["grad"]], [dev(x) for x in M["bgrad"]]
    inlet = torch.from_numpy(M["kind_of"] == "inlet").to("cuda:0")
    off_wall = torch.from_numpy(~wall).to("cuda:0")
    bcells = torch.from_numpy(boundary_cells(L).astype(np.int64)).to("cuda:0")
    mat = eng.Matrix(addr)
    libs = S.TRANSCENDENTALS[kind]

    def boundary_of(cell, inlet_value):
        out = E(nb)
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            p.internal_field(cell, out[a:b])
        out[inlet] = inlet_value
        return out

    def full_grad(vf, bvf):
        ssf, gr, bg = E(nf), [E(n) for _ in range(3)], [E(nb) for _ in range(3)]
        A.face_interpolate(g["lam"], vf, ssf)
        A.gauss_grad(Sf, ssf, None, gr)
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            for d in range(3):
                p.add_product(bSf[d][a:b], bvf[a:b], gr[d], 0)
        gr = [x / g["V"] for x in gr]
        sn = g["bdc"] * (bvf - vf[bcells])
        for p, a, b in zip(patches, cut[:-1], cut[1:]):
            p.gauss_grad_correct([x[a:b] for x in bSf], g["bms"][a:b], [sn[a:b]], gr, [x[a:b] for x in bg])
        return gr, bg

    def nut_update(nt, bnt, bnut, fv1=None, bfv1=None):
        nut, bcalc, ev = E(n), E(nb), torch.full((10 * nb,), NAN, dtype=torch.float64, device="cuda:0")
        it = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
        if fv1 is None:
            A.sa_nut(K, nt, nut, nu=nu); A.sa_nut(K, bnt, bcalc, nu=nu)
        else:
            A.sa_nut(K, nt, nut, fv1=fv1); A.sa_nut(K, bnt, bcalc, fv1=bfv1)
        bnut = bnut.clone()
        bnut[off_wall] = bcalc[off_wall]
        A.sa_nut_spalding_wall(H, K, U, Uw, g["bdc"], g["by"], g["bnuw"], bnut, ev, it)
        return nut, bnut, host(ev).reshape(nb, 10), host(it)

    def terms(m, nt, gr, gnt, y, delta, nusgs, hmax):
        req, opt = [E(m) for _ in range(5)], {key: E(m) for key in ("s", "dtilda", "stilda") + libs}
        A.sa_terms(K, kind, ash, nt, gr, gnt, y, nu, *req, delta=delta, nusgs=nusgs, hmax=hmax, **opt)
        return dict(zip(S.OUTPUTS[:5], req), **opt)

    nt, bnt = dev(St["nt"]), dev(St["bnt"])
    nut, bnut, ev, _ = nut_update(nt, bnt, torch.zeros(nb, dtype=torch.float64, device="cuda:0"))
    St = S.restate_channel_constructor(M, St, dict(ev=ev))
    _eq(host(nut), St["nut"], (kind, "nut0")); _eq(host(bnut), St["bnut"], (kind, "bnut0"))
    keys = ("nt", "bnt", "nut", "bnut")
    states = [{key: np.array(St[key]) for key in keys}]
    for step in range(M["steps"]):
        D = {}
        gn, bgn = full_grad(nt, bnt)
        for d in range(3):
            D.update({"gradNt%d" % d: host(gn[d]), "bgradNt%d" % d: host(bgn[d])})
        o = terms(n, nt, grad, gn, g["y"], g["delta"], nut, g["hmax"])
        b = terms(nb, bnt, bgrad, bgn, g["by"], g["bdelta"], bnut, g["bhmax"])
        D.update({key: host(o[key]) for key in S.OUTPUTS}); D.update({"b" + key: host(b[key]) for key in S.OUTPUTS})
        X = dict(lib={t: host(o[t]) for t in libs}, blib={t: host(b[t]) for t in libs})
        gam = E(nf)
        A.face_interpolate(g["lam"], o["dnu"], gam)
        gam = gam * g["magSf"]
        upper, lower, diag, source, uL, lL, dL, sL = E(nf), E(nf), E(n), E(n), E(nf), E(nf), E(n), E(n)
        common = dict(ddt=dict(r_delta_t=rdt, vol=g["V"], psi_old=[nt.clone()]), div=dict(flux=g["phi"], weights=g["lam"]),
                      laplacian=dict(delta_coeffs=g["dc"], gamma_magsf=gam))
        A.assemble(uL, dL, lL, [sL], **common)
        A.assemble(upper, diag, lower, [source], sp=(o["sp"], 1.0), su=[(-1.0, [o["su_grad"]]), (-1.0, [o["su_prod"]])], **common)
        D.update(gam=host(gam), upper0=host(upper), lower0=host(lower), diagL=host(dL), sourceL=host(sL), diag0=host(diag), source0=host(source))
        V, a_, b_ = M["V"], D["su_grad"], D["su_prod"]
        _eq(D["diag0"], D["diagL"] + V * D["sp"], (kind, step, "diagL + V*sp"))
        _eq(D["source0"], (D["sourceL"] + V * a_) + V * b_, (kind, step, "(sourceL + V*su_grad) + V*su_prod"))
        assert not same_n(D["source0"], D["sourceL"] + V * (a_ + b_)), "the summed form differs in a compared bit"
        ich, bch = patch_coeffs(M, D["bdnu"], M["nt_in"])
        ic, bc = [dev(x) for x in ich], [dev(x) for x in bch]
        A.relax(M["alpha_nt"], diag, lower, upper, source, nt, patches, ic, bc, [0] * len(patches))
        ds, ss = diag.clone(), source.clone()
        for p, i, c_ in zip(patches, ic, bc):
            p.add(i, ds, 0); p.add(c_, ss, 0)
        D.update(diag1=host(diag), source1=host(source), ic=np.concatenate([host(x) for x in ic]), bc=np.concatenate([host(x) for x in bc]),
                 diag_solve=host(ds), source_solve=host(ss))
        mat.set_coeffs(ds, upper, lower)
        perf = mat.pbicg(nt, ss, "diagonal", tolerance=1e-10, relTol=0.0, maxIter=300)
        assert 0 < perf["nIterations"] < 300
        X["nt_solved"] = host(nt).copy()
        bnt = boundary_of(nt, M["nt_in"])
        lo_ = min(A.min_max(nt)[0], A.min_max(bnt)[0])
        D["bounded"] = bool(lo_ < 0.0)
        if D["bounded"]:
            A.vec_max_value(bnt, 0.0, bnt)
            A.bound(AV, 0.0, g["lam"], g["magSf"], nt, g["bms"], bnt)
        stored = kind == "RAS"
        nut, bnut, ev, it = nut_update(nt, bnt, bnut, o["fv1"] if stored else None, b["fv1"] if stored else None)
        X["ev"] = ev
        D.update(nt_new=host(nt), bnt_new=host(bnt), nut=host(nut), bnut=host(bnut), iters=it)
        want, St = S.restate_channel_correct(orc, M, kind, ash, St, X)
        assert set(want) == set(D), set(want) ^ set(D)
        for key in sorted(want):
            if isinstance(want[key], bool):
                assert D[key] == want[key], (kind, step, key)
            elif key == "iters":
                assert np.array_equal(D[key], want[key]), (kind, step, key)
            else:
                _eq(D[key], want[key], (kind, step, key))
        for key in keys:
            assert np.all(np.isfinite(St[key])) and np.all(St[key] >= 0), (kind, step, key)
        assert np.all(St["nt"] > 0)
        print(f"{kind} step {step}: nuTilda {St['nt'].min():.3e}..{St['nt'].max():.3e}  nut {St['nut'].min():.3e}..{St['nut'].max():.3e}  "
              f"wall nut {St['bnut'][wall].min():.3e}..{St['bnut'][wall].max():.3e}  Newton steps {D['iters'][wall].min()}..{D['iters'][wall].max()}")
        states.append({key: np.array(St[key]) for key in keys})
    for h in (AV, H, Bd):
        h.close()
    return M, states


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["caller", "ordered"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_channel_walk(pkg, orc, kind, ordered):
    """_sa_channel_walk for each of the four models under the caller's numbering and under ordered addressing"""
    _sa_channel_walk(pkg, orc, kind, ordered)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------
def test_mirror_declares_the_spalart_allmaras_classes(pkg):
    """foam/miFoam: incompressible::RASModels::SpalartAllmaras and LESModels::SpalartAllmaras, SpalartAllmarasDDES and SpalartAllmarasIDDES (the
    last two derived from the first LES class) with the reference's coefficient names and the virtuals S and dTilda are declared and in the
    library"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    text = open(os.path.join(PKG, "foam", "miFoam.H")).read()
    body = text[text.index("class SpalartAllmarasBase"):]
    for word in ("sigmaNut_", "kappa_", "Cb1_", "Cb2_", "Cw1_", "Cw2_", "Cw3_", "Cv1_", "Cv2_", "CDES_", "ck_", "fwStar_", "cl_", "ct_", "ashfordCorrection_",
                 "class SpalartAllmarasDDES : public SpalartAllmaras", "class SpalartAllmarasIDDES : public SpalartAllmaras", "virtual void S(",
                 "virtual void dTilda(", "void fd(", "nuTilda()", "nut()", "nuSgs()", "DnuTildaEff(", "void correct(", "updateSubGridScaleFields("):
        assert word in body, word
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libmiFoam.so")], capture_output=True, text=True, check=True).stdout
    inc = "Foam::incompressible::"
    for name in (inc + "SpalartAllmarasBase::correct(", inc + "RASModels::SpalartAllmaras::SpalartAllmaras(", inc + "LESModels::SpalartAllmaras::SpalartAllmaras(",
                 inc + "LESModels::SpalartAllmaras::S(", inc + "LESModels::SpalartAllmaras::dTilda(", inc + "LESModels::SpalartAllmarasDDES::SpalartAllmarasDDES(",
                 inc + "LESModels::SpalartAllmarasDDES::S(", inc + "LESModels::SpalartAllmarasDDES::dTilda(", inc + "LESModels::SpalartAllmarasDDES::fd(",
                 inc + "LESModels::SpalartAllmarasIDDES::SpalartAllmarasIDDES(", inc + "LESModels::SpalartAllmarasIDDES::dTilda(",
                 inc + "LESModels::SpalartAllmarasIDDES::fd("):
        assert len(re.findall(r" T " + re.escape(name), syms)) >= 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.KINDS)
def test_mirror_walks_the_channel(pkg, orc, tmp_path, kind):
    """foam/miFoam's Spalart-Allmaras classes -- the constructor and three correct() calls of each model, through the driver
    foam/spalartAllmarasChannel.C in a process of its own, with the solver of the walk (PBiCG, diagonal, 1e-10) -- give nuTilda, nut / nuSgs and
    their boundary values of the Python walk bit for bit after the constructor and after every step; S() of the LES classes (skew; symm for
    DDES, through the virtual) and dTilda() of the DES class equal the restatement on the constructor's state"""
    import subprocess
    from komegasst_support import restate_grad
    M, states = _sa_channel_walk(pkg, orc, kind, False)
    L = M["L"]
    types = {"inlet": 0, "outlet": 1, "wall": 2}
    d = str(tmp_path)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{kind} {M['n']} {M['nf']} {M['steps']} {repr(1.0 / M['dt'])} {repr(M['nu'])} {repr(M['alpha_nt'])} {len(M['kinds'])}\n")
        for (fc, _), kd in zip(L["patches"], M["kinds"]):
            f.write(f"{fc.shape[0]} {types[kd]}\n")
    put = lambda name, a, dt=np.float64: np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name + ".bin"))
    put("lower", M["lo"], np.int32); put("upper", M["up"], np.int32); put("faceCells", boundary_cells(L), np.int32)
    for name, key in (("weights", "lam"), ("deltaCoeffs", "dc"), ("magSf", "magSf"), ("V", "V"), ("bMagSf", "bms"), ("bDeltaCoeffs", "bdc"), ("y", "by"),
                      ("yCell", "y"), ("phi", "phi"), ("bPhi", "bphi"), ("delta", "delta"), ("bDelta", "bdelta"), ("hmax", "hmax"), ("bHmax", "bhmax")):
        put(name, M[key])
    for c in range(3):
        put(f"U{c}", M["U"][c]); put(f"bU{c}", M["Uw"][c]); put(f"Sf{c}", M["Sf"][c]); put(f"bSf{c}", M["bSf"][c])
        for k in range(3):
            put(f"gradU{c}_{k}", M["grad"][3 * c + k]); put(f"bgradU{c}_{k}", M["bgrad"][3 * c + k])
    first = states[0]
    put("nuTilda", first["nt"]); put("bnuTilda", first["bnt"])
    app = os.path.join(os.path.dirname(pkg.engine.LIB_PATH), "spalartAllmarasChannel")
    run = subprocess.run([app, d], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    names = dict(nt="nuTilda", bnt="bnuTilda", nut="nut", bnut="bnut")
    for step, want in enumerate(states):
        for key, name in names.items():
            got = np.fromfile(os.path.join(d, f"{name}_{step}.bin"), dtype=np.float64)
            _eq(got, want[key], (kind, step, key))
    if kind != "RAS":
        g, _ = restate_grad(orc, M, first["nt"], first["bnt"])
        F = dict(nt=first["nt"], grad=M["grad"], gnt=g, y=M["y"], nu=M["nu"], delta=M["delta"], nusgs=first["nut"], hmax=M["hmax"])
        R = S.restate_terms(M["SA"], kind, True, F)
        _eq(np.fromfile(os.path.join(d, "S_0.bin"), dtype=np.float64), R["s"], (kind, "S()"))
        if kind == "DES":
            _eq(np.fromfile(os.path.join(d, "dTilda_0.bin"), dtype=np.float64), R["dtilda"], (kind, "dTilda()"))


class Misaligned:
    """a device address four bytes into a float64 tensor, as engine._ptr takes one: not aligned for a double"""

    def __init__(self, t):
        self.t, self.dtype = t, t.dtype

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def numel(self):
        return self.t.numel() - 1

    def data_ptr(self):
        return self.t.data_ptr() + 4


@pytest.mark.gpu
def test_refusals_launch_nothing(pkg):
    import torch
    fill = -77.0
    eng, ctx, dev, host, E = gpu_env(pkg, fill=fill)
    c = _case(pkg, "box")
    L, F = c["L"], c["F"]
    n, K = L["n"], eng.sa_coeffs()
    addr = eng.Addressing(ctx, n, L["lo"], L["up"])
    A = eng.Assembly(addr)
    bad = Misaligned(E(n + 1))
    f = {key: dev(F[key]) for key in ("nt", "y", "delta", "nusgs", "hmax", "nu_f")}
    f["grad"], f["gnt"] = [dev(x) for x in F["grad"]], [dev(x) for x in F["gnt"]]
    o = [E(n) for _ in range(16)]
    broken = eng.sa_coeffs()
    broken.invCv2 = NAN

    def terms(kind="IDDES", K_=K, nu=1e-5, req=None, **kw):
        g = dict(f)
        opt = {key: kw.pop(key) for key in list(kw) if key in eng.SA_OPTIONAL}
        g.update(kw)
        _call_terms(A, K_, kind, True, g, nu, o[:5] if req is None else req, opt)

    for kw, why in ((dict(nt=None), "missing"), (dict(y=None), "missing"), (dict(grad=f["grad"][:8] + [None]), "missing"), (dict(gnt=None), "missing"),
                    (dict(kind="DES", delta=None), "delta"), (dict(kind="DDES", nusgs=None), "nuSgs"), (dict(hmax=None), "hmax"),
                    (dict(req=o[:4] + [None]), "missing"), (dict(req=o[:4] + [f["y"]]), "alias"), (dict(req=o[:4] + [o[0]]), "differ"),
                    (dict(s=f["nt"]), "alias"), (dict(exp=o[2]), "differ"), (dict(req=o[:4] + [bad]), "aligned"), (dict(y=bad), "aligned"),
                    (dict(nu=bad), "aligned"), (dict(K_=None), "coefficients"), (dict(K_=broken), "above zero"), (dict(kind=7), "kind"),
                    (dict(nu=0.0), "nu must be"), (dict(nu=NAN), "nu must be"), (dict(kind="RAS", tanh_fd=o[9]), "does not form"),
                    (dict(kind="DDES", exp=o[10]), "does not form")):
        with pytest.raises(eng.MiError, match=why):
            terms(**kw)
    for kw, why in ((dict(nutilda=None), "missing"), (dict(nut_out=None), "missing"), (dict(nut_out=f["nt"]), "alias"), (dict(fv1_out=o[0]), "differ"),
                    (dict(nut_out=bad), "aligned"), (dict(nu=-1.0), "nu must be"), (dict(fv1=f["y"], nu=None, fv1_out=o[1]), "not an output"),
                    (dict(coeffs=broken), "above zero")):
        args = dict(coeffs=K, nutilda=f["nt"], nut_out=o[0], nu=1e-5)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            A.sa_nut(**args)
    # the wall function (a handle cannot be of another addressing than its own: mi_ke_create binds it, and the entry takes no second one)
    W = F["wall"]
    B = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(L["patches"]))
    H = eng.KEpsilon(addr, B, [w for _, w in L["patches"]])
    nb = boundary_cells(L).shape[0]
    u, uw = [dev(x) for x in W["U"]], [dev(x) for x in W["Uw"]]
    bdc, by, bnuw, nut = dev(W["bdc"]), dev(W["by"]), dev(W["bnuw"]), dev(W["bnutw"])
    ev, it = E(10 * nb), torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
    good = dict(coeffs=K, u=u, b_uw=uw, b_delta_coeffs=bdc, b_y=by, b_nuw=bnuw, b_nutw_inout=nut, b_exp_out=ev, b_iter_out=it)
    for kw, why in ((dict(u=None), "missing"), (dict(b_uw=uw[:2] + [None]), "missing"), (dict(b_y=None), "missing"), (dict(b_nutw_inout=None), "missing"),
                    (dict(b_nutw_inout=by), "alias"), (dict(b_exp_out=nut), "differ"), (dict(b_exp_out=bnuw), "alias"), (dict(b_nuw=bad), "aligned"),
                    (dict(b_nutw_inout=bad), "aligned"), (dict(coeffs=None), "coefficients"), (dict(coeffs=broken), "above zero")):
        args = dict(good)
        args.update(kw)
        with pytest.raises(eng.MiError, match=why):
            H.sa_nut_spalding_wall(**args)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == fill)) for t in o + [bad.t, ev]) and bool(torch.all(it == -1))
    assert same(host(nut), W["bnutw"]) and same(host(f["nt"]), F["nt"]) and same(host(f["y"]), F["y"])
    # the valid calls after them write every value
    terms(**{key: o[5 + i] for i, key in enumerate(eng.SA_OPTIONAL)})
    H.sa_nut_spalding_wall(**good)
    torch.cuda.synchronize()
    assert not any(bool(torch.any(t == fill)) for t in o) and not same(host(nut), W["bnutw"])
    H.close(); B.close()


@pytest.mark.gpu
def test_zero_cells_and_zero_wall_faces_are_ok(pkg):
    """MI_OK and nothing read or written: every cell pass on empty arrays, the wall function on a handle without wall patches"""
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg, fill=-77.0)
    L = _case(pkg, "box")["L"]
    addr = eng.Addressing(ctx, L["n"], L["lo"], L["up"])
    A = eng.Assembly(addr)
    e, K = E(0), eng.sa_coeffs()
    for kind in S.KINDS:
        A.sa_terms(K, kind, True, e, [e] * 9, [e] * 3, e, 1e-5, e, e, e, e, e, delta=e, nusgs=e, hmax=e)
    A.sa_nut(K, e, e, nu=1e-5)
    A.sa_nut(K, e, e, fv1=e)
    B = eng.GradBoundary(addr, [fc for fc, _ in L["patches"]], ["other"] * len(L["patches"]))
    H = eng.KEpsilon(addr, B, [False] * len(L["patches"]))
    nb = boundary_cells(L).shape[0]
    nut = E(nb)
    H.sa_nut_spalding_wall(K, None, None, None, None, None, nut)
    torch.cuda.synchronize()
    assert bool(torch.all(nut == -77.0))
    H.close(); B.close()
