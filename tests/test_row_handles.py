"""What the row-pass entries share on the host, pinned entry by entry: the six handle creates refuse a boundary of another addressing with
one text, every row entry reports the first of two simultaneous faults (an output that aliases an input, an array four bytes off 8-byte
alignment) in its own order, and one valid call per entry equals its support module's restatement bit for bit.  Two boxes of
synthetic.box_case, 2x2x2 and 3x2x2, each with one plain patch that gives every cell one boundary face."""
import numpy as np
import pytest

import cmules_support
import interface_support
import least_squares_support
import mules_support
import reconstruct_support
import turbulence_support
from assembly_support import gpu_env, same
from test_limited_grad import restate as restate_limited_grad
from test_reconstruct import Misaligned

DIMS = ((2, 2, 2), (3, 2, 2))
CREATES = ("mi_ls_vectors_create", "mi_reconstruct_create", "mi_mules_create", "mi_interface_create", "mi_average_create", "mi_ke_create")
ALIAS, ALIGN = "an output must not alias an input", "arrays must be aligned to 8 bytes"
# the fault each entry reports when both are present: the entries that test alignment first say ALIGN.  mi_limited_grad and mi_ls_grad have
# no alignment check at all, so their misaligned array is inert and the case pins the alias message, not an order; the three entries of
# interface.inc and turbulence.inc test aliasing before alignment
FIRST_FAULT = {"mi_limited_grad": ALIAS, "mi_ls_grad": ALIAS, "mi_fvc_reconstruct": ALIGN, "mi_mules_limiter": ALIGN, "mi_mules_correct": ALIGN,
               "mi_interface_curvature": ALIAS, "mi_fvc_average": ALIAS, "mi_bound": ALIAS}
FILL = -77.0


def box(syn, dims, seed):
    """the box's addressing with seeded geometry and fields: a dict every support module reads (fcs / kinds, and patches for turbulence_support)"""
    case = syn.box_case(*dims)
    n = case.n_cells
    lo, up = np.ascontiguousarray(case.lower_addr, dtype=np.int32), np.ascontiguousarray(case.upper_addr, dtype=np.int32)
    nf, nb = lo.shape[0], n
    u = lambda k, m: syn.splitmix_uniform(seed + k, m)
    fc = np.arange(n, dtype=np.int32)
    L = dict(n=n, lo=lo, up=up, fcs=[fc], kinds=[0], patches=[(fc, False)],
             C=[u(d, n) for d in range(3)], Cf=[u(3 + d, nf) for d in range(3)], bcf=[u(6 + d, nb) for d in range(3)],
             w=0.3 + 0.4 * u(9, nf), magSf=0.5 + u(10, nf), bw=0.3 + 0.4 * u(11, nb), bms=0.5 + u(12, nb), bd=[u(13 + d, nb) - 0.5 for d in range(3)],
             Sf=[u(16 + d, nf) - 0.5 for d in range(3)], bSf=[u(19 + d, nb) - 0.5 for d in range(3)])
    v = u(22, n) - 0.5
    v[::3] = -v[::3] - 0.6                                     # bound: cells below the bound
    L.update(vf=u(23, n) - 0.5, bv=u(24, nb) - 0.5, grad=[40.0 * (u(25 + d, n) - 0.5) for d in range(3)], ssf=u(28, nf) - 0.5, bssf=u(29, nb) - 0.5,
             vol=0.5 + u(30, n), lam=0.3 + 0.4 * u(31, nf), v=v, bface=u(32, nb) - 0.3, lb=1e-15)
    L["I"] = mules_support.make_inputs(syn, L, seed + 40)
    return L


class Device:
    """one box on the device: the addressing, its boundary, the six handles and the device copies of the box's arrays"""

    def __init__(self, env, L):
        self.eng, self.ctx, self.dev, self.host, self.E = env
        eng, dev = self.eng, self.dev
        self.L = L
        self.addr = eng.Addressing(self.ctx, L["n"], L["lo"], L["up"])
        self.A = eng.Assembly(self.addr)
        self.B = eng.GradBoundary(self.addr, L["fcs"], L["kinds"])
        self.d = {k: ([dev(x) for x in v] if isinstance(v, list) else dev(v)) for k, v in L.items()
                  if k not in ("n", "lo", "up", "fcs", "kinds", "patches", "I", "lb")}
        self.handles = {name: self.create(name, self.B) for name in CREATES}

    def create(self, name, B):
        eng, d, addr = self.eng, self.d, self.addr
        if name == "mi_ls_vectors_create":
            return eng.LsVectors(addr, B, d["C"], d["w"], d["magSf"], b_weights=d["bw"], b_mag_sf=d["bms"], b_delta=d["bd"])
        if name == "mi_reconstruct_create":
            return eng.Reconstruct(addr, B, d["Sf"], d["magSf"], d["bSf"], d["bms"])
        if name == "mi_mules_create":
            return eng.Mules(addr, B, None)
        if name == "mi_interface_create":
            return eng.Interface(addr, B)
        if name == "mi_average_create":
            return eng.Average(addr, B, d["magSf"], d["bms"])
        return eng.KEpsilon(addr, B, [False])

    def mules_fields(self, I, vol=None, with_psi=True):
        dev = self.dev
        psi = dev(I["psi"]) if with_psi else None
        return self.eng.mules_fields(dev(I["V"]) if vol is None else vol, psi, dev(I["psi0"]) if with_psi else None, r_delta_t=I["rdt"],
                                     b_psi=dev(I["bpsi"]) if with_psi else None, psi_max=I["psiMax"], psi_min=I["psiMin"])

    def close(self):
        for h in self.handles.values():
            h.close()
        self.B.close()


# ---- one call per entry: bad=True makes the two faults, otherwise -> [(got, want)] --------------------------------------------------------
def limited_grad(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    lim = D.eng.grad_limiter("cellLimited Gauss linear 0.5")
    g, lout = [x.clone() for x in d["grad"]], [E(n)]
    C = [d["C"][0], Misaligned(E(n + 1)), d["C"][2]] if bad else d["C"]
    D.A.limited_grad(lim, [d["vf"]], C, d["Cf"], [d["vf"]] + g[1:] if bad else g, boundary=D.B, bvalue=[d["bv"]], bcf=d["bcf"], limiter_out=lout)
    rg, rlim = restate_limited_grad("cellLimited", 0.5, n, L["lo"], L["up"], L["C"], L["Cf"], [L["vf"]], L["grad"], L["fcs"][0], np.zeros(n, int),
                                    [L["bv"]], L["bcf"])
    return list(zip(g + lout, rg + rlim))


def ls_grad(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    out = [E(n) for _ in range(3)]
    D.A.ls_grad(D.handles["mi_ls_vectors_create"], [d["vf"]], [d["vf"]] + out[1:] if bad else out, bvalue=[Misaligned(E(n + 1)) if bad else d["bv"]])
    return list(zip(out, least_squares_support.restate_grad(orc, L, least_squares_support.restate_vectors(orc, L), [L["vf"]], [L["bv"]])))


def fvc_reconstruct(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    out = [E(n) for _ in range(3)]
    D.A.reconstruct(D.handles["mi_reconstruct_create"], [d["ssf"]], [d["ssf"]] + out[1:] if bad else out,
                    b_ssf=[Misaligned(E(n + 1)) if bad else d["bssf"]])
    return list(zip(out, reconstruct_support.restate_reconstruct(orc, L, reconstruct_support.restate_build(orc, L), L["ssf"], L["bssf"])))


def mules_limiter(D, orc, bad):
    L, I, dev, E = D.L, D.L["I"], D.dev, D.E
    bd, corr, lam = mules_support.restate_form(L, I)
    t = dict(phi_bd=dev(bd[0]), b_phi_bd=dev(bd[1]), phi_corr=dev(corr[0]), b_phi_corr=dev(corr[1]), lambda_=dev(lam[0]), b_lambda_=dev(lam[1]))
    if bad:
        t["lambda_"] = t["phi_corr"]
    D.handles["mi_mules_create"].limiter(D.mules_fields(I, vol=Misaligned(E(L["n"] + 1)) if bad else None), D.eng.mules_flux(**t), 3)
    want = mules_support.restate_limit(L, I, 3, False, given=(bd, corr, lam))["lam"]
    return [(t["lambda_"], want[0]), (t["b_lambda_"], want[1])]


def mules_correct(D, orc, bad):
    L, I, dev, E = D.L, D.L["I"], D.dev, D.E
    corr = mules_support.restate_form(L, I)[1]
    vol, psi = dev(I["V"]), dev(I["psi"])
    D.handles["mi_mules_create"].correct(D.mules_fields(I, vol=vol, with_psi=False), Misaligned(E(L["lo"].shape[0] + 1)) if bad else dev(corr[0]),
                                         vol if bad else psi, dev(corr[1]))
    return [(psi, cmules_support.restate_correct(L, I, corr))]


def interface_curvature(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    K = E(n)
    D.handles["mi_interface_create"].curvature(Misaligned(E(L["lo"].shape[0] + 1)) if bad else d["ssf"], d["vol"], d["vol"] if bad else K, d["bssf"])
    return [(K, interface_support.restate_curvature(L, L["ssf"], L["bssf"], L["vol"]))]


def fvc_average(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    out = E(n)
    D.handles["mi_average_create"].fvc_average(d["magSf"], d["ssf"], d["ssf"] if bad else out, d["bms"], Misaligned(E(n + 1)) if bad else d["bssf"])
    return [(out, turbulence_support.restate_average(L, L["magSf"], L["bms"], L["ssf"], L["bssf"])[0])]


def bound(D, orc, bad):
    L, d, E, n = D.L, D.d, D.E, D.L["n"]
    v = d["v"].clone()
    D.handles["mi_average_create"].bound(L["lb"], d["lam"], d["magSf"], d["lam"] if bad else v, d["bms"], Misaligned(E(n + 1)) if bad else d["bface"])
    return [(v, turbulence_support.restate_bound(L, L["lb"], L["lam"], L["magSf"], L["bms"], L["bface"], L["v"]))]


ENTRIES = {"mi_limited_grad": limited_grad, "mi_ls_grad": ls_grad, "mi_fvc_reconstruct": fvc_reconstruct, "mi_mules_limiter": mules_limiter,
           "mi_mules_correct": mules_correct, "mi_interface_curvature": interface_curvature, "mi_fvc_average": fvc_average, "mi_bound": bound}


@pytest.fixture(scope="module")
def boxes(pkg):
    env = gpu_env(pkg, fill=FILL)
    out = [Device(env, box(pkg.synthetic, dims, 900 + 100 * i)) for i, dims in enumerate(DIMS)]
    yield out
    for D in out:
        D.close()


def refusal(eng, text, call):
    with pytest.raises(eng.MiError) as e:
        call()
    assert str(e.value) == "mi error -1: " + text


@pytest.mark.gpu
@pytest.mark.parametrize("name", CREATES)
def test_create_refuses_the_boundary_of_the_other_box(pkg, boxes, name):
    assert [D.L["n"] for D in boxes] == [8, 12]
    for D, other in (boxes, boxes[::-1]):
        refusal(D.eng, name + ": the boundary was built for another addressing", lambda: D.create(name, other.B))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENTRIES))
def test_two_faults_report_the_entry_s_first(pkg, orc, boxes, name):
    for D in boxes:
        refusal(D.eng, name + ": " + FIRST_FAULT[name], lambda: ENTRIES[name](D, orc, True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENTRIES))
def test_valid_call_equals_the_restatement(pkg, orc, boxes, name):
    for D in boxes:
        pairs = ENTRIES[name](D, orc, False)
        assert pairs
        for i, (got, want) in enumerate(pairs):
            assert np.all(np.isfinite(want)), (name, D.L["n"], i)
            assert same(D.host(got), want), (name, D.L["n"], i)
