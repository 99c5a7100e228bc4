"""The TVD/NVD limited interpolation schemes (limitedSchemes/*, LimitedScheme.C:32-57,140-196, limitedSurfaceInterpolationScheme.C:155-161)
and their V (NVDVTVDV.H) and bounded (Limited.H, Limited01.H) forms.  An independent restatement of every limiter from the reference
headers, with fma written out exactly (Fraction) where the compiled reference contracts; then mi_limiter_parse on the
host and the engine's face pass and coupled-patch pass against the restatement, bit for bit (gpu)."""
import os
import numpy as np
import pytest

from assembly_support import bits, dot_contracted, fma, gpu_env, rmax, rmin, same, set_row_tables, signed_flux

SMALL = 1e-15                                                   # doubleScalar.H: SMALL = 1.0e-15
KINDS = ["limitedLinear", "vanLeer", "MUSCL", "Minmod", "SuperBee", "UMIST", "vanAlbada", "OSPRE", "QUICK", "limitedCubic", "Gamma", "SFCD"]
WITH_K = {"limitedLinear", "limitedCubic", "Gamma"}             # limiters whose constructor reads a coefficient k
BOUNDED = {"limitedLinear": ("limitedLimitedLinear", "limitedLinear01"), "vanLeer": ("limitedVanLeer", "vanLeer01"),
           "MUSCL": ("limitedMUSCL", "MUSCL01"), "limitedCubic": ("limitedLimitedCubic", "limitedCubic01"),
           "Gamma": ("limitedGamma", "Gamma01")}               # makeLLimitedSurfaceInterpolationTypeScheme in vanLeer.C, MUSCL.C, ...


def dot(a, b):
    """Vector & Vector of two triples, as the compiled reference contracts it"""
    return dot_contracted(a[0], a[1], a[2], b[0], b[1], b[2])


def sign(s):
    """Scalar.H sign(): s >= 0 ? 1 : -1 (sign(0) = +1)"""
    return 1.0 if s >= 0 else -1.0


def stabilise(s, small):
    """Scalar.H stabilise(): s >= 0 ? s + small : s - small"""
    return s + small if s >= 0 else s - small


def d_and_grad(d, g):
    """vector & tensor for a vector field's gradient, g[3*j + k] = d(phi_j)/dx_k: component j is d & grad(phi_j) (assumed to contract as
    vector & vector)"""
    return [dot(d, g[3 * j:3 * j + 3]) for j in range(3)]


class Hits:
    """counts the branches the inputs reached"""
    def __init__(self):
        self.n = {}

    def __call__(self, key):
        self.n[key] = self.n.get(key, 0) + 1


def _ratio(gradf, gradcf, hit):
    """NVDTVD.H:119-126 / NVDVTVDV.H:121-128: r = 2*(gradcf/gradf) - 1, the guard |gradcf| >= 1000*|gradf| (the product by a power of two
    cannot change the bits fused or not)"""
    if abs(gradcf) >= 1000 * abs(gradf):
        hit("r_guard")
        if gradf == 0:
            hit("gradf_zero")
        return 2 * 1000 * sign(gradcf) * sign(gradf) - 1
    return fma(2.0, gradcf / gradf, -1.0)


def _phict(gradf, gradcf, hit):
    """NVDTVD.H:85-92 / NVDVTVDV.H:85-92: phict = 1 - 0.5*gradf/gradcf, the guard |gradf| >= 1000*|gradcf|"""
    if abs(gradf) >= 1000 * abs(gradcf):
        hit("phict_guard")
        return 1 - 0.5 * 1000 * sign(gradcf) * sign(gradf)
    return 1 - 0.5 * gradf / gradcf


def limiter_face(kind, vec, bounds, k, cdw, flux, pP, pN, gP, gN, d, hit=lambda key: None):
    """LimitedSchemeCalcLimiterFunctor (LimitedScheme.C:41-55) on one face: the limiter of `kind` (its header) over NVDTVD (scalar pP, pN;
    gP, gN 3 components) or NVDVTVDV (vec: pP, pN 3 components; gP, gN 9: g[3*j + k] = d(phi_j)/dx_k); bounds (lower, upper): the
    LimitedLimiter wrapper (Limited.H:93-133, scalar form only); d = C[N] - C[P] (or the patch delta)"""
    if flux == 0:
        hit("zero_flux")
    if bounds is not None:                                      # Limited.H:105-118: upwind outside [lower, upper]; a zero flux is in neither branch
        lo, hi = bounds
        if (flux > 0 and (pP < lo or pN > hi)) or (flux < 0 and (pN < lo or pP > hi)):
            hit("bounded_pos" if flux > 0 else "bounded_neg")
            return 0.0
    up = flux > 0                                               # NVDTVD.H:110: strict
    if vec:
        gfV = [pN[j] - pP[j] for j in range(3)]                 # NVDVTVDV.H:107-119
        gradf = dot(gfV, gfV)
        gradcf = dot(gfV, d_and_grad(d, gP if up else gN))
    else:
        gradf = pN - pP                                         # NVDTVD.H:106-117
        gradcf = dot(d, gP if up else gN)
    if kind in ("Gamma", "SFCD"):
        phict = _phict(gradf, gradcf, hit)
        if kind == "Gamma":                                     # Gamma.H:76 (k rescaled in the constructor), :96
            kk = rmax(k / 2.0, SMALL)
            return rmin(rmax(phict / kk, 0.0), 1.0)
        lp = rmin(rmax(phict, 0.0), 0.5)                          # SFCD.H:81-82
        return lp / (1 - lp)
    if kind == "QUICK":
        q = 1 - cdw
        if vec:                                                 # QUICKV.H:80-101
            w = [fma(cdw, pP[j], q * pN[j]) for j in range(3)]
            phiCD = dot(gfV, w)
            if up:
                phiU = dot(gfV, pP)
                phif = 0.5 * fma(q, dot(gfV, d_and_grad(d, gP)), phiCD + phiU)
            else:
                phiU = dot(gfV, pN)
                phif = 0.5 * fma(-cdw, dot(gfV, d_and_grad(d, gN)), phiCD + phiU)
        else:                                                   # QUICK.H:80-99
            phiCD = fma(cdw, pP, q * pN)
            if up:
                phiU = pP
                phif = 0.5 * fma(q, dot(d, gP), phiCD + pP)
            else:
                phiU = pN
                phif = 0.5 * fma(-cdw, dot(d, gN), phiCD + pN)
        s = phiCD - phiU
        if s < 0:
            hit("stabilise_neg")
        return rmax(rmin((phif - phiU) / stabilise(s, SMALL), 2.0), 0.0)
    r = _ratio(gradf, gradcf, hit)
    if kind in ("limitedLinear", "limitedCubic"):
        twoByk = 2.0 / rmax(k, SMALL)                            # limitedLinear.H:76, limitedCubic.H:76
    if kind == "limitedLinear":
        return rmax(rmin(twoByk * r, 1.0), 0.0)                   # limitedLinear.H:96
    if kind == "vanLeer":
        return (r + abs(r)) / (1 + abs(r))                      # vanLeer.H:81
    if kind == "MUSCL":
        return rmax(rmin(rmin(2 * r, 0.5 * r + 0.5), 2.0), 0.0)    # MUSCL.H:80 (0.5*r exact: fused or not, the same bits)
    if kind == "Minmod":
        return rmax(rmin(r, 1.0), 0.0)                            # Minmod.H:80
    if kind == "SuperBee":
        return rmax(rmax(rmin(2 * r, 1.0), rmin(r, 2.0)), 0.0)      # SuperBee.H:81
    if kind == "UMIST":                                         # UMIST.H:80: 0.75*r + 0.25 fused; 0.25*r exact
        return rmax(rmin(rmin(rmin(2 * r, fma(0.75, r, 0.25)), 0.25 * r + 0.75), 2.0), 0.0)
    if kind == "vanAlbada":
        return r * (r + 1) / fma(r, r, 1.0)                     # vanAlbada.H:81: sqr(r) + 1 fused
    if kind == "OSPRE":
        rrp1 = r * (r + 1)                                      # OSPRE.H:81-82
        return 1.5 * rrp1 / (rrp1 + 1)
    assert kind == "limitedCubic"
    twor = twoByk * r
    q = 1 - cdw
    if vec:                                                     # limitedCubicV.H:91-124
        fV = [fma(cdw, pP[j], (1.0 - cdw) * pN[j]) for j in range(3)]
        fP, fN = dot(fV, pP), dot(fV, pN)
        fU = fP if up else fN
        phif = fma(cdw, fP - 0.25 * dot(fV, d_and_grad(d, gN)), q * (fN + 0.25 * dot(fV, d_and_grad(d, gP))))
        phiCD = fma(cdw, fP, q * fN)
    else:                                                       # limitedCubic.H:91-127
        fU = pP if up else pN
        phif = fma(cdw, pP - 0.25 * dot(d, gN), q * (pN + 0.25 * dot(d, gP)))
        phiCD = fma(cdw, pP, q * pN)
    s = phiCD - fU
    if s < 0:
        hit("stabilise_neg")
    cubic = (phif - fU) / stabilise(s, SMALL)
    return rmax(rmin(rmin(twor, cubic), 2.0), 0.0)


def weight(lim, cdw, flux):
    """limitedSurfaceInterpolationSchemeWeightsFunctor (limitedSurfaceInterpolationScheme.C:155-161): lim*cdw + (1 - lim)*pos(flux), the
    first product fused; pos(): >= 0"""
    return fma(lim, cdw, (1.0 - lim) * (1.0 if flux >= 0 else 0.0))


def restate_internal(kind, vec, bounds, k, lo, up, cdw, flux, phi, grad, Cc, faces=None, hit=lambda key: None):
    """the limiter and weights on the internal faces (or the subset `faces`): phi a list of 1 / 3 cell arrays, grad 3 / 9, Cc 3;
    d = C[N] - C[P] (LimitedScheme.C:53)"""
    m = len(phi)
    faces = range(len(flux)) if faces is None else faces
    lim, w = [], []
    for f in faces:
        P, N = int(lo[f]), int(up[f])
        d = [Cc[j][N] - Cc[j][P] for j in range(3)]
        pP = [phi[j][P] for j in range(m)]
        pN = [phi[j][N] for j in range(m)]
        gP = [g[P] for g in grad]
        gN = [g[N] for g in grad]
        x = limiter_face(kind, vec, bounds, k, float(cdw[f]), float(flux[f]), pP if vec else pP[0], pN if vec else pN[0], gP, gN, d, hit)
        lim.append(x)
        w.append(weight(x, float(cdw[f]), float(flux[f])))
    return np.array(w), np.array(lim)


def restate_patch(kind, vec, bounds, k, fc, pcdw, pflux, phi, nbr_phi, grad, nbr_grad, pd, hit=lambda key: None):
    """LimitedScheme.C:145-195 on one coupled patch: phiP, gradcP the patchInternalField, phiN, gradcN the patchNeighbourField,
    d = pd - (0,0,0) (the patch delta; the subtraction of a zero vector changes no bits)"""
    m = len(phi)
    lim, w = [], []
    for i in range(len(pflux)):
        o = int(fc[i])
        d = [pd[j][i] - 0.0 for j in range(3)]
        pP = [phi[j][o] for j in range(m)]
        pN = [nbr_phi[j][i] for j in range(m)]
        gP = [g[o] for g in grad]
        gN = [g[i] for g in nbr_grad]
        x = limiter_face(kind, vec, bounds, k, float(pcdw[i]), float(pflux[i]), pP if vec else pP[0], pN if vec else pN[0], gP, gN, d, hit)
        lim.append(x)
        w.append(weight(x, float(pcdw[i]), float(pflux[i])))
    return np.array(w), np.array(lim)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def _names():
    """every registered name with valid coefficients -> (kind, vector_form, bounded, k, lower, upper)"""
    out = {}
    for i, kind in enumerate(KINDS):
        ks = " 0.5" if kind in WITH_K else ""
        k = 0.5 if kind in WITH_K else 0.0
        out[kind + ks] = (i, 0, 0, k, 0.0, 0.0)
        out[kind + "V" + ks] = (i, 1, 0, k, 0.0, 0.0)
        if kind in BOUNDED:
            lim_name, name01 = BOUNDED[kind]
            out[lim_name + ks + " -1 2.5"] = (i, 0, 1, k, -1.0, 2.5)
            out[name01 + ks] = (i, 0, 1, k, 0.0, 1.0)
    return out


def test_parse_accepts_every_registered_name(pkg):
    eng = pkg.engine
    names = _names()
    assert len(names) == 34
    for s, want in names.items():
        l = eng.limiter(s)
        assert (l.kind, l.vector_form, l.bounded, l.k, l.lower, l.upper) == want, s
        assert eng.LIMITER_KINDS[l.kind] == KINDS[l.kind]
    for k in ("0", "1", "0.33"):                                # both ends of [0, 1] are valid
        assert eng.limiter("limitedLinear " + k).k == float(k)
    assert eng.limiter("  vanLeer  ").kind == 1                # whitespace around the name
    assert eng.limiter("limitedVanLeer 0.5 0.5").bounded == 1  # lower == upper is allowed (Limited.H:56: lower > upper only)


@pytest.mark.parametrize("scheme, why", [
    ("vanleer", "unknown"), ("upwind", "unknown"), ("linearUpwind grad(U)", "unknown"), ("filteredLinear", "unknown"), ("limitedMinmod -1 1", "unknown"),
    ("Minmod01", "unknown"), ("limitedLinearV01 1", "unknown"), ("vanLeerV01", "unknown"), ("limitedVanLeerV -1 1", "unknown"), ("", "empty"),
    ("limitedLinear", "takes 1"), ("limitedLinearV", "takes 1"), ("vanLeer 1", "extra"), ("limitedLinear 1 1", "extra"), ("Gamma01", "takes 1"),
    ("limitedVanLeer -1", "takes 2"), ("limitedLimitedLinear 1 0", "takes 3"), ("vanLeer01 0.5", "extra"),
    ("limitedLinear 1.5", "k should be"), ("limitedCubic -0.1", "k should be"), ("GammaV 2", "k should be"), ("limitedCubic01 1.01", "k should be"),
    ("limitedVanLeer 2 1", "lower bound"), ("limitedLimitedCubic 0.5 1 -1", "lower bound"), ("limitedLinear x", "not a number"),
])
def test_parse_refuses(pkg, scheme, why):
    eng = pkg.engine
    with pytest.raises(eng.MiError, match=why):
        eng.limiter(scheme)


def test_restatement_limited_linear_equals_the_reference_functor(pkg):
    """the shared r (NVDTVD.H), the limitedLinear limiter and the weight blend against the reference's own compiled functors
    (tests/golden/golden_ref_fvm.npz, inputs rebuilt as tests/test_oracle.py does)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_ref as mg
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ref_fvm.npz"))
    cols = lambda a: [np.ascontiguousarray(a[:, k]) for k in range(3)]
    for name, case in mg.fvm_cases(pkg).items():
        q = mg.fvm_inputs(pkg, case)
        for k in (1.0, 0.33):
            w, lim = restate_internal("limitedLinear", False, None, k, case.lower_addr, case.upper_addr, q["cdw"], q["flux"], [q["phi"]],
                                      cols(q["g3"]), cols(q["C3"]))
            assert same(lim, G[f"{name}/limitedLinear_{k}/limiter"]), (name, k)
            assert same(w, G[f"{name}/limitedLinear_{k}/weights"]), (name, k)


def test_restatement_semantics():
    """the edge semantics each limiter must keep: strict flux > 0 for the upwind side, pos() >= 0 in the weights, both 1000-guards,
    sign(0) = +1, the bounded cut-off (a zero flux in neither branch), stabilise of a negative argument, k = 0"""
    z3 = [0.0, 0.0, 0.0]
    g = [1.0, 0.0, 0.0]
    d = [1.0, 0.0, 0.0]
    # gradf == 0, gradcf > 0: r = 2*1000*1*1 - 1 (sign(0) = +1)
    assert limiter_face("Minmod", False, None, None, 0.5, 1.0, 0.3, 0.3, g, g, d) == 1.0
    assert limiter_face("SuperBee", False, None, None, 0.5, 1.0, 0.3, 0.3, g, g, d) == 2.0
    # zero flux: the NEIGHBOUR's gradient (strict >), weight pos(0) = 1
    assert limiter_face("Minmod", False, None, None, 0.5, 0.0, 0.0, 1.0, g, [-1.0, 0, 0], d) == 0.0
    assert limiter_face("Minmod", False, None, None, 0.5, 1e-300, 0.0, 1.0, g, [-1.0, 0, 0], d) == 1.0
    assert weight(0.0, 0.3, 0.0) == 1.0 and weight(0.0, 0.3, -0.0) == 1.0 and weight(0.0, 0.3, -1e-300) == 0.0
    # phict guard: |gradf| >= 1000*|gradcf| -> 1 - 500*sign*sign; gradcf = 0 -> sign +1
    assert _phict(1.0, 0.0, lambda k: None) == -499.0 and _phict(-1.0, 0.0, lambda k: None) == 501.0
    assert limiter_face("SFCD", False, None, None, 0.5, 1.0, 0.0, -1.0, z3, z3, d) == 1.0      # phict 501 -> 0.5/(1 - 0.5)
    # k = 0: twoByk = 2/SMALL; Gamma k = 0: max(0/2, SMALL)
    assert limiter_face("limitedLinear", False, None, 0.0, 0.5, 1.0, 0.0, 1.0, [1e-3, 0, 0], z3, d) == 0.0    # r = -0.998
    assert limiter_face("limitedLinear", False, None, 0.0, 0.5, 1.0, 0.0, 1.0, [0.6, 0, 0], z3, d) == 1.0
    # bounded: flux > 0 looks at phiP < lo or phiN > hi; flux < 0 the other way; zero flux in neither
    b = (0.0, 1.0)
    assert limiter_face("vanLeer", False, b, None, 0.5, 1.0, -0.1, 0.5, g, g, d) == 0.0
    assert limiter_face("vanLeer", False, b, None, 0.5, -1.0, -0.1, 0.5, g, g, d) != 0.0
    assert limiter_face("vanLeer", False, b, None, 0.5, -1.0, 0.5, -0.1, g, g, d) == 0.0
    assert limiter_face("vanLeer", False, b, None, 0.5, 0.0, -0.1, 1.5, g, g, d) != 0.0
    # max(-0.0, 0) is +0.0 (reference max), not Python's first argument
    assert bits(np.array([rmax(-0.0, 0.0)]))[0] == 0


def test_mirror_exposes_the_limited_schemes(pkg, tmp_path):
    """foam/miFoam: limitedScheme::New parses through mi_limiter_parse (no GPU); an unregistered name is a FatalError"""
    import subprocess
    PKG = os.path.dirname(pkg.engine.LIB_PATH)
    src = tmp_path / "lim.C"
    src.write_text('#include "miFoam.H"\n#include <cstdio>\nusing namespace Foam;\nint main(int argc, char** argv)\n{\n'
                   '    for (int i = 1; i < argc; ++i) { const limitedScheme s = limitedScheme::New(argv[i]);\n'
                   '        std::printf("%d %d %d %.17g %.17g %.17g\\n", s.data().kind, s.data().vector_form, s.data().bounded, s.data().k, s.data().lower, s.data().upper); }\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "lim"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "foam"), "-I", os.path.join(os.path.dirname(PKG), "include"), str(src), "-o", str(exe),
                    "-L" + PKG, "-lmiFoam", "-lrapidcfd_amd", "-Wl,-rpath," + PKG], check=True, capture_output=True)
    names = ["QUICKV", "limitedCubic01 0.25", "limitedVanLeer -1 2", "GammaV 1"]
    out = subprocess.run([str(exe), *names], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [tuple(float(x) for x in line.split()) for line in out.stdout.split("\n") if line]
    assert got == [(8, 1, 0, 0, 0, 0), (9, 0, 1, 0.25, 0, 1), (1, 0, 1, 0, -1, 2), (10, 1, 0, 1, 0, 0)]
    bad = subprocess.run([str(exe), "vanLeerV01"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "unknown limited scheme" in (bad.stdout + bad.stderr)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _schemes():
    """(scheme string, kind name, vec, bounds, k) over every kind x {scalar, V} x {unbounded, the registered bounded forms} x k in {1, 0.33, 0}"""
    out = []
    for kind in KINDS:
        for ks in ((" 1", " 0.33", " 0") if kind in WITH_K else ("",)):
            k = float(ks) if ks else None
            out.append((kind + ks, kind, False, None, k))
            out.append((kind + "V" + ks, kind, True, None, k))
            if kind in BOUNDED:
                out.append((BOUNDED[kind][0] + ks + " -0.2 0.3", kind, False, (-0.2, 0.3), k))
                out.append((BOUNDED[kind][1] + ks, kind, False, (0.0, 1.0), k))
    return out


def _fields(pkg, n, nf, seed):
    """inputs that reach every branch: zero fluxes of both signs, equal and nearly equal neighbour values (gradf == 0, the r guard),
    zero gradients (the phict guard), values either side of the bounds"""
    u = pkg.synthetic.splitmix_uniform
    flux = signed_flux(u(seed, nf))
    cdw = 0.3 + 0.4 * u(seed + 1, nf)
    phi = []
    for j in range(3):
        p = u(seed + 2 + j, n) * 1.6 - 0.5
        sel = u(seed + 5 + j, n)
        p[sel < 0.25] = 0.25
        near = (sel >= 0.25) & (sel < 0.4)
        p[near] = 0.25 + 1e-6 * (u(seed + 8 + j, n)[near] - 0.5)
        phi.append(p)
    grad = []
    for c in range(9):
        g = 2.0 * (u(seed + 20 + c, n) - 0.5)
        g[::9] = 0.0
        grad.append(g)
    return flux, cdw, phi, grad


def _graded_box(pkg, dims):
    """the box with graded cell centres (spacing growing by 5 % per cell in x, 3 % in y)"""
    syn = pkg.synthetic
    case = syn.box_case(*dims)
    nx, ny, nz = dims
    xs = np.cumsum(1.05 ** np.arange(nx)); ys = np.cumsum(1.03 ** np.arange(ny)); zs = np.arange(nz) + 0.5
    c = np.arange(nx * ny * nz)
    return case, [xs[c % nx], ys[(c // nx) % ny], zs[c // (nx * ny)]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "graph", "box_noxcd"])
def test_every_scheme_against_the_restatement(pkg, monkeypatch, name):
    from conftest import random_graph_case
    if name.endswith("_noxcd"):   # the plain blockIdx.x mapping of k_limited_weights
        set_row_tables(monkeypatch, "noxcd"); name = name[:-len("_noxcd")]
    eng, ctx, dev, host, E = gpu_env(pkg)
    if name == "box":
        case, Cc = _graded_box(pkg, (9, 8, 7))
    else:
        case = random_graph_case(pkg, 600, extra=3.0, seed=13)
        Cc = [pkg.synthetic.splitmix_uniform(90 + k, case.n_cells) for k in range(3)]
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    flux, cdw, phi, grad = _fields(pkg, n, nf, 300)
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    fd, wd, pd_, gd, Cd = dev(flux), dev(cdw), [dev(x) for x in phi], [dev(x) for x in grad], [dev(x) for x in Cc]
    hit = Hits()
    for scheme, kind, vec, bounds, k in _schemes():
        lim = eng.limiter(scheme)
        w, lo_ = E(nf), E(nf)
        A.limited_weights(lim, wd, fd, pd_[:3] if vec else pd_[:1], gd if vec else gd[:3], Cd, w, lo_)
        rw, rl = restate_internal(kind, vec, bounds, k, lo, up, cdw, flux, phi[:3] if vec else phi[:1], grad if vec else grad[:3], Cc, hit=hit)
        assert same(host(lo_), rl), scheme
        assert same(host(w), rw), scheme
        w2 = E(nf)
        A.limited_weights(scheme, wd, fd, pd_[:3] if vec else pd_[:1], gd if vec else gd[:3], Cd, w2)   # no limiter output: the same weights
        assert same(host(w2), rw), scheme
    for key in ("zero_flux", "gradf_zero", "r_guard", "phict_guard", "bounded_pos", "bounded_neg", "stabilise_neg"):
        assert hit.n.get(key, 0) > 0, (key, hit.n)


@pytest.mark.gpu
def test_limited_linear_equals_the_existing_kernel_and_the_reference(pkg):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_ref as mg
    eng, ctx, dev, host, E = gpu_env(pkg)
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ref_fvm.npz"))
    cols = lambda a: [dev(np.ascontiguousarray(a[:, k])) for k in range(3)]
    for name, case in mg.fvm_cases(pkg).items():
        q = mg.fvm_inputs(pkg, case)
        nf = case.n_faces
        A = eng.Assembly(eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr))
        g, Cd = cols(q["g3"]), cols(q["C3"])
        for k in (1.0, 0.33):
            w, l, w0, l0 = E(nf), E(nf), E(nf), E(nf)
            A.limited_weights(f"limitedLinear {k}", dev(q["cdw"]), dev(q["flux"]), [dev(q["phi"])], g, Cd, w, l)
            A.limited_linear_weights(k, dev(q["cdw"]), dev(q["flux"]), dev(q["phi"]), g, Cd, w0, l0)
            assert same(host(w), G[f"{name}/limitedLinear_{k}/weights"]) and same(host(l), G[f"{name}/limitedLinear_{k}/limiter"]), (name, k)
            assert same(host(w), host(w0)) and same(host(l), host(l0)), (name, k)


@pytest.mark.gpu
def test_cyclic_patch_against_the_restatement(pkg):
    """LimitedScheme.C:145-195 on a cyclic channel (x-min <-> x-max): phiN and gradcN from mi_matrix_patch_neighbour_field"""
    eng, ctx, dev, host, E = gpu_env(pkg)
    syn = pkg.synthetic
    u = syn.splitmix_uniform
    dims = (12, 7, 6)
    case = syn.box_case(*dims)
    n = case.n_cells
    flux, cdw, phi, grad = _fields(pkg, n, case.n_faces, 400)
    cyc = syn.add_cyclic_x(case)
    fcs = [i.face_cells for i in cyc.interfaces]
    nbrs = [cyc.interfaces[i.nbr_patch].face_cells for i in cyc.interfaces]
    caddr = eng.Addressing(ctx, n, case.lower_addr, case.upper_addr, fcs, nbrs)
    mat = eng.Matrix(caddr)
    npf = [len(f) for f in fcs]
    off = [0, npf[0]]
    pdv, gd = [dev(x) for x in phi], [dev(x) for x in grad]
    nbr_phi = [E(sum(npf)) for _ in range(3)]
    nbr_grad = [E(sum(npf)) for _ in range(9)]
    for j in range(3):
        mat.patch_neighbour_field(pdv[j], nbr_phi[j])
    for c in range(9):
        mat.patch_neighbour_field(gd[c], nbr_grad[c])
    nph, ngh = [host(x) for x in nbr_phi], [host(x) for x in nbr_grad]
    assert same(nph[0], np.concatenate([phi[0][q] for q in nbrs]))
    h = 1.0 / dims[0]
    hit = Hits()
    for p in range(2):
        P = eng.Patch(ctx, n, fcs[p])
        m = npf[p]
        pflux = u(500 + p, m) - 0.45
        pflux[::5] = 0.0
        pcdw = 0.3 + 0.4 * u(510 + p, m)
        pdelta = [np.full(m, -h if p == 0 else h), 0.01 * (u(520 + p, m) - 0.5), np.zeros(m)]
        sl = lambda a: a[off[p]:off[p] + m]
        for scheme, kind, vec, bounds, k in _schemes():
            nc = 3 if vec else 1
            w, l = E(m), E(m)
            P.limited_weights(scheme, dev(pcdw), dev(pflux), pdv[:nc], [sl(x).contiguous() for x in nbr_phi[:nc]], gd[:3 * nc],
                              [sl(x).contiguous() for x in nbr_grad[:3 * nc]], [dev(x) for x in pdelta], w, l)
            rw, rl = restate_patch(kind, vec, bounds, k, fcs[p], pcdw, pflux, phi[:nc], [sl(x) for x in nph[:nc]], grad[:3 * nc],
                                   [sl(x) for x in ngh[:3 * nc]], pdelta, hit=hit)
            assert same(host(l), rl), (p, scheme)
            assert same(host(w), rw), (p, scheme)
        P.close()
    assert hit.n.get("zero_flux", 0) > 0 and hit.n.get("stabilise_neg", 0) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["vanLeer", "limitedLinearV 1"])
def test_limited_weights_feed_the_assembly(pkg, orc, scheme):
    """ddt + div - laplacian with the limited weights through mi_fvm_assemble against the oracle's unfused assembly of the same terms
    with the restated weights"""
    from assembly_full_size import oracle_assemble
    eng, ctx, dev, host, E = gpu_env(pkg)
    case, Cc = _graded_box(pkg, (10, 9, 8))
    n, nf, lo, up = case.n_cells, case.n_faces, case.lower_addr, case.upper_addr
    u = pkg.synthetic.splitmix_uniform
    flux, cdw, phi, grad = _fields(pkg, n, nf, 600)
    vec = scheme.split()[0].endswith("V")
    nc = 3 if vec else 1
    A = eng.Assembly(eng.Addressing(ctx, n, lo, up))
    w = E(nf)
    A.limited_weights(scheme, dev(cdw), dev(flux), [dev(x) for x in phi[:nc]], [dev(x) for x in grad[:3 * nc]], [dev(x) for x in Cc], w)
    l = eng.limiter(scheme)
    rw, _ = restate_internal(eng.LIMITER_KINDS[l.kind], vec, None, l.k, lo, up, cdw, flux, phi[:nc], grad[:3 * nc], Cc)
    assert same(host(w), rw)
    q = dict(vol=0.5 + u(610, n), delta=1.0 + u(611, nf), gamma=0.5 + u(612, nf))
    psi0 = [u(613 + r, n) - 0.5 for r in range(nc)]
    rdt = 1.0 / 3e-4
    up_o, lo_o, dg = E(nf), E(nf), E(n)
    src = [E(n) for _ in range(nc)]
    A.assemble(up_o, dg, lower_out=lo_o, sources_out=src, ddt=dict(vol=dev(q["vol"]), r_delta_t=rdt, psi_old=[dev(x) for x in psi0]),
               div=dict(flux=dev(flux), weights=w), laplacian=dict(delta_coeffs=dev(q["delta"]), gamma_magsf=dev(q["gamma"])))
    ref = oracle_assemble(orc, dict(n=n, lo=lo, up=up), q, dict(rdt=rdt, rho_value=1.0, psi_old=psi0), dict(flux=flux, weights=rw),
                          dict(delta=q["delta"], gamma=q["gamma"]), n_rhs=nc)
    assert same(host(lo_o), ref["lower"]) and same(host(up_o), ref["upper"]) and same(host(dg), ref["diag"])
    for r in range(nc):
        assert same(host(src[r]), ref[f"source{r}"]), r


@pytest.mark.gpu
def test_every_kind_at_the_bench_size(pkg):
    """216^3: every kind, scalar and V, runs over the 30 M faces; 4096 seeded faces per kind against the restatement; limitedLinear
    equals mi_limited_linear_weights over the whole array"""
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg)
    case = pkg.synthetic.box_case(216, 216, 216)
    n, nf = case.n_cells, case.n_faces
    A = eng.Assembly(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr))
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device="cuda:0", generator=gen) * (b - a) + a
    flux, cdw = R(nf, -0.5, 0.5), R(nf, 0.3, 0.7)
    flux[::7] = 0.0
    phi = [R(n, -0.5, 1.1) for _ in range(3)]
    grad = [R(n, -1.0, 1.0) for _ in range(9)]
    Cc = [R(n) for _ in range(3)]
    faces = np.sort(pkg.synthetic.splitmix_uniform(700, 4096) * nf).astype(np.int64)
    lo, up = case.lower_addr[faces], case.upper_addr[faces]
    cells = np.unique(np.concatenate([lo, up]))
    loc = {c: i for i, c in enumerate(cells.tolist())}
    li, ui = np.array([loc[c] for c in lo.tolist()]), np.array([loc[c] for c in up.tolist()])
    ci = torch.from_numpy(cells).to("cuda:0")
    fi = torch.from_numpy(faces).to("cuda:0")
    hc = lambda t: host(t[ci])
    sphi, sgrad, sC = [hc(x) for x in phi], [hc(x) for x in grad], [hc(x) for x in Cc]
    sflux, scdw = host(flux[fi]), host(cdw[fi])
    w, l = E(nf), E(nf)
    for scheme, kind, vec, bounds, k in _schemes():
        if k not in (None, 0.33):
            continue
        nc = 3 if vec else 1
        A.limited_weights(scheme, cdw, flux, phi[:nc], grad[:3 * nc], Cc, w, l)
        rw, rl = restate_internal(kind, vec, bounds, k, li, ui, scdw, sflux, sphi[:nc], sgrad[:3 * nc], sC)
        assert same(host(l[fi]), rl) and same(host(w[fi]), rw), scheme
        if scheme == "limitedLinear 0.33":
            w0, l0 = E(nf), E(nf)
            A.limited_linear_weights(0.33, cdw, flux, phi[0], grad[:3], Cc, w0, l0)
            assert torch.equal(w.view(torch.int64), w0.view(torch.int64)) and torch.equal(l.view(torch.int64), l0.view(torch.int64))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_argument_errors(pkg):
    import torch
    eng, ctx, dev, host, E = gpu_env(pkg)
    case = pkg.synthetic.box_case(6, 5, 4)
    n, nf = case.n_cells, case.n_faces
    flux, cdw, phi, grad = _fields(pkg, n, nf, 800)
    A = eng.Assembly(eng.Addressing(ctx, n, case.lower_addr, case.upper_addr))
    fd, wd, pd_, gd, Cd = dev(flux), dev(cdw), [dev(x) for x in phi], [dev(x) for x in grad], [dev(np.arange(n, dtype=float) * 0.1) for _ in range(3)]
    w, l = E(nf), E(nf)
    sentinel = torch.full((nf,), 7.0, dtype=torch.float64, device="cuda:0")
    call = lambda lim="vanLeer", **kw: A.limited_weights(lim, kw.get("cdw", wd), kw.get("flux", fd), kw.get("phi", pd_[:1]), kw.get("grad", gd[:3]),
                                                         kw.get("C", Cd), kw.get("w", w), kw.get("l", l))
    call()
    bad = eng.limiter("vanLeer"); bad.kind = 12
    with pytest.raises(eng.MiError, match="invalid mi_limiter"):
        call(bad)
    bv = eng.limiter("vanLeerV"); bv.bounded = 1; bv.lower, bv.upper = 0.0, 1.0
    with pytest.raises(eng.MiError, match="scalar fields only"):
        call(bv)
    bk = eng.limiter("limitedLinear 1"); bk.k = 1.5
    with pytest.raises(eng.MiError, match="k should be"):
        call(bk)
    bb = eng.limiter("vanLeer01"); bb.lower = 2.0
    with pytest.raises(eng.MiError, match="lower bound"):
        call(bb)
    with pytest.raises(eng.MiError, match="missing"):
        call(grad=[gd[0], None, gd[2]])
    with pytest.raises(eng.MiError, match="missing"):
        call("vanLeerV", phi=pd_[:1] + [None, None], grad=gd)
    with pytest.raises(eng.MiError, match="missing"):
        call(w=None)
    with pytest.raises(eng.MiError, match="aligned"):
        big = E(nf + 1)
        call(flux=big[1:])
    with pytest.raises(eng.MiError, match="alias"):
        call(w=fd)
    with pytest.raises(eng.MiError, match="alias"):
        call(l=gd[1])
    with pytest.raises(eng.MiError, match="differ"):
        call(w=sentinel, l=sentinel)
    assert torch.all(sentinel == 7.0)                           # nothing was launched
    P = eng.Patch(ctx, n, np.arange(5, dtype=np.int32))
    m5 = E(5)
    with pytest.raises(eng.MiError, match="alias"):
        P.limited_weights("vanLeer", m5, dev(np.ones(5)), pd_[:1], [dev(np.zeros(5))], gd[:3], [dev(np.zeros(5)) for _ in range(3)],
                          [dev(np.ones(5)) for _ in range(3)], m5)
    with pytest.raises(eng.MiError, match="invalid mi_limiter"):
        P.limited_weights(bad, dev(np.ones(5)), dev(np.ones(5)), pd_[:1], [dev(np.zeros(5))], gd[:3], [dev(np.zeros(5)) for _ in range(3)],
                          [dev(np.ones(5)) for _ in range(3)], E(5))
    P.close()
    torch.cuda.synchronize()
