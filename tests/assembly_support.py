"""Shared by the scheme tests that pin the engine to the reference bit for bit: the device helpers, the row-plan shapes, the exact
arithmetic, and the fused-assembly check (mi_fvm_assemble* against the engine's own scheme-by-scheme sequence and against a restatement).

Functions and constants only; `monkeypatch` comes from the calling test.  A new scheme's row-shape test starts from set_row_tables /
set_row_blocks / shaped_addressing, its fused-assembly test from FusedCase (tests/test_backward_ddt.py is the shortest user)."""
from fractions import Fraction

import numpy as np


# ---- device helpers --------------------------------------------------------------------------------------------------------------
def gpu_env(pkg, fill=None):
    """-> eng, ctx, dev (host array -> float64 device tensor), host (device tensor -> array, after a synchronize), E (m -> an output
    tensor: uninitialised, or filled with `fill` where a test asserts that a refused call launched nothing)"""
    import torch
    eng = pkg.engine
    ctx = eng.Context(0, torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    host = lambda t: (torch.cuda.synchronize(), t.cpu().numpy())[1]
    if fill is None:
        E = lambda m: torch.empty(m, dtype=torch.float64, device="cuda:0")
    else:
        E = lambda m: torch.full((m,), fill, dtype=torch.float64, device="cuda:0")
    return eng, ctx, dev, host, E


# ---- row-plan shapes ---------------------------------------------------------------------------------------------------------------
ROW_MODES = ("fixed256", "fixed1024", "tiles", "tiles_unstaged", "fixed_unstaged")
# the forms of the row tables and of the block mapping that the defaults never take: (tables, mode)
OTHER_TABLES = ([("row32", m) for m in ROW_MODES] + [("noxcd", m) for m in ("fixed256", "tiles")])
# (mesh, mode, tables) of the time schemes' fused-assembly tests
SHAPES = ([(name, mode, "default") for name in ("box", "graph") for mode in ROW_MODES[:4]]
          + [("box", "fixed256", "row32"), ("graph", "tiles", "noxcd")])


def set_row_tables(monkeypatch, tables):
    """"default" | "row32" | "noxcd".  Call it BEFORE gpu_env: MI_XCD_ROWS is read by mi_ctx_create, MI_ROW16 when an addressing makes
    its row plans (ensure_caller_tables, at its first caller-order operator).  Set later, the test passes and tests the default."""
    monkeypatch.delenv("MI_ROW16", raising=False); monkeypatch.delenv("MI_XCD_ROWS", raising=False)
    if tables == "row32":       # the 32-bit row tables: also what a block that does not fit 16 bits falls back to
        monkeypatch.setenv("MI_ROW16", "0")
    elif tables == "noxcd":     # blockIdx.x as it comes, in every row pass, face pass and gradient pass
        monkeypatch.setenv("MI_XCD_ROWS", "0")
    else:
        assert tables == "default"


def set_row_blocks(monkeypatch, mode, grad=False):
    """the block shape of a ROW_MODES entry: cells per block under the caller's numbering (MI_ROW_BS; grad: MI_GRAD_BS too, the plan of
    the gradient passes) and, for the *_unstaged modes, a staging capacity no block fits (MI_ROW_CAP=64).  Call it before creating the
    addressing the test runs on: the three are read when that addressing makes its row plans."""
    bs = "1024" if mode == "fixed1024" else "256"
    monkeypatch.setenv("MI_ROW_BS", bs)
    if grad:
        monkeypatch.setenv("MI_GRAD_BS", bs)
    if mode.endswith("unstaged"):
        monkeypatch.setenv("MI_ROW_CAP", "64")


def shaped_addressing(eng, ctx, syn, case, mode):
    """-> (case, addr).  tiles*: the case renumbered into the tile order of a probe addressing, under ordered addressing on the probe's
    tile starts (the row passes own the layout's tiles); otherwise the case as it is (fixed ranges of cells)"""
    if mode.startswith("tiles"):
        a0 = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
        case = syn.renumber(case, a0.cell_perm())
        addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
        assert addr.is_ordered
        return case, addr
    return case, eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)


def shape_case(pkg, name, symmetric=False):
    """the two meshes of the shape tests, the smallest with several tiles and several 1024-cell blocks with cut faces on both sides"""
    from conftest import random_graph_case
    if name == "box":
        return pkg.synthetic.box_case(31, 23, 19, symmetric=symmetric)
    return random_graph_case(pkg, 9000, extra=3.0, seed=5, symmetric=symmetric)


# ---- exact arithmetic --------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, signed zeros included"""
    return np.array_equal(bits(a), bits(b))


def fma(a, b, c):
    """one rounding: exact rational arithmetic, then float() rounds to nearest even"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma_each(a, b, c):
    """element-wise fma with ONE rounding (non-finite operands: a*b + c)"""
    out = np.empty(a.shape[0])
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        out[i] = float(Fraction(x) * Fraction(y) + Fraction(z)) if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) else x * y + z
    return out


def dot_contracted(ax, ay, az, bx, by, bz):
    """Vector & Vector as the compiled reference contracts it and as every face pass of the engine does: fma(az, bz, fma(ax, bx, ay*by)).
    Pinned by the oracle's flux_face against the compiled reference (tests/test_oracle.py)"""
    return fma(az, bz, fma(ax, bx, ay * by))


def rmax(a, b):
    """doubleScalar max (label.H:285-298 MAXMIN): (s1 > s2) ? s1 : s2 -- max(-0.0, 0.0) is +0.0"""
    return a if a > b else b


def rmin(a, b):
    """(s1 < s2) ? s1 : s2"""
    return a if a < b else b


def box_centres(dims):
    """cell centres of the uniform lexicographic box"""
    nx, ny, nz = dims
    h = 1.0 / nx
    c = np.arange(nx * ny * nz)
    return [(c % nx + 0.5) * h, ((c // nx) % ny + 0.5) * h, (c // (nx * ny) + 0.5) * h]


def signed_flux(u, neg_zero=True):
    """a face flux of both signs from uniform numbers, with exact zeros -- of both signs unless neg_zero is False"""
    f = u - 0.45
    f[::7] = 0.0
    if neg_zero:
        f[3::11] = -0.0
    return f


# ---- the fused-assembly check -------------------------------------------------------------------------------------------------------
# n_rhs, density, convection weights (None: upwind; "w": given; False: no convection), Sp and the two explicit terms, the correction
VARIANTS = [
    dict(tag="momentum", n_rhs=3, field=True, div=None, extras=True, corr=False),
    dict(tag="scalar", n_rhs=1, field=False, div="w", extras=False, corr=False),
    dict(tag="symmetric", n_rhs=1, field=False, div=False, extras=True, corr=False),
    dict(tag="corrected", n_rhs=3, field=True, div=None, extras=True, corr=True),
    dict(tag="corrected_scalar", n_rhs=1, field=False, div=None, extras=False, corr=True),
]


def fused_inputs(pkg, n, nf):
    u = pkg.synthetic.splitmix_uniform
    return dict(flux=signed_flux(u(110, nf), neg_zero=False), w=0.3 + 0.4 * u(140, nf), vol=0.5 + u(111, n), delta=1.0 + u(107, nf),
                gamma=0.5 + u(108, nf), rho=0.8 + u(135, n), rho0=0.7 + u(136, n), rho00=0.6 + u(137, n), sp=u(153, n),
                psi0=[u(131 + k, n) - 0.5 for k in range(3)], psi00=[u(171 + k, n) - 0.5 for k in range(3)],
                su=[u(154 + k, n) - 0.5 for k in range(3)], su2=[u(158 + k, n) - 0.5 for k in range(3)],
                C=[u(144 + k, n) for k in range(3)], cf=[u(147 + k, nf) for k in range(3)],
                grad=[[4.0 * (u(200 + 3 * r + k, n) - 0.5) for k in range(3)] for r in range(3)])


def euler_ddt_call(A, r_delta_t, vol, psi_old, rho_value=None, rho=None, rho_old=None):
    """the ddt_call of unfused_sequence for the Euler scheme: fvm::ddt(rho, vf) with a density field, or with the constant rho_value"""
    if rho is not None:
        return lambda r, dd, ds: A.fvm_ddt_euler_rho(r_delta_t, rho, rho_old, vol, psi_old[r], dd, ds)
    return lambda r, dd, ds: A.fvm_ddt_euler(r_delta_t, rho_value, vol, psi_old[r], dd, ds)


def unfused_sequence(A, E, vol, ddt_call, n_rhs, lap, div=None, sp=None, su=()):
    """The engine's scheme-by-scheme calls for  ddt + [div] - laplacian [- Sp] == [- su + su2], combined with mi_vec_axpby the way
    fvMatrix::operator+ / - combine them (fvMatrix.C:1693-2030) -- what one mi_fvm_assemble* call must equal bit for bit.  div, lap, sp
    and su as Assembly.assemble takes them (device arrays; div["weights"] None: upwind; su: () or the pair [(1.0, su), (-1.0, su2)]);
    ddt_call(r, diag_out, source_out) issues the time scheme's one launch for right-hand side r.  -> dict(lower, upper, diag, src, t):
    t the correction's face fields"""
    n, nf = vol.numel(), lap["delta_coeffs"].numel()
    corr = div.get("correction") if div else None
    cl, cu, cd, lu, ld, dd, ds = E(nf), E(nf), E(n), E(nf), E(n), E(n), [E(n) for _ in range(n_rhs)]
    t = [E(nf) for _ in range(n_rhs)]
    if div:
        flux, wts = div["flux"], div.get("weights")
        if wts is None:
            wts = E(nf); A.upwind_weights(flux, wts)
        A.fvm_div(wts, flux, cl, cu, cd)
        if corr:
            A.linear_upwind_correction(flux, corr["cf"], corr["c"], corr["grad"], t)
    A.fvm_laplacian(lap["delta_coeffs"], lap["gamma_magsf"], lu, ld)
    for r in range(n_rhs):
        ddt_call(r, dd, ds[r])
        if corr:
            ivf = E(n); A.surface_integrate(t[r], vol, ivf); A.submul(vol, ivf, ds[r])
        if su:
            A.fvm_su(vol, su[0][1][r], ds[r])                           # + su: source -= V*su
            p = vol * su[1][1][r]; ds[r].add_(p)                        # == su2: source += V*su2
    if div:
        A.axpby(1.0, cl, -1.0, lu, cl); A.axpby(1.0, cu, -1.0, lu, cu)
        A.axpby(1.0, dd, 1.0, cd, dd)
    else:
        A.axpby(-1.0, lu, 0.0, lu, cu)
    A.axpby(1.0, dd, -1.0, ld, dd)
    if sp is not None:
        p = vol * sp[0]; dd.sub_(p)
    return dict(lower=cl if div else None, upper=cu, diag=dd, src=ds, t=t)


class FusedCase:
    """one (mesh, mode, tables) of SHAPES: the row tables and blocks, the device, the mesh under its addressing, fused_inputs, the
    Assembly, and what every variant shares"""

    def __init__(self, pkg, orc, monkeypatch, name, mode, tables):
        set_row_tables(monkeypatch, tables)
        set_row_blocks(monkeypatch, mode)
        self.orc = orc
        self.eng, self.ctx, self.dev, self.host, self.E = gpu_env(pkg)
        self.case, self.addr = shaped_addressing(self.eng, self.ctx, pkg.synthetic, shape_case(pkg, name), mode)
        self.n, self.nf, self.lo, self.up = self.case.n_cells, self.case.n_faces, self.case.lower_addr, self.case.upper_addr
        self.q = fused_inputs(pkg, self.n, self.nf)
        self.A = self.eng.Assembly(self.addr)
        self.vol, self.flux = self.dev(self.q["vol"]), self.dev(self.q["flux"])
        self.lap = dict(delta_coeffs=self.dev(self.q["delta"]), gamma_magsf=self.dev(self.q["gamma"]))
        self.uL, self.dL = orc.fvm_laplacian(self.n, self.lo, self.up, self.q["delta"], self.q["gamma"])

    def variant(self, v):
        return FusedVariant(self, v)


class FusedVariant:
    """one entry of VARIANTS on a FusedCase: the arguments of Assembly.assemble on the device --
      ddt   vol, psi_old and the density (rho + rho_old, or rho_value); the scheme's test adds r_delta_t and its own key
      rho   the density part of ddt alone, as the keywords of the unfused ddt calls
      div, sp, su, and the case's lap
    -- and psi_old_old / rho_old_old (None without a density field) for the schemes that read them"""

    def __init__(self, case, v):
        q, dev = case.q, case.dev
        self.case, self.v, self.tag, self.R = case, v, v["tag"], v["n_rhs"]
        R = self.R
        self.psi_old = [dev(x) for x in q["psi0"][:R]]
        self.psi_old_old = [dev(x) for x in q["psi00"][:R]]
        if v["field"]:
            self.rho, self.rho_old_old = dict(rho=dev(q["rho"]), rho_old=dev(q["rho0"])), dev(q["rho00"])
        else:
            self.rho, self.rho_old_old = dict(rho_value=1.2), None
        self.ddt = dict(vol=case.vol, psi_old=self.psi_old, **self.rho)
        self.div = None
        if v["div"] is not False:
            self.div = dict(flux=case.flux, weights=dev(q["w"]) if v["div"] == "w" else None)
            if v["corr"]:
                grads = [[dev(x) for x in g] for g in q["grad"][:R]]
                self.div["correction"] = dict(scale=1.0, cf=[dev(x) for x in q["cf"]], c=[dev(x) for x in q["C"]], grad=grads)
        self.sp = (dev(q["sp"]), -1.0) if v["extras"] else None
        self.su = [(1.0, [dev(x) for x in q["su"][:R]]), (-1.0, [dev(x) for x in q["su2"][:R]])] if v["extras"] else []

    def fused(self, ddt_arg):
        """one Assembly.assemble call -> its outputs (lower None without convection)"""
        c, E = self.case, self.case.E
        o = dict(lower=E(c.nf) if self.div else None, upper=E(c.nf), diag=E(c.n), mag=E(c.n), src=[E(c.n) for _ in range(self.R)])
        c.A.assemble(o["upper"], o["diag"], lower_out=o["lower"], sources_out=o["src"], ddt=ddt_arg, div=self.div, laplacian=c.lap, sp=self.sp,
                     su=self.su, sum_mag_out=o["mag"])
        return o

    def unfused(self, ddt_call):
        c = self.case
        return unfused_sequence(c.A, c.E, c.vol, ddt_call, self.R, c.lap, div=self.div, sp=self.sp, su=self.su)

    def euler(self, r_delta_t):
        """the Euler scheme's ddt_call on this variant's fields"""
        return euler_ddt_call(self.case.A, r_delta_t, self.case.vol, self.psi_old, **self.rho)

    def assert_same(self, got, seq, what):
        """(a) a fused call's coefficients and every source against an unfused sequence's"""
        host = self.case.host
        for key in ("lower", "upper", "diag"):
            if got[key] is not None:
                assert np.array_equal(host(got[key]), host(seq[key])), (self.tag, what, key)
        for r in range(self.R):
            assert np.array_equal(host(got["src"][r]), host(seq["src"][r])), (self.tag, what, r)

    def assert_restated(self, got, seq, restated_ddt):
        """(b) a fused call against the restatement: restated_ddt(r) -> (diag, source) of the time scheme for right-hand side r in numpy,
        the rest by the oracle's sweeps and numpy field operations, one rounding each; the corrected variants take the correction's face
        field from the engine's own face pass (seq["t"]), which tests/test_linear_upwind.py pins"""
        c, v, q, orc, host = self.case, self.v, self.case.q, self.case.orc, self.case.host
        n, lo, up = c.n, c.lo, c.up
        if self.div:
            wh = orc.upwind_weights(q["flux"]) if v["div"] is None else q["w"]
            lB, uB, dB = orc.fvm_div(n, lo, up, wh, q["flux"])
            lower, upper = lB - c.uL, uB - c.uL
        else:
            lower, upper = None, -c.uL
        for r in range(self.R):
            dD, s = restated_ddt(r)
            if v["corr"]:
                ivf = orc.surface_integrate(n, lo, up, host(seq["t"][r]), q["vol"])
                s = s - q["vol"] * ivf
            if v["extras"]:
                s = s - q["vol"] * q["su"][r]
                s = s + q["vol"] * q["su2"][r]
            assert np.array_equal(host(got["src"][r]), s), (self.tag, r)
        diag = ((dD + dB) - c.dL) if self.div else (dD - c.dL)
        if v["extras"]:
            diag = diag - q["vol"] * q["sp"]
        assert np.array_equal(host(got["diag"]), diag) and np.array_equal(host(got["upper"]), upper), self.tag
        if self.div:
            assert np.array_equal(host(got["lower"]), lower), self.tag
        assert np.array_equal(host(got["mag"]), orc.row_face_op(2, n, lo, up, lower, upper, np.zeros(n))), self.tag
