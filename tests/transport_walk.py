"""Shared by the application tests: ONE walk of scalarTransportFoam's statements on the oracle

    solve(fvm::ddt(T) + fvm::div(phi, T) - fvm::laplacian(DT, T))      per time step and non-orthogonal corrector

with the convection scheme, the Laplacian's explicit part, the step sizes and the time scheme as parameters, and what the tests that run an
application do with its output: the solver lines of a log, their comparison with a walk's, the rewrite of a case's fvSchemes entries.

A time scheme is a small object with its own state:  start_step(step, dts, Told)  at the start of every time step,  assemble(V, non_orth, rep)
-> (diag, source) of fvm::ddt(T) for one assembly (rep counts the assemblies of a repeated first corrector), state() -> what a recorded system
keeps of it.  Euler (through the oracle) is here; backward and CrankNicolson restate the reference in numpy and live beside their restatements
(test_backward_ddt.BackwardDdt, test_crank_nicolson.CrankNicolsonDdt)."""
import os
from types import SimpleNamespace

import numpy as np

from test_polymesh import LINE, geometry


class EulerDdt:
    def __init__(self, orc):
        self.orc = orc

    def start_step(self, step, dts, Told):
        self.rdt, self.Told = 1.0 / dts[step], Told

    def assemble(self, V, non_orth, rep):
        return self.orc.fvm_ddt_euler(self.rdt, 1.0, V, self.Told)

    def state(self):
        return {}


def walk(pkg, orc, pts, faces, owner, neighbour, patches, tin, T0, DT, dts, scheme="linear", correction=None, n_non_orth=0, ddt=None, repeat_at=()):
    """dts: one step size per time step.  scheme: div(phi,T) `Gauss` linear | upwind | limitedLinear k.  correction: the explicit part of the
    Laplacian -- None (uncorrected), "corrected", or ("limited", k) through the restatement of test_limited_sngrad.py.  ddt: a time scheme
    object, None: Euler.  repeat_at: steps whose first assembly is formed twice (a scheme with state must give the same again).
    -> lines (the solver lines), T, mesh (G, n, nI, lo, up, phi, P: what a test needs to pose the same system to the engine), systems (per
    time step the first corrector's system before the Laplacian's explicit part and the patches, with the scheme's state()), limited_share
    (("limited", k): the share of faces with limiter < 1 over the run)"""
    syn = pkg.synthetic
    ddt = EulerDdt(orc) if ddt is None else ddt
    limited_lap = correction is not None and correction != "corrected"
    if limited_lap:
        from test_limited_sngrad import limited_flux
    G = geometry(pts, faces, owner, neighbour)
    n, nI = int(owner.max()) + 1, len(neighbour)
    lo, up = owner[:nI].astype(np.int32), neighbour.astype(np.int32)
    V, lam, delta, magSf = G["V"], G["weights"], G["delta"], G["magSf"][:nI]
    Sf = [np.ascontiguousarray(G["Sf"][:nI, k]) for k in range(3)]
    centres = [np.ascontiguousarray(G["C"][:, k]) for k in range(3)]
    nhat = G["Sf"][:nI] / magSf[:, None]
    cv = nhat - (G["C"][up] - G["C"][lo]) * delta[:, None]
    cv = [np.ascontiguousarray(cv[:, k]) for k in range(3)]
    u0 = np.array([1.0, 0.2, 0.0])
    U = [np.full(n, u0[k]) for k in range(3)]
    phi = orc.flux_div(n, lo, up, lam, Sf, U, want_div=False)
    P = []
    for name, ptype, cnt, start in patches:
        fc = owner[start:start + cnt].astype(np.int32)
        sfb = G["Sf"][start:start + cnt]
        ub = np.tile(u0, (cnt, 1)) if name in ("inlet", "outlet") else np.zeros((cnt, 3))
        phib = ub[:, 0] * sfb[:, 0] + ub[:, 1] * sfb[:, 1] + ub[:, 2] * sfb[:, 2]
        diff = DT * G["magSf"][start:start + cnt] * G["delta_b"][start - nI:start - nI + cnt]
        fixed = name == "inlet"
        tb = tin if fixed else None
        P.append(dict(fc=fc, sf=[np.ascontiguousarray(sfb[:, k]) for k in range(3)], tb=tb,
                      ic=diff if fixed else phib, bc=(diff * tb - phib * tb) if fixed else np.zeros(cnt)))

    def grad(T):
        g = orc.gauss_grad(n, lo, up, Sf, orc.face_interpolate(lo, up, lam, T), None)
        for q in P:
            for k in range(3):
                g[k] = orc.patch_add_product(q["fc"], q["sf"][k], T[q["fc"]] if q["tb"] is None else q["tb"], g[k], 0)
        return [x / V for x in g]

    T = T0.copy()
    uL, dL = orc.fvm_laplacian(n, lo, up, delta, DT * magSf)
    lines, systems, limited, total = [], [], 0, 0
    for step in range(len(dts)):
        ddt.start_step(step, dts, T.copy())
        for non_orth in range(n_non_orth + 1):
            gT = grad(T) if (correction is not None or scheme.startswith("limitedLinear")) else None
            if scheme == "upwind":
                w = orc.upwind_weights(phi)
            elif scheme.startswith("limitedLinear"):
                w, _ = orc.limited_linear_weights(lo, up, float(scheme.split()[1]), lam, phi, T, gT, centres)
            else:
                w = lam
            lB, uB, dB = orc.fvm_div(n, lo, up, w, phi)
            for rep in range(2 if (step in repeat_at and non_orth == 0) else 1):
                dD, sD = ddt.assemble(V, non_orth, rep)
            lower, upper, diag, source = lB - uL, uB - uL, (dD + dB) - dL, sD
            if non_orth == 0:
                systems.append(dict(lower=lower, upper=upper, diag=diag, source=source, **ddt.state()))
            if correction is not None:
                if limited_lap:
                    (cf,), lim = limited_flux(orc, lo, up, correction[1], cv, lam, delta, [T], gT, -(DT * magSf))
                    limited += int(np.sum(lim < 1.0)); total += nI
                else:
                    cf = orc.sngrad_correction_flux(lo, up, cv, lam, gT, -(DT * magSf))
                source = orc.submul(V, orc.surface_integrate(n, lo, up, cf, V), source)
            for q in P:
                diag = orc.patch_add(q["fc"], q["ic"], diag, 0); source = orc.patch_add(q["fc"], q["bc"], source, 0)
            T, perf = orc.System([syn.LduCase(n, lo, up, diag, upper, lower, source)]).pbicg(T, source, "AINV", tolerance=1e-10, relTol=0.0)
            lines.append(("AINVPBiCG", "T", perf["initialResidual"], perf["finalResidual"], perf["nIterations"]))
    return SimpleNamespace(lines=lines, T=T, mesh=dict(G=G, n=n, nI=nI, lo=lo, up=up, phi=phi, P=P), systems=systems, limited_share=limited / max(total, 1))


def solver_lines(stdout):
    """(solver, field, initial residual, final residual, iterations) of every solver line of an application's log"""
    return [(m.group(1), m.group(2), float(m.group(3)), float(m.group(4)), int(m.group(5))) for m in map(LINE.match, stdout.splitlines()) if m]


def assert_solver_lines(got, ref):
    """an application's solver lines against a walk's: names and iteration counts equal, the residuals to the bars every application test uses"""
    for g, r in zip(got, ref):
        assert g[:2] == r[:2] and g[4] == r[4], (g, r)
        assert abs(g[2] - r[2]) <= 1e-7 * max(r[2], 1e-12) + 1e-14 and abs(g[3] - r[3]) <= 1e-6 * max(r[2], 1e-12) + 1e-14, (g, r)


def rewrite_schemes(case_dir, *replacements):
    """system/fvSchemes of a written case with every (old, new) applied; each old text must be there"""
    path = os.path.join(case_dir, "system", "fvSchemes")
    text = open(path).read()
    for old, new in replacements:
        assert old in text
        text = text.replace(old, new)
    open(path, "w").write(text)
