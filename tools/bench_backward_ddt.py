"""The backward time scheme beside Euler on the 216^3 box, device events on the engine's stream, every variant timed in turn in each round
(all in one process):
  (i)   the fused momentum-like assembly -- ddt(rho, U) + div(phi, U) [upwind] - laplacian(mu, U), three right-hand sides, sumMagOffDiag --
        with the backward time derivative (mi_fvm_assemble_backward) beside Euler's (mi_fvm_assemble), in the caller's numbering (fixed
        blocks) and under ordered addressing (blocks = the layout's tiles);
  (ii)  fvc::ddtCorr(rho, U, phi): mi_ddt_phi_corr_backward beside mi_ddt_phi_corr;
  (iii) with --parent-lib PATH: the Euler assembly of another build of the library (the parent commit's, built to a side directory), its own
        context and addressing, in the same rounds.
Every Euler variant is timed TWICE per round (A, B): the spread between two alternated runs of identical code is the margin the comparisons
are judged within.
Algorithmic bytes (every array once; tools/bench_assembly.py's Euler formulas plus 8N per old-old field and 8N for rho00):
  assembly  Euler 40F + 88N      backward 40F + 120N   (three old-old fields, rho00)
  ddtCorr   Euler 48F + 32N      backward 56F + 64N    (phi00; U00 x3, rho00)
Prints the result as one JSON line; `--out FILE` also writes it there."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, nargs=3, default=[216, 216, 216])
ap.add_argument("--reps", type=int, default=9, help="rounds; each round times every variant once, in turn")
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--parent-lib", default=None, help="another build of librapidcfd_amd.so whose Euler assembly is timed in the same rounds")
ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
args = ap.parse_args()

graft.build()
pkg = graft.load_package()
syn, eng = pkg.synthetic, pkg.engine
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
this_lib = eng.lib()


class use_lib:
    """the wrappers of engine.py resolve the library at every call: inside this block they call `lib`"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        eng._lib = self.lib

    def __exit__(self, *exc):
        eng._lib = this_lib


T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
E = lambda n: torch.empty(n, dtype=torch.float64, device=dev)
case = syn.box_case(*args.dims)
N, F = case.n_cells, case.n_faces
u = syn.splitmix_uniform
flux, delta, gamma, lam = T(u(2, F) - 0.5), T(u(3, F)), T(u(23, F)), T(u(20, F))
Sf = [T(u(10 + k, F)) for k in range(3)]
vol, rho, rho0, rho00 = T(np.full(N, 1.0)), T(0.8 + u(21, N)), T(0.8 + u(31, N)), T(0.8 + u(32, N))
U0, U00 = [T(u(24 + k, N) - 0.5) for k in range(3)], [T(u(27 + k, N) - 0.5) for k in range(3)]
phi0, phi00 = T(u(33, F) - 0.5), T(u(34, F) - 0.5)
lower, upper, diag, mag, srcs, fout = E(F), E(F), E(N), E(N), [E(N) for _ in range(3)], E(F)
coeffs = eng.ddt_backward_coeffs(1e-4, 1.25e-4)
EULER = dict(r_delta_t=1e4, vol=vol, psi_old=U0, rho=rho, rho_old=rho0)
BACK = dict(EULER, backward=dict(coeffs=coeffs, psi_old_old=U00, rho_old_old=rho00))


def assemble(asm, ddt):
    return lambda: asm.assemble(upper, diag, lower_out=lower, sources_out=srcs, ddt=ddt, div=dict(flux=flux),
                                laplacian=dict(delta_coeffs=delta, gamma_magsf=gamma), sum_mag_out=mag)


ctx = eng.Context(0, stream.cuda_stream)
a0 = eng.Addressing(ctx, N, case.lower_addr, case.upper_addr)
rc = syn.renumber(case, a0.cell_perm())
a1 = eng.Addressing(ctx, N, rc.lower_addr, rc.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
asm0, asm1 = eng.Assembly(a0), eng.Assembly(a1)
B_E, B_B = 40 * F + 88 * N, 40 * F + 120 * N
variants = {}   # name -> (fn, bytes, library)
for tag, asm in (("caller numbering", asm0), ("ordered addressing", asm1)):
    variants[f"assemble Euler A [{tag}]"] = (assemble(asm, EULER), B_E, this_lib)
    variants[f"assemble backward [{tag}]"] = (assemble(asm, BACK), B_B, this_lib)
    variants[f"assemble Euler B [{tag}]"] = (assemble(asm, EULER), B_E, this_lib)
variants["ddtCorr Euler A"] = (lambda: asm0.ddt_phi_corr(1e4, lam, Sf, U0, rho0, phi0, fout), 48 * F + 32 * N, this_lib)
variants["ddtCorr backward"] = (lambda: asm0.ddt_phi_corr_backward(1e4, coeffs, lam, Sf, U0, U00, rho0, rho00, phi0, phi00, fout), 56 * F + 64 * N, this_lib)
variants["ddtCorr Euler B"] = (lambda: asm0.ddt_phi_corr(1e4, lam, Sf, U0, rho0, phi0, fout), 48 * F + 32 * N, this_lib)
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.mi_last_error.restype = ctypes.c_char_p
    with use_lib(parent):
        pctx = eng.Context(0, stream.cuda_stream)
        pa0 = eng.Addressing(pctx, N, case.lower_addr, case.upper_addr)
        pa1 = eng.Addressing(pctx, N, rc.lower_addr, rc.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
    for tag, pa in (("caller numbering", pa0), ("ordered addressing", pa1)):
        variants[f"assemble Euler, parent library [{tag}]"] = (assemble(eng.Assembly(pa), EULER), B_E, parent)

times = {k: [] for k in variants}
for fn, _, lib in variants.values():
    with use_lib(lib):
        fn()
torch.cuda.synchronize()
for _ in range(args.reps):
    for name, (fn, _, lib) in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with use_lib(lib):
            a.record(stream)
            for _ in range(args.iters):
                fn()
            b.record(stream)
        b.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
res = {}
for name, (_, nbytes, _) in variants.items():
    us = statistics.median(times[name])
    res[name] = dict(us=round(us, 1), min_us=round(min(times[name]), 1), max_us=round(max(times[name]), 1), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3))


def ratio(a, b):
    """median over rounds of the per-round ratio a/b"""
    return round(statistics.median([x / y for x, y in zip(times[a], times[b])]), 4)


cmp = {}
for tag in ("caller numbering", "ordered addressing"):
    cmp[f"identical code, Euler B / Euler A [{tag}]"] = ratio(f"assemble Euler B [{tag}]", f"assemble Euler A [{tag}]")
    cmp[f"backward / Euler A, time [{tag}]"] = ratio(f"assemble backward [{tag}]", f"assemble Euler A [{tag}]")
    cmp[f"backward / Euler A, fraction of 8 TB/s [{tag}]"] = round(res[f"assemble backward [{tag}]"]["frac_8TBs"] / res[f"assemble Euler A [{tag}]"]["frac_8TBs"], 4)
    if args.parent_lib:
        cmp[f"Euler A / parent library [{tag}]"] = ratio(f"assemble Euler A [{tag}]", f"assemble Euler, parent library [{tag}]")
cmp["identical code, ddtCorr Euler B / Euler A"] = ratio("ddtCorr Euler B", "ddtCorr Euler A")
cmp["ddtCorr backward / Euler A, time"] = ratio("ddtCorr backward", "ddtCorr Euler A")
cmp["ddtCorr backward / Euler A, fraction of 8 TB/s"] = round(res["ddtCorr backward"]["frac_8TBs"] / res["ddtCorr Euler A"]["frac_8TBs"], 4)
line = json.dumps(dict(tool="bench_backward_ddt", dims=args.dims, cells=N, faces=F, reps=args.reps, iters=args.iters,
                       parent_library=bool(args.parent_lib), variants=res, comparisons=cmp))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
