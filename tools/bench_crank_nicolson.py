"""The CrankNicolson time scheme beside Euler and backward on the 216^3 box, device events on the engine's stream, every variant timed in
turn in each round (all in one process):
  (i)   the fused momentum-like assembly -- ddt(rho, U) + div(phi, U) [upwind] - laplacian(mu, U), three right-hand sides, sumMagOffDiag --
        with the CrankNicolson time derivative (mi_fvm_assemble_cn) beside Euler's (mi_fvm_assemble) and backward's
        (mi_fvm_assemble_backward), in the caller's numbering (fixed blocks) and under ordered addressing (blocks = the layout's tiles);
  (ii)  the evaluate-once ddt0 update of the three components in one launch (mi_ddt_cn_update, density field);
  (iii) with --parent-lib PATH: the Euler, backward and CrankNicolson assemblies of another build of the library (the parent commit's, built to a side
        directory), its own context and addressing, in the same rounds.
The Euler assembly is timed TWICE per round (A, B): the spread between two alternated runs of identical code is the margin the comparisons
are judged within.
Algorithmic bytes (every array once; tools/bench_assembly.py's Euler formulas):
  assembly  Euler 40F + 88N      CrankNicolson 40F + 112N  (one ddt0 field per right-hand side: 8 n_rhs bytes per cell)
            backward 40F + 120N  (three old-old fields, rho00)
  update    112N                 (ddt0 read and written, U0, U00: 3 x 32N; rho0, rho00: 16N)
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
ap.add_argument("--parent-lib", default=None, help="another build of librapidcfd_amd.so whose Euler, backward and CrankNicolson assemblies are timed in the same rounds")
ap.add_argument("--reverse", action="store_true", help="time the variants of a round in the reverse order")
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
flux, delta, gamma = T(u(2, F) - 0.5), T(u(3, F)), T(u(23, F))
vol, rho, rho0, rho00 = T(np.full(N, 1.0)), T(0.8 + u(21, N)), T(0.8 + u(31, N)), T(0.8 + u(32, N))
U0, U00 = [T(u(24 + k, N) - 0.5) for k in range(3)], [T(u(27 + k, N) - 0.5) for k in range(3)]
ddt0, ddt0w = [T(u(35 + k, N) - 0.5) for k in range(3)], [torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(3)]
lower, upper, diag, mag, srcs = E(F), E(F), E(N), E(N), [E(N) for _ in range(3)]
OC = 0.9
coeffs = eng.ddt_backward_coeffs(1e-4, 1.25e-4)
EULER = dict(r_delta_t=1e4, vol=vol, psi_old=U0, rho=rho, rho_old=rho0)
BACK = dict(EULER, backward=dict(coeffs=coeffs, psi_old_old=U00, rho_old_old=rho00))
CN = dict(EULER, r_delta_t=1.9e4, crank_nicolson=dict(oc=OC, ddt0=ddt0))


def assemble(asm, ddt):
    return lambda: asm.assemble(upper, diag, lower_out=lower, sources_out=srcs, ddt=ddt, div=dict(flux=flux),
                                laplacian=dict(delta_coeffs=delta, gamma_magsf=gamma), sum_mag_out=mag)


ctx = eng.Context(0, stream.cuda_stream)
a0 = eng.Addressing(ctx, N, case.lower_addr, case.upper_addr)
rc = syn.renumber(case, a0.cell_perm())
a1 = eng.Addressing(ctx, N, rc.lower_addr, rc.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
asm0, asm1 = eng.Assembly(a0), eng.Assembly(a1)
B_E, B_B, B_C = 40 * F + 88 * N, 40 * F + 120 * N, 40 * F + 112 * N
variants = {}   # name -> (fn, bytes, library)
for tag, asm in (("caller numbering", asm0), ("ordered addressing", asm1)):
    variants[f"assemble Euler A [{tag}]"] = (assemble(asm, EULER), B_E, this_lib)
    variants[f"assemble CrankNicolson [{tag}]"] = (assemble(asm, CN), B_C, this_lib)
    variants[f"assemble backward [{tag}]"] = (assemble(asm, BACK), B_B, this_lib)
    variants[f"assemble Euler B [{tag}]"] = (assemble(asm, EULER), B_E, this_lib)
# (the update runs in place on arrays of its own, which start at zero: with oc < 1 and bounded inputs the repeated update stays bounded)
variants["ddt0 update, three fields"] = (lambda: asm0.ddt_cn_update(1.9e4, OC, U0, U00, ddt0w, rho_old=rho0, rho_old_old=rho00), 112 * N, this_lib)
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.mi_last_error.restype = ctypes.c_char_p
    with use_lib(parent):
        pctx = eng.Context(0, stream.cuda_stream)
        pa0 = eng.Addressing(pctx, N, case.lower_addr, case.upper_addr)
        pa1 = eng.Addressing(pctx, N, rc.lower_addr, rc.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
    for tag, pa in (("caller numbering", pa0), ("ordered addressing", pa1)):
        variants[f"assemble Euler, parent library [{tag}]"] = (assemble(eng.Assembly(pa), EULER), B_E, parent)
        variants[f"assemble backward, parent library [{tag}]"] = (assemble(eng.Assembly(pa), BACK), B_B, parent)
        variants[f"assemble CrankNicolson, parent library [{tag}]"] = (assemble(eng.Assembly(pa), CN), B_C, parent)
if args.reverse:
    variants = dict(reversed(list(variants.items())))

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
    cmp[f"CrankNicolson / Euler A, time [{tag}]"] = ratio(f"assemble CrankNicolson [{tag}]", f"assemble Euler A [{tag}]")
    cmp[f"CrankNicolson / Euler A, algorithmic bytes [{tag}]"] = round(B_C / B_E, 4)
    cmp[f"CrankNicolson / Euler A, fraction of 8 TB/s [{tag}]"] = round(res[f"assemble CrankNicolson [{tag}]"]["frac_8TBs"] / res[f"assemble Euler A [{tag}]"]["frac_8TBs"], 4)
    if args.parent_lib:
        cmp[f"Euler A / parent library [{tag}]"] = ratio(f"assemble Euler A [{tag}]", f"assemble Euler, parent library [{tag}]")
        cmp[f"backward / parent library [{tag}]"] = ratio(f"assemble backward [{tag}]", f"assemble backward, parent library [{tag}]")
        cmp[f"CrankNicolson / parent library [{tag}]"] = ratio(f"assemble CrankNicolson [{tag}]", f"assemble CrankNicolson, parent library [{tag}]")
line = json.dumps(dict(tool="bench_crank_nicolson", dims=args.dims, cells=N, faces=F, reps=args.reps, iters=args.iters,
                       parent_library=bool(args.parent_lib), reverse=args.reverse, variants=res, comparisons=cmp))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
