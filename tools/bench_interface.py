"""interfaceProperties on the device (mi_interface_nhatf, mi_interface_curvature, mi_surface_tension_force, mi_near_interface) on the 216^3 box
renumbered into the engine's tile order (ordered addressing), with the three boundary patches of tools/bench_mules.py -- device events on the
engine's stream; in each round every variant is timed in turn, all in one process, so the compared runs alternate.  Every yardstick is an entry
the engine had before these passes:
  nHatf       against the three mi_face_interpolate calls the unfused sequence BEGINS with (it goes on with mag, + deltaN, the vector division
              and the dot with Sf, which are not entries of the engine and are not in the figure)
  curvature   against mi_surface_integrate + mi_patch_add per patch + mi_vec_div on the same inputs (the negation is not in the figure)
  force       beside mi_alpha_compression_flux, the gathering face pass of the same size
Algorithmic bytes (every array once, owner / neighbour counted for the face passes; row tables and boundary lists not counted; b = per boundary face):
  nHatf                      lambda, Sf read, nHatf written 40F, owner / neighbour 8F, the gradient gathered 24N      -> 48F + 24N  (+ 24F with nHatfv)
  three mi_face_interpolate  3 x (lambda read, out written 16F, owner / neighbour 8F, one cell array gathered 8N)    -> 72F + 24N
  curvature                  nHatf 8F; V read, K written 16N; 8b
  integrate + add + div      8F + 8N; per patch 8b and its cells read and written; 24N
  surface tension force      lambda, deltaCoeffs read, out written 24F, owner / neighbour 8F, K and alpha gathered 16N (+ 8F with the correction)
  mi_alpha_compression_flux  24F + 8F + 8N
Prints one JSON line as tools/bench_cmules.py does.  `--reps 2 --iters 3` for a run under a profiler."""
import argparse
import ctypes as C
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
ap.add_argument("--reps", type=int, default=5, help="rounds; each round times every variant once, in turn")
ap.add_argument("--iters", type=int, default=100, help="calls per timed window")
ap.add_argument("--caller", action="store_true", help="the caller's numbering as it is (fixed blocks of cells) instead of ordered addressing")
ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
args = ap.parse_args()

graft.build()
pkg = graft.load_package()
syn, eng = pkg.synthetic, pkg.engine
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = eng.Context(0, stream.cuda_stream)
case = syn.box_case(*args.dims)
if args.caller:
    addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
else:
    a0 = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
    case = syn.renumber(case, a0.cell_perm())
    addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
    assert addr.is_ordered
N, F = case.n_cells, case.n_faces
lo, up = case.lower_addr, case.upper_addr
asm = eng.Assembly(addr)
missing = 6 - (np.bincount(lo, minlength=N) + np.bincount(up, minlength=N))
fcs = [np.nonzero(missing > k)[0].astype(np.int32) for k in range(3)]
B = eng.GradBoundary(addr, fcs, ["other"] * 3)
NB = B.n_faces
patches = [eng.Patch(ctx, N, fc) for fc in fcs]
H = eng.Interface(addr, B)
gen = torch.Generator(device=dev).manual_seed(7)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
vol = R(N, 0.5, 1.5)
delta_n = 1e-8 / float(vol.mean()) ** (1.0 / 3.0)
alpha = R(N)
grad = [R(N, -10.0, 10.0) for _ in range(3)]
pick = R(N)
for g in grad:                                           # away from the interface the gradient is exactly zero
    g[pick < 0.5] = 0.0
del pick
lam, dc, corr, cdw, phir = R(F, 0.3, 0.7), R(F, 0.5, 1.5), R(F, -0.5, 0.5), R(F, 0.3, 0.7), R(F, -0.75, 0.75)
Sf = [R(F, -0.5, 0.5) for _ in range(3)]
gf, nv = [E(F) for _ in range(3)], [E(F) for _ in range(3)]
nhatf, force, fused = E(F), E(F), E(F)
bn = R(NB, -0.5, 0.5)
bn_p, off = [], 0
for fc in fcs:
    bn_p.append(bn[off:off + fc.shape[0]].clone())
    off += fc.shape[0]
K, K2, ni = E(N), E(N), E(N)
asm.interface_nhatf(delta_n, lam, Sf, grad, nhatf)
sigma = 0.07


def three_interpolates():
    for k in range(3):
        asm.face_interpolate(lam, grad[k], gf[k])


def unfused_curvature():
    asm.surface_integrate(nhatf, None, K2)
    for p, b in zip(patches, bn_p):
        p.add(b, K2)
    eng._chk(eng.lib().mi_vec_div(ctx.h, C.c_int64(N), eng._ptr(K2), eng._ptr(vol), eng._ptr(K2)))


interp, unf, comp = "three mi_face_interpolate", "surface_integrate + patch_add x 3 + vec_div", "mi_alpha_compression_flux"
yard_bytes = {interp: 72 * F + 24 * N, unf: 8 * F + 32 * N + 24 * NB, comp: 32 * F + 8 * N}
# name -> (call, bytes, yardstick)
variants = {
    interp: (three_interpolates, yard_bytes[interp], interp),
    unf: (unfused_curvature, yard_bytes[unf], unf),
    comp: (lambda: asm.alpha_compression_flux(cdw, phir, alpha, fused), yard_bytes[comp], comp),
    "interface_nhatf": (lambda: asm.interface_nhatf(delta_n, lam, Sf, grad, nhatf), 48 * F + 24 * N, interp),
    "interface_nhatf with nHatfv": (lambda: asm.interface_nhatf(delta_n, lam, Sf, grad, nhatf, nv), 72 * F + 24 * N, interp),
    "interface_curvature": (lambda: asm.interface_curvature(H, nhatf, vol, K, bn), 8 * F + 16 * N + 8 * NB, unf),
    "surface_tension_force": (lambda: asm.surface_tension_force(sigma, lam, dc, K, alpha, force), 32 * F + 16 * N, comp),
    "surface_tension_force with corr": (lambda: asm.surface_tension_force(sigma, lam, dc, K, alpha, force, corr), 40 * F + 16 * N, comp),
    "near_interface": (lambda: asm.near_interface(alpha, ni), 16 * N, comp),
}
times = {k: [] for k in variants}
for fn, _, _ in variants.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
for _ in range(args.reps):
    for name, (fn, _, _) in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.iters):
            fn()
        b.record(stream)
        b.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
res = {}
for name, (_, nbytes, yard) in variants.items():
    us = statistics.median(times[name])
    res[name] = dict(us=round(us, 1), spread=round((max(times[name]) - min(times[name])) / us, 3), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3), yardstick=yard,
                     ratio_to_yardstick=round(statistics.median([x / x0 for x, x0 in zip(times[name], times[yard])]), 3),
                     byte_ratio=round(nbytes / yard_bytes[yard], 3))
same_K = bool(torch.equal(K.view(torch.int64), (-K2).view(torch.int64)))     # the fused curvature is the unfused sequence with the sign flipped
line = json.dumps(dict(tool="bench_interface", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB,
                       reps=args.reps, iters=args.iters, curvature_equals_unfused_bits=same_K, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
H.close()
B.close()
