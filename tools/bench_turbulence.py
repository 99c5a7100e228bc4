"""The kEpsilon passes on the device (mi_ke_production, mi_ke_epsilon_terms, mi_ke_k_terms, mi_ke_nut, mi_fvc_average, mi_bound, mi_ke_wall_cells,
mi_ke_nut_wall, mi_min_max, mi_vec_max_value) on the 216^3 box renumbered into the engine's tile order (ordered addressing), with the three
boundary patches of tools/bench_mules.py, all of them walls -- device events on the engine's stream; in each round every variant is timed in
turn, all in one process, so the compared runs alternate.  Every yardstick is composed of entries the engine had before these passes; what such
a composition cannot express (a face product, the max) is left out of ITS figure, which flatters the yardstick.  The one cell product the
earlier entries can form is mi_vec_submul on a zeroed array: that zero fill (a memset) and mi_vec_submul's read of its in-out array are
part of the composition, are timed with it and are counted in its bytes:
  nut            against zero fill + mi_vec_submul (k*k) + mi_vec_axpby (Cmu) + mi_vec_div
  k terms        against mi_vec_div + mi_vec_axpby
  epsilon terms  against zero fill + mi_vec_submul + mi_vec_axpby + mi_vec_div (su), mi_vec_axpby + mi_vec_div (sp), mi_vec_axpby (deps)
  fvc_average    against mi_surface_sum + mi_patch_add per patch + mi_vec_div (the products magSf*ssf are not in the figure)
  bound          against mi_face_interpolate + the same (the two max passes, the product and the cell algebra are not in the figure)
  wall cells     against mi_patch_add per patch for G and for epsilon (forming the face values and the boundary assignment are not in the figure)
  min_max        beside mi_sum, the engine's reduction over the same array
  production and nut on the walls have no composition among the earlier entries: time and share of 8 TB/s only.
Algorithmic bytes (every array once; row tables and boundary lists not counted; b = per boundary face, w = per wall cell):
  production 88N; epsilon terms 64N (nu a field); k terms 48N; nut 24N; max 16N; min_max 8N
  the compositions: zero fill 8N, mi_vec_submul 32N, mi_vec_axpby in place 16N or with two inputs 24N, mi_vec_div 24N
  fvc_average 16F + 16N + 16b; bound 16F + 32N + 16b (+ 16N for the copy back); wall cells 80w + 72b; nut on the walls 40b
Prints one JSON line as tools/bench_interface.py does.  `--reps 2 --iters 3` for a run under a profiler."""
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
cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
gen = torch.Generator(device=dev).manual_seed(11)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
Kc = eng.ke_coeffs()
k, eps, nut, nu_f, G = R(N, 0.01, 1.0), R(N, 0.1, 10.0), R(N, 1e-4, 1e-2), R(N, 0.5e-5, 1.5e-5), R(N)
grad = [R(N, -10.0, 10.0) for _ in range(9)]
U = [R(N, -0.5, 0.5) for _ in range(3)]
lam, magSf, ssf = R(F, 0.3, 0.7), R(F, 0.5, 1.5), R(F, -0.5, 0.5)
bms, bssf, bdc, bnuw, bnutw = R(NB, 0.5, 1.5), R(NB, -0.5, 0.5), R(NB, 50.0, 150.0), R(NB, 0.5e-5, 1.5e-5), R(NB, 0.0, 1e-4)
Uw = [R(NB, -0.1, 0.1) for _ in range(3)]
bc = torch.from_numpy(np.concatenate(fcs).astype(np.int64)).to(dev)
by = Kc.yPlusLam * torch.exp(2.0 * (R(NB) - 0.5)) * bnuw / (Kc.Cmu25 * torch.sqrt(k[bc]))      # yPlus on both sides of yPlusLam
v = R(N, -0.3, 1.0)                                       # what bound sees: three cells in thirteen negative
v0 = v.clone()
bface = R(NB, 1e-15, 1.0)
AV = eng.Average(addr, B, magSf, bms)
KE = eng.KEpsilon(addr, B, [True] * 3)
NW = KE.wall_cell_labels().numel()
out = [E(N) for _ in range(3)]
t1, t2, m, face, avg, avg2 = E(N), E(N), E(N), E(F), E(N), E(N)
Gw, epsw, beps, bnut = G.clone(), eps.clone(), E(NB), E(NB)
bvals = [R(fc.shape[0]) for fc in fcs]
lib, cx, ptr, I64 = eng.lib(), ctx.h, eng._ptr, C.c_int64(N)


def vec_div(x, y, o):
    eng._chk(lib.mi_vec_div(cx, I64, ptr(x), ptr(y), ptr(o)))


def unfused_nut():
    t1.zero_()
    asm.submul(k, k, t1)
    asm.axpby(-Kc.Cmu, t1, 0.0, t1, t1)
    vec_div(t1, eps, out[0])


def unfused_k_terms():
    vec_div(eps, k, out[0])
    asm.axpby(1.0, nut, 1.0, nu_f, out[1])


def unfused_epsilon_terms():
    t1.zero_()
    asm.submul(G, eps, t1)
    asm.axpby(-Kc.C1, t1, 0.0, t1, t1)
    vec_div(t1, k, out[0])
    asm.axpby(Kc.C2, eps, 0.0, eps, t2)
    vec_div(t2, k, out[1])
    asm.axpby(1.0 / Kc.sigmaEps, nut, 1.0, nu_f, out[2])


def unfused_average(field=ssf):
    asm.surface_sum(field, avg2)
    for p, b in zip(patches, bvals):
        p.add(b, avg2)
    vec_div(avg2, t2, avg2)


def unfused_bound():
    asm.face_interpolate(lam, v0, face)
    unfused_average(face)


def unfused_wall_sums():
    for p, b in zip(patches, bvals):
        p.add(b, Gw)
        p.add(b, epsw)


def bound():
    v.copy_(v0)                                           # the field is bounded in place: start from the same values every time
    asm.bound(AV, 1e-15, lam, magSf, v, bms, bface)


def total(x):
    s = C.c_double(0.0)
    eng._chk(lib.mi_sum(cx, ptr(x), I64, C.byref(s)))


names = dict(nut="zero fill + submul + axpby + vec_div", kt="vec_div + axpby", et="zero fill + submul + 3 axpby + 2 vec_div", av="surface_sum + patch_add x 3 + vec_div",
             bd="face_interpolate + surface_sum + patch_add x 3 + vec_div", ws="patch_add x 3 for G and for epsilon", rs="mi_sum", cp="copy of a cell array")
yard_bytes = {names["nut"]: (8 + 32 + 16 + 24) * N, names["kt"]: 24 * N + 24 * N, names["et"]: (8 + 32 + 16 + 24 + 16 + 24 + 24) * N,
              names["av"]: 8 * F + 8 * N + 24 * NB + 24 * N, names["bd"]: 16 * F + 8 * N + 8 * F + 8 * N + 24 * NB + 24 * N,
              names["ws"]: 2 * (8 * NB + 16 * NW), names["rs"]: 8 * N, names["cp"]: 16 * N}
# name -> (call, bytes, yardstick)
variants = {
    names["nut"]: (unfused_nut, yard_bytes[names["nut"]], names["nut"]),
    names["kt"]: (unfused_k_terms, yard_bytes[names["kt"]], names["kt"]),
    names["et"]: (unfused_epsilon_terms, yard_bytes[names["et"]], names["et"]),
    names["av"]: (unfused_average, yard_bytes[names["av"]], names["av"]),
    names["bd"]: (unfused_bound, yard_bytes[names["bd"]], names["bd"]),
    names["ws"]: (unfused_wall_sums, yard_bytes[names["ws"]], names["ws"]),
    names["rs"]: (lambda: total(v0), yard_bytes[names["rs"]], names["rs"]),
    names["cp"]: (lambda: v.copy_(v0), yard_bytes[names["cp"]], names["cp"]),
    "ke_nut": (lambda: asm.ke_nut(Kc.Cmu, k, eps, out[0]), 24 * N, names["nut"]),
    "ke_k_terms": (lambda: asm.ke_k_terms(eps, k, nut, nu_f, out[0], out[1]), 48 * N, names["kt"]),
    "ke_epsilon_terms": (lambda: asm.ke_epsilon_terms(Kc, G, eps, k, nut, nu_f, *out), 64 * N, names["et"]),
    "ke_production": (lambda: asm.ke_production(nut, grad, out[0]), 88 * N, names["cp"]),
    "vec_max_value": (lambda: asm.vec_max_value(v0, 1e-15, m), 16 * N, names["cp"]),
    "min_max": (lambda: asm.min_max(v0), 8 * N, names["rs"]),
    "fvc_average": (lambda: asm.fvc_average(AV, magSf, ssf, avg, bms, bssf), 16 * F + 16 * N + 16 * NB, names["av"]),
    "bound (with the copy that restores its input)": (bound, 16 * F + 48 * N + 16 * NB + 16 * N, names["bd"]),
    "ke_wall_cells": (lambda: asm.ke_wall_cells(KE, Kc, k, U, Uw, bdc, by, bnuw, bnutw, Gw, epsw, beps), 80 * NW + 72 * NB, names["ws"]),
    "ke_nut_wall": (lambda: asm.ke_nut_wall(KE, Kc, k, by, bnuw, bnut), 40 * NB, names["ws"]),
}
asm.surface_sum(magSf, t2)                                # the yardstick's surfaceSum(magSf), formed once as the handle forms its own
for p, fc, a, b in zip(patches, fcs, cut[:-1], cut[1:]):
    p.add(bms[a:b].clone(), t2)
times = {name: [] for name in variants}
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
line = json.dumps(dict(tool="bench_turbulence", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB,
                       wall_cells=NW, reps=args.reps, iters=args.iters, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
KE.close()
AV.close()
B.close()
