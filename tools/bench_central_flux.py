"""rhoCentralFoam's flux evaluation on the device (mi_central_flux, mi_patch_central_flux, mi_central_sound_speed, mi_central_courant) on the
216^3 box renumbered into the engine's tile order (ordered addressing) -- device events on the engine's stream; in each round every variant is
timed in turn, all in one process, so the compared runs alternate.  No counters, no trace.  Every yardstick is made of entries the engine had
before these passes:
  central_flux      against the part of the unfused sequence those entries can form on the same box and inputs: ten mi_limited_weights calls
                    (eight scalar, two V; flux arrays of +1 and -1) followed by fourteen mi_face_interpolate calls.  It leaves out all of the
                    roughly forty-five algebra passes of rhoCentralFoam.C:107-185, so the fused pass has to stay below 1.0 x its time
  limited_weights   one mi_limited_weights call (vanLeer), the gathering face pass the fraction of 8 TB/s is read beside
  patch             the plain form on the largest boundary patch
  sound_speed       beside mi_vec_div
  courant           beside mi_sum over the stored product + mi_min_max over the stored quotient (internal and boundary faces in one array)
Algorithmic bytes (every array once; owner / neighbour counted for the face passes; b = per patch face):
  central_flux      cdw, Sf, magSf, owner / neighbour 48F; phi, phiUp, phiEp, amaxSf 48F; 7 fields, 21 gradient arrays, 3 centres gathered 248N
                    -> 96F + 248N (128F + 248N with a_pos and aU)
  unfused start     a scalar mi_limited_weights 32F + 56N, a V one 32F + 120N, mi_face_interpolate 24F + 8N -> 656F + 800N
Prints one JSON line and writes <out-dir>/central_flux.json and central_flux.md.  `--reps 2 --iters 3` for a run under a profiler."""
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
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--caller", action="store_true", help="the caller's numbering as it is (fixed blocks of cells) instead of ordered addressing")
ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"), help="where central_flux.json and central_flux.md go")
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
fc = np.nonzero(missing > 0)[0].astype(np.int32)
NB = fc.shape[0]
patch = eng.Patch(ctx, N, fc)
gen = torch.Generator(device=dev).manual_seed(11)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)

# a gas of both subsonic and supersonic faces: rho about 1, c about 340, |U| up to 600
rho, rPsi, e, c = R(N, 0.6, 1.4), R(N, 7.0e4, 9.0e4), R(N, 2.0e5, 3.0e5), R(N, 300.0, 380.0)
rhoU = [rho * R(N, -600.0, 600.0) for _ in range(3)]
g_rho, g_rPsi, g_e, g_c = [R(N, -1.0, 1.0) for _ in range(3)], [R(N, -2e4, 2e4) for _ in range(3)], [R(N, -1e5, 1e5) for _ in range(3)], [R(N, -50.0, 50.0) for _ in range(3)]
g_rhoU = [R(N, -1000.0, 1000.0) for _ in range(9)]
cc = [R(N) for _ in range(3)]
cdw, magSf = R(F, 0.3, 0.7), R(F, 0.5, 1.5)
Sf = [R(F, -0.5, 0.5) for _ in range(3)]
cells = eng.central_cells(rho=rho, rhoU=rhoU, rPsi=rPsi, e=e, c=c, grad_rho=g_rho, grad_rhoU=g_rhoU, grad_rPsi=g_rPsi, grad_e=g_e, grad_c=g_c)
o6 = dict(phi=E(F), phiUp=[E(F) for _ in range(3)], phiEp=E(F), amaxSf=E(F))
o10 = dict(o6, a_pos=E(F), aU=[E(F) for _ in range(3)])
out6, out10 = eng.central_out(**o6), eng.central_out(**o10)
kurganov = eng.central_scheme("Kurganov", "vanLeer", "vanLeerV", "vanLeer")
tadmor = eng.central_scheme("Tadmor", "vanLeer", "vanLeerV", "vanLeer")
mixed = eng.central_scheme("Kurganov", "vanAlbada", "MinmodV", "limitedVanLeer 0 260000")

# the unfused start
plus, minus = torch.ones(F, dtype=torch.float64, device=dev), -torch.ones(F, dtype=torch.float64, device=dev)
w_s, w_v, face = E(F), E(F), E(F)
van_leer, van_leer_v = eng.limiter("vanLeer"), eng.limiter("vanLeerV")
scalars = [(rho, g_rho), (rPsi, g_rPsi), (e, g_e), (c, g_c)]


def unfused_start():
    for fl in (plus, minus):
        for x, g in scalars:
            asm.limited_weights(van_leer, cdw, fl, [x], g, cc, w_s)
            asm.face_interpolate(w_s, x, face)
        asm.limited_weights(van_leer_v, cdw, fl, rhoU, g_rhoU, cc, w_v)
        for k in range(3):
            asm.face_interpolate(w_v, rhoU[k], face)


# the patch, the cell pass and the reduction
b_vals = dict(rho=R(NB, 0.6, 1.4), rhoU=[R(NB, -600.0, 600.0) for _ in range(3)], rPsi=R(NB, 7.0e4, 9.0e4), e=R(NB, 2.0e5, 3.0e5), c=R(NB, 300.0, 380.0))
b_cells = eng.central_cells(**b_vals)
b_sf, b_ms = [R(NB, -0.5, 0.5) for _ in range(3)], R(NB, 0.5, 1.5)
b_o = dict(phi=E(NB), phiUp=[E(NB) for _ in range(3)], phiEp=E(NB), amaxSf=E(NB))
b_out = eng.central_out(**b_o)
Cp, Cv, psi, rPsi2, c2, quot = R(N, 1000.0, 1010.0), R(N, 700.0, 730.0), R(N, 1.0e-5, 2.0e-5), E(N), E(N), E(N)
dc, b_dc = R(F, 0.5, 1.5), R(NB, 0.5, 1.5)
asm.central_flux(kurganov, cdw, Sf, magSf, cells, cc, out6)
patch.central_flux(kurganov, b_sf, b_ms, b_cells, b_out)
prod = dc * o6["amaxSf"]
both = torch.cat([prod / magSf, (b_dc * b_o["amaxSf"]) / b_ms])
vec_div = lambda: eng._chk(eng.lib().mi_vec_div(ctx.h, C.c_int64(N), eng._ptr(Cp), eng._ptr(Cv), eng._ptr(quot)))


def stored_reductions():
    ctx.sum(prod)
    asm.min_max(both)


start, one_w, div_n, red = "ten mi_limited_weights + fourteen mi_face_interpolate", "mi_limited_weights (vanLeer)", "mi_vec_div", "mi_sum + mi_min_max over stored products"
yard_bytes = {start: 656 * F + 800 * N, one_w: 32 * F + 56 * N, div_n: 24 * N, red: 16 * F + 8 * NB}
fused = 96 * F + 248 * N
# name -> (call, bytes, yardstick)
variants = {
    start: (unfused_start, yard_bytes[start], start),
    one_w: (lambda: asm.limited_weights(van_leer, cdw, plus, [rho], g_rho, cc, w_s), yard_bytes[one_w], one_w),
    div_n: (vec_div, yard_bytes[div_n], div_n),
    red: (stored_reductions, yard_bytes[red], red),
    "central_flux Kurganov": (lambda: asm.central_flux(kurganov, cdw, Sf, magSf, cells, cc, out6), fused, start),
    "central_flux Kurganov with a_pos and aU": (lambda: asm.central_flux(kurganov, cdw, Sf, magSf, cells, cc, out10), fused + 32 * F, start),
    "central_flux Tadmor": (lambda: asm.central_flux(tadmor, cdw, Sf, magSf, cells, cc, out6), fused, start),
    "central_flux vanAlbada / MinmodV / limitedVanLeer": (lambda: asm.central_flux(mixed, cdw, Sf, magSf, cells, cc, out6), fused, start),
    "patch_central_flux (plain)": (lambda: patch.central_flux(kurganov, b_sf, b_ms, b_cells, b_out), 136 * NB, one_w),
    "central_sound_speed": (lambda: asm.central_sound_speed(Cp, Cv, psi, rPsi2, c2), 40 * N, div_n),
    "central_courant": (lambda: asm.central_courant(dc, magSf, o6["amaxSf"], b_dc, b_ms, b_o["amaxSf"]), 24 * F + 24 * NB, red),
}
times = {k: [] for k in variants}
for fn, _, _ in variants.values():
    for _ in range(2):
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
asm.central_flux(kurganov, cdw, Sf, magSf, cells, cc, out6)            # the amaxSf the stored products were formed from
co = asm.central_courant(dc, magSf, o6["amaxSf"], b_dc, b_ms, b_o["amaxSf"])
result = dict(tool="bench_central_flux", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, patch_faces=NB,
              reps=args.reps, iters=args.iters,
              courant_equals_stored_reductions=bool(co == (asm.min_max(both)[1], ctx.sum(prod))), variants=res)
line = json.dumps(result)
print(line)
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "central_flux.json"), "w") as f:
    f.write(line + "\n")
with open(os.path.join(args.out_dir, "central_flux.md"), "w") as f:
    f.write("# rhoCentralFoam's flux evaluation on the device: tools/bench_central_flux.py\n\n")
    f.write("%d x %d x %d box, %s addressing: %d cells, %d internal faces, a patch of %d faces.  %d rounds of %d calls a window, the variants in turn in one\n"
            "process; median of the rounds, spread = (max - min)/median.  The yardsticks are entries the engine had before these passes.\n\n"
            % (args.dims[0], args.dims[1], args.dims[2], result["addressing"], N, F, NB, args.reps, args.iters))
    f.write("| variant | us | spread | bytes | of 8 TB/s | yardstick | time / yardstick | bytes / yardstick |\n|---|---|---|---|---|---|---|---|\n")
    for name, r in res.items():
        f.write("| %s | %.1f | %.3f | %d | %.3f | %s | %.3f | %.3f |\n" % (name, r["us"], r["spread"], r["bytes"], r["frac_8TBs"], r["yardstick"],
                                                                        r["ratio_to_yardstick"], r["byte_ratio"]))
    f.write("\nmi_central_courant returns what mi_min_max and mi_sum return over the stored products: %s.\n" % result["courant_equals_stored_reductions"])
