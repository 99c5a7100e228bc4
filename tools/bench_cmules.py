"""Semi-implicit MULES (mi_mules_begin_corr, mi_mules_limit_corr, mi_mules_correct) and the interfaceCompression face passes on the 216^3 box
renumbered into the engine's tile order (ordered addressing), with the three boundary patches of tools/bench_mules.py -- device events on the
engine's stream; in each round every variant is timed in turn, all in one process.  The yardsticks of the same run are mi_gauss_grad (the row
pass with the same skeleton) and mi_limited_weights with vanLeer (the gathering face pass).  The values are seeded as tools/bench_mules.py seeds
them; phiCorr is the high-order flux minus the upwind flux.
Algorithmic bytes (every array once; the row tables, owner / neighbour and the per-cell boundary lists not counted; b = per boundary face):
  begin_corr, limit form     phiCorr read, lambda written 16F; psi, V read, four work arrays written 48N; 24b
  begin_corr, limiter form   phiCorr read 8F; 48N; 16b
  iterate(1), corr rule      sums 16F + 48N + 16b; lambda 24F + 16N + 37b (b_phi in the place of b_phi_bd)               -> 40F + 64N + 53b
  apply in place             lambda, phiCorr read, phiCorr written 24F; 24b
  correct                    phiCorr 8F; psi, V read, psi written 24N; 8b
  limit_corr, 3 iterations   begin_corr + 3 iterate + the product                                                        -> 160F + 240N + 207b
  interfaceCompression       weights: cdw, flux read, weights written 24F, alpha gathered 8N; the fused flux the same 24F + 8N
  unfused compression flux   two weight passes 48F + 16N, two mi_face_interpolate 32F + 16N (the host's negations, products and the cell pass
                             for alpha2 are NOT in it: they are not device entries of the engine)
  mi_gauss_grad              32F + 32N;   mi_limited_weights (scalar)  24F + 56N
The in-place entries change their arrays from call to call (phiCorr shrinks, psi drifts); "limit_corr, staged out of place" is the same kernels
on constant inputs.  Prints one JSON line as tools/bench_mules.py does.  `--reps 2 --iters 3` for a run under rocprofv3."""
import argparse
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
gen = torch.Generator(device=dev).manual_seed(5)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
lo_d, up_d = torch.from_numpy(lo.astype(np.int64)).to(dev), torch.from_numpy(up.astype(np.int64)).to(dev)
psi = R(N)
pick = R(N)
psi[pick < 0.25] = 0.0
psi[pick > 0.75] = 1.0
vol = R(N, 0.5, 1.5)
phi, bphi, bpsi = R(F, -0.75, 0.75), R(NB, -0.75, 0.75), R(NB)
P, Q = psi[lo_d], psi[up_d]
phiCorr = phi * (0.5 * (P + Q)) + R(F, -0.0375, 0.0375) - phi * torch.where(phi >= 0, P, Q)
bphiCorr = R(NB, -0.0375, 0.0375)
del lo_d, up_d, pick, P, Q
mu = eng.Mules(addr, B)
fields = eng.mules_fields(vol, psi, None, r_delta_t=1.0, b_psi=bpsi)
lam, out = (E(F), E(NB)), (E(F), E(NB))
flux = eng.mules_flux(phi_corr=phiCorr, b_phi_corr=bphiCorr, b_phi=bphi, lambda_=lam[0], b_lambda_=lam[1], out=out[0], b_out=out[1])
work_corr = (phiCorr.clone(), bphiCorr.clone())                  # what the in-place entries shrink
flux_in_place = eng.mules_flux(phi_corr=work_corr[0], b_phi_corr=work_corr[1], b_phi=bphi, lambda_=lam[0], b_lambda_=lam[1], out=work_corr[0],
                               b_out=work_corr[1])
psi_c = psi.clone()                                              # what correct updates
# the yardsticks' own arrays, and the compression passes'
Sf = [R(F, -0.5, 0.5) for _ in range(3)]
gg = [E(N) for _ in range(3)]
grad, C, cdw, w, w2, i1, i2, fused = [R(N, -1.0, 1.0) for _ in range(3)], [R(N) for _ in range(3)], R(F, 0.3, 0.7), E(F), E(F), E(F), E(F), E(F)
alpha2 = 1.0 - psi
vanLeer = eng.limiter("vanLeer")

row, face = "mi_gauss_grad (row pass)", "mi_limited_weights vanLeer (face pass)"
yard_bytes = {row: 32 * F + 32 * N, face: 24 * F + 56 * N}


def staged():
    asm.mules_begin_corr(mu, "limit", fields, flux)
    asm.mules_iterate(mu, 3, fields, flux)
    asm.mules_apply(mu, True, fields, flux)


def limit_and_correct():
    asm.mules_limit_corr(mu, fields, flux_in_place, 3)
    asm.mules_correct(mu, fields, work_corr[0], psi_c, b_phi_corr=work_corr[1])


def two_weights():
    asm.interface_compression_weights(cdw, phi, alpha2, w2)
    asm.interface_compression_weights(cdw, phi, psi, w)


def unfused():
    asm.interface_compression_weights(cdw, phi, alpha2, w2)
    asm.face_interpolate(w2, alpha2, i2)
    asm.interface_compression_weights(cdw, phi, psi, w)
    asm.face_interpolate(w, psi, i1)


# name -> (call, bytes, {yardstick: how many of it the variant is compared with})
variants = {
    row: (lambda: asm.gauss_grad(Sf, phi, vol, gg), yard_bytes[row], {row: 1}),
    face: (lambda: asm.limited_weights(vanLeer, cdw, phi, [psi], grad, C, w), yard_bytes[face], {face: 1}),
    "begin_corr, limit form": (lambda: asm.mules_begin_corr(mu, "limit", fields, flux), 16 * F + 48 * N + 24 * NB, {row: 1}),
    "begin_corr, limiter form": (lambda: asm.mules_begin_corr(mu, "limiter", fields, flux), 8 * F + 48 * N + 16 * NB, {row: 1}),
    "iterate(1), corr rule: sums + lambda": (lambda: asm.mules_iterate(mu, 1, fields, flux), 40 * F + 64 * N + 53 * NB, {row: 1, face: 1}),
    "apply in place": (lambda: asm.mules_apply(mu, True, fields, flux_in_place), 24 * F + 24 * NB, {face: 1}),
    "correct": (lambda: asm.mules_correct(mu, fields, phiCorr, psi_c, b_phi_corr=bphiCorr), 8 * F + 24 * N + 8 * NB, {row: 1}),
    "limit_corr, staged out of place": (staged, 160 * F + 240 * N + 207 * NB, {row: 4, face: 4}),
    "limit_corr, nLimiterIter 3": (lambda: asm.mules_limit_corr(mu, fields, flux_in_place, 3), 160 * F + 240 * N + 207 * NB, {row: 4, face: 4}),
    "limit_corr + correct": (limit_and_correct, 168 * F + 264 * N + 215 * NB, {row: 5, face: 4}),
    "interface_compression_weights": (lambda: asm.interface_compression_weights(cdw, phi, psi, w), 24 * F + 8 * N, {face: 1}),
    "alpha_compression_flux (fused)": (lambda: asm.alpha_compression_flux(cdw, phi, psi, fused), 24 * F + 8 * N, {face: 1}),
    "two weight passes": (two_weights, 48 * F + 16 * N, {face: 2}),
    "unfused: 2 weights + 2 face_interpolate": (unfused, 80 * F + 32 * N, {face: 4}),
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
    base = [sum(k * times[y][r] for y, k in yard.items()) for r in range(args.reps)]
    res[name] = dict(us=round(us, 1), spread=round((max(times[name]) - min(times[name])) / us, 3), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3), yardstick=" + ".join(f"{k} x {y}" for y, k in yard.items()),
                     ratio_to_yardstick=round(statistics.median([x / x0 for x, x0 in zip(times[name], base)]), 3),
                     byte_ratio=round(nbytes / sum(k * yard_bytes[y] for y, k in yard.items()), 3))
fused_vs = {k: round(statistics.median([x / y for x, y in zip(times["alpha_compression_flux (fused)"], times[k])]), 3)
            for k in ("two weight passes", "unfused: 2 weights + 2 face_interpolate")}
staged()
lam0 = lam[0]
shares = dict(ones=round(float((lam0 == 1.0).double().mean()), 3), zeros=round(float((lam0 == 0.0).double().mean()), 3))
line = json.dumps(dict(tool="bench_cmules", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB,
                       reps=args.reps, iters=args.iters, lambda_after_limit_corr=shares, fused_flux_time_over=fused_vs, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
mu.close()
B.close()
