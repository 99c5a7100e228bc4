"""Explicit MULES (mi_mules_*) on the 216^3 box renumbered into the engine's tile order (ordered addressing: the row passes own the layout's
tiles), with the three boundary patches of tools/bench_reconstruct.py -- device events on the engine's stream; in each round every variant is
timed in turn, all in one process.  The yardsticks of the same run are mi_gauss_grad (the row pass with the same skeleton) and mi_limited_weights
with vanLeer (the gathering face pass).  The values are seeded: psi in [0, 1] with exact zeros and ones, the high-order flux the central flux
plus noise, so that the limiter's branches are all taken.
Algorithmic bytes (every array once; the row tables, owner / neighbour and the per-cell boundary lists not counted; b = per boundary face):
  begin, limit form    phi, phiPsi read, phiBD, phiCorr, lambda written 40F; psi, psi0, V read, four work arrays written 56N; 49b
  begin, limiter form  phiBD, phiCorr read 16F; 56N; 24b
  iterate(1)           sums: lambda, phiCorr 16F; four work arrays read, lambdap / lambdam written 48N; 16b
                       lambda: phiCorr, lambda read, lambda written 24F; lambdap / lambdam gathered 16N; 37b             -> 40F + 64N + 53b
  apply                phiBD, phiCorr, lambda read, the flux written 32F; 32b
  explicit_solve       the flux 8F; psi0, V read, psi written 24N; 8b
  limit, 3 iterations  begin + 3 iterate + apply                                                                       -> 192F + 248N + 240b
  mi_gauss_grad        32F + 32N;   mi_limited_weights (scalar)  24F + 56N
Prints the result as one JSON line: per variant the median us, the spread (max - min)/median over the rounds, its bytes, the fraction of 8 TB/s,
the ratio to its yardstick (median over rounds of the per-round ratio; a variant made of row and face passes is compared with the sum of the
yardsticks it is made of) beside the byte ratio.  `--reps 2 --iters 3` for a run under rocprofv3."""
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
phiPsi = phi * (0.5 * (psi[lo_d] + psi[up_d])) + R(F, -0.0375, 0.0375)
bphiPsi = bphi * bpsi + R(NB, -0.0375, 0.0375)
del lo_d, up_d, pick
mu = eng.Mules(addr, B)
fields = eng.mules_fields(vol, psi, psi.clone(), r_delta_t=1.0, b_psi=bpsi)
t = dict(phi=(phi, bphi), phi_psi=(phiPsi, bphiPsi), phi_bd=(E(F), E(NB)), phi_corr=(E(F), E(NB)), lambda_=(E(F), E(NB)), out=(E(F), E(NB)))
flux = eng.mules_flux(**{k: v[0] for k, v in t.items()}, **{"b_" + k: v[1] for k, v in t.items()})
psi_out = E(N)
# the yardsticks' own arrays
Sf = [R(F, -0.5, 0.5) for _ in range(3)]
gg = [E(N) for _ in range(3)]
grad, C, cdw, w = [R(N, -1.0, 1.0) for _ in range(3)], [R(N) for _ in range(3)], R(F, 0.3, 0.7), E(F)
vanLeer = eng.limiter("vanLeer")

row, face = "mi_gauss_grad (row pass)", "mi_limited_weights vanLeer (face pass)"
yard_bytes = {row: 32 * F + 32 * N, face: 24 * F + 56 * N}
# name -> (call, bytes, {yardstick: how many of it the variant is compared with})
variants = {
    row: (lambda: asm.gauss_grad(Sf, phi, vol, gg), yard_bytes[row], {row: 1}),
    face: (lambda: asm.limited_weights(vanLeer, cdw, phi, [psi], grad, C, w), yard_bytes[face], {face: 1}),
    "begin, limit form": (lambda: asm.mules_begin(mu, "limit", fields, flux), 40 * F + 56 * N + 49 * NB, {row: 1}),
    "begin, limiter form": (lambda: asm.mules_begin(mu, "limiter", fields, flux), 16 * F + 56 * N + 24 * NB, {row: 1}),
    "iterate(1): sums + lambda": (lambda: asm.mules_iterate(mu, 1, fields, flux), 40 * F + 64 * N + 53 * NB, {row: 1, face: 1}),
    "apply": (lambda: asm.mules_apply(mu, False, fields, flux), 32 * F + 32 * NB, {face: 1}),
    "explicit_solve": (lambda: asm.mules_explicit_solve(mu, fields, t["out"][0], psi_out, b_phi_psi=t["out"][1]), 8 * F + 24 * N + 8 * NB, {row: 1}),
    "limit, nLimiterIter 3": (lambda: asm.mules_limit(mu, fields, flux, 3, False), 192 * F + 248 * N + 240 * NB, {row: 4, face: 4}),
}


def limit_and_solve():
    asm.mules_limit(mu, fields, flux, 3, False)
    asm.mules_explicit_solve(mu, fields, t["out"][0], psi_out, b_phi_psi=t["out"][1])


variants["limit + explicit_solve"] = (limit_and_solve, 200 * F + 272 * N + 248 * NB, {row: 5, face: 4})
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
lam = t["lambda_"][0]
shares = dict(ones=round(float((lam == 1.0).double().mean()), 3), zeros=round(float((lam == 0.0).double().mean()), 3))
line = json.dumps(dict(tool="bench_mules", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB,
                       reps=args.reps, iters=args.iters, lambda_after_limit=shares, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
mu.close()
B.close()
