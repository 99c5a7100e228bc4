"""The filtered schemes' weights (mi_filtered_weights) and the cubic correction (mi_cubic_correction) on the 216^3 box, device events on
the engine's stream; in each round every variant is timed in turn, all in one process.
  filtered kinds: the yardsticks are mi_limited_weights with limitedCubic (scalar) and limitedCubicV, which gather the same cell arrays.
    Algorithmic bytes as tools/bench_limited_schemes.py: scalar 24F + 56N, V 24F + 120N (addressing not counted).
  cubic correction: the yardstick is mi_linear_upwind_correction at the same n_rhs.  Byte model of cubic: 8F indices + 56F streamed
    (lambda, Sf x3, magSf, deltaCoeffs, flux) + 8F*n_rhs written + 32N*n_rhs gathered once (the field and three gradient components);
    of linearUpwind: 8F + 32F (flux, Cf x3) + 8F*n_rhs + 24N (C) + 24N*n_rhs.
Prints one JSON line: per variant the median us, the spread (max - min)/median over the rounds, its bytes, the fraction of 8 TB/s and the
ratio to its yardstick (median over rounds of the per-round ratio).  `--reps 2 --iters 3` for a run under rocprofv3."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, nargs=3, default=[216, 216, 216])
ap.add_argument("--reps", type=int, default=7, help="rounds; each round times every variant once, in turn")
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
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
N, F = case.n_cells, case.n_faces
asm = eng.Assembly(eng.Addressing(ctx, N, case.lower_addr, case.upper_addr))
gen = torch.Generator(device=dev).manual_seed(5)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
flux, cdw = R(F, -0.5, 0.5), R(F, 0.3, 0.7)
phi = [R(N, -0.5, 0.5) for _ in range(4)]
grads = [[R(N, -1.0, 1.0) for _ in range(3)] for _ in range(4)]
flat = [g for gr in grads for g in gr]
C, cf = [R(N) for _ in range(3)], [R(F) for _ in range(3)]
geo = eng.cubic_geometry(cdw, [R(F, -0.5, 0.5) for _ in range(3)], R(F, 0.5, 1.5), R(F, 1.0, 2.0))
w = E(F)
t = [E(F) for _ in range(4)]

variants = {}   # name -> (call, bytes, yardstick name)
for vec in (False, True):
    nc, nbytes = (3, 24 * F + 120 * N) if vec else (1, 24 * F + 56 * N)
    yard = "limitedCubicV 1" if vec else "limitedCubic 1"
    lim = eng.limiter(yard)
    variants[yard] = ((lambda lim=lim, nc=nc: asm.limited_weights(lim, cdw, flux, phi[:nc], flat[:3 * nc], C, w)), nbytes, yard)
    for s in (("filteredLinear2V 1 0", "filteredLinear3V 1") if vec else ("filteredLinear", "filteredLinear2 1 0", "filteredLinear3 1")):
        lim = eng.filtered(s)
        variants[s] = ((lambda lim=lim, nc=nc: asm.filtered_weights(lim, cdw, flux, phi[:nc], flat[:3 * nc], C, w)), nbytes, yard)
for n_rhs in (1, 3, 4):
    yard = f"linearUpwind n_rhs={n_rhs}"
    variants[yard] = ((lambda n=n_rhs: asm.linear_upwind_correction(flux, cf, C, grads[:n], t[:n])), 8 * F + 32 * F + 8 * F * n_rhs + 24 * N + 24 * N * n_rhs, yard)
    variants[f"cubic n_rhs={n_rhs}"] = ((lambda n=n_rhs: asm.cubic_correction(geo, phi[:n], grads[:n], t[:n], face_flux=flux)),
                                        8 * F + 56 * F + 8 * F * n_rhs + 32 * N * n_rhs, yard)

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
                     ratio_to_yardstick=round(statistics.median([x / y for x, y in zip(times[name], times[yard])]), 3))
line = json.dumps(dict(tool="bench_filtered_cubic", dims=args.dims, cells=N, faces=F, reps=args.reps, iters=args.iters, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
