"""The limited schemes' weights (mi_limited_weights) on the 216^3 box, device events on the engine's stream: in each round every kind,
scalar and V, is timed in turn, with mi_limited_linear_weights as the yardstick, all in one process.
Algorithmic bytes (every array once, addressing not counted -- the convention of tools/bench_kernels.py's limitedLinear row):
  scalar: cdw, flux in + w out = 24F; phi, 3 gradient components, 3 centre components = 56N          -> 24F + 56N
  V:      24F; 3 phi components, 9 gradient components, 3 centre components = 120N                     -> 24F + 120N
Prints the result as one JSON line: per variant the median us, its bytes, the fraction of 8 TB/s, and the ratio to the yardstick
(median over rounds of the per-round ratio).  `--reps 2 --iters 3` for a run under rocprofv3."""
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
flux, cdw = R(F, -0.5, 0.5), R(F, 0.3, 0.7)
phi = [R(N, -0.5, 0.5) for _ in range(3)]
grad = [R(N, -1.0, 1.0) for _ in range(9)]
C = [R(N) for _ in range(3)]
w = torch.empty(F, dtype=torch.float64, device=dev)

variants = {"limitedLinear (mi_limited_linear_weights)": (lambda: asm.limited_linear_weights(1.0, cdw, flux, phi[0], grad[:3], C, w), 24 * F + 56 * N)}
for kind in eng.LIMITER_KINDS:
    ks = " 1" if kind in ("limitedLinear", "limitedCubic", "Gamma") else ""
    for vec in (False, True):
        lim = eng.limiter(kind + ("V" if vec else "") + ks)
        nc = 3 if vec else 1
        variants[kind + ("V" if vec else "")] = ((lambda lim=lim, nc=nc: asm.limited_weights(lim, cdw, flux, phi[:nc], grad[:3 * nc], C, w)),
                                                  24 * F + (120 if vec else 56) * N)
times = {k: [] for k in variants}
for fn, _ in variants.values():
    fn()
torch.cuda.synchronize()
for _ in range(args.reps):
    for name, (fn, _) in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.iters):
            fn()
        b.record(stream)
        b.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
base = "limitedLinear (mi_limited_linear_weights)"
res = {}
for name, (_, nbytes) in variants.items():
    us = statistics.median(times[name])
    res[name] = dict(us=round(us, 1), bytes=nbytes, frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3),
                     ratio_to_yardstick=round(statistics.median([t / t0 for t, t0 in zip(times[name], times[base])]), 3))
line = json.dumps(dict(tool="bench_limited_schemes", dims=args.dims, cells=N, faces=F, reps=args.reps, iters=args.iters, variants=res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
