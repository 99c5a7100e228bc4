"""The `limited` snGrad scheme's correction flux (mi_sngrad_limited_correction_flux) on the 216^3 box with non-zero correction vectors --
device events on the engine's stream.  In each round mi_sngrad_correction_flux (the `corrected` scheme's face pass) is timed as the
yardstick, then the scalar and the vector limited form in turn, then the unfused composition the scalar form replaces: the yardstick
call without gammaMagSf plus the element-wise passes for snGrad, the two mag, the products, the sum, the quotient, min and the two
products (torch ops).  All in one process.
Algorithmic bytes (every array once, addressing counted as 8F):
  yardstick:      lo, up 8F; cv 24F, lambda 8F, gammaMagSf 8F, flux 8F; g 24N                       -> 56F + 24N
  limited scalar: + deltaCoeffs 8F; vf 8N                                                           -> 64F + 32N
  limited vector: lo, up 8F; cv 24F, lambda, deltaCoeffs, gammaMagSf 24F, flux 24F; vf 24N, g 72N   -> 80F + 96N
The model does not count the 8 (scalar) or 24 (vector) gathers per face.
Prints one JSON line: per variant the time of every window, the median, the spread between windows ((max - min)/median), the bytes, the
fraction of 8 TB/s, the ratio to the yardstick (median, min and max over the rounds of the per-round ratio) beside the byte ratio, and
`miss`: the measured ratio exceeds the byte ratio by more than the yardstick's own spread.  `--reps 2 --iters 3` for a run under rocprofv3."""
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
ap.add_argument("--reps", type=int, default=7, help="rounds (windows per variant); each round times every variant once, in turn")
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--k", type=float, default=0.5, help="limitCoeff")
ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
args = ap.parse_args()

graft.build()
pkg = graft.load_package()
syn, eng = pkg.synthetic, pkg.engine
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = eng.Context(0, stream.cuda_stream)
nx, ny, nz = args.dims
case = syn.box_case(nx, ny, nz)
N, F = case.n_cells, case.n_faces
lo, up = case.lower_addr, case.upper_addr
addr = eng.Addressing(ctx, N, lo, up)
asm = eng.Assembly(addr)
h = 1.0 / nx
gen = torch.Generator(device=dev).manual_seed(7)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
cv = [R(F, -0.3, 0.3) for _ in range(3)]                      # non-zero correction vectors: a mesh that is not orthogonal
lam, dc, gms = R(F, 0.4, 0.6), R(F, 0.9 / h, 1.1 / h), R(F, 0.8 * h * h, 1.2 * h * h)
vf = [R(N, -0.5, 0.5) for _ in range(3)]
g = [R(N, -0.5 / h, 0.5 / h) for _ in range(9)]               # |corr| and |snGrad| of the same size: both branches of the min are taken
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
y, out, lim = E(F), [E(F) for _ in range(3)], E(F)
lo64, up64 = torch.from_numpy(lo.astype(np.int64)).to(dev), torch.from_numpy(up.astype(np.int64)).to(dev)
k = args.k


def unfused_scalar():
    """the parent's composition for limitedSnGrad<scalar>::correction: the `corrected` face pass, then one pass per field operator"""
    asm.sngrad_correction_flux(cv, lam, g[:3], None, y)
    sn = dc * (vf[0][up64] - vf[0][lo64])
    num = k * sn.abs()
    den = (1 - k) * y.abs() + 1e-15
    limiter = torch.clamp(num / den, max=1.0)
    return gms * (limiter * y)


base = "corrected (mi_sngrad_correction_flux)"
variants = {
    base: (lambda: asm.sngrad_correction_flux(cv, lam, g[:3], gms, y), 56 * F + 24 * N),
    "limited scalar": (lambda: asm.sngrad_limited_correction_flux(k, cv, lam, dc, vf[:1], g[:3], gms, out[:1]), 64 * F + 32 * N),
    "limited vector": (lambda: asm.sngrad_limited_correction_flux(k, cv, lam, dc, vf, g, gms, out), 80 * F + 96 * N),
    "limited scalar, unfused (yardstick + torch passes)": (unfused_scalar, None),
}
asm.sngrad_limited_correction_flux(k, cv, lam, dc, vf[:1], g[:3], gms, out[:1], lim)
share = float((lim < 1.0).double().mean().item())
ref = unfused_scalar()
agree = bool(torch.equal(ref, out[0]))                        # torch's passes round as the reference's field operators do
times = {name: [] for name in variants}
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
spread = lambda ts: (max(ts) - min(ts)) / statistics.median(ts)
base_spread = spread(times[base])
res = {}
for name, (_, nbytes) in variants.items():
    us = statistics.median(times[name])
    ratios = [t / t0 for t, t0 in zip(times[name], times[base])]
    r = dict(us=round(us, 1), windows_us=[round(t, 1) for t in times[name]], spread=round(spread(times[name]), 3),
             ratio_to_yardstick=round(statistics.median(ratios), 3), ratio_min=round(min(ratios), 3), ratio_max=round(max(ratios), 3))
    if nbytes is not None:
        byte_ratio = nbytes / variants[base][1]
        r.update(bytes=nbytes, frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3), byte_ratio=round(byte_ratio, 3),
                 miss=bool(statistics.median(ratios) > byte_ratio + base_spread))
    res[name] = r
line = json.dumps(dict(tool="bench_limited_sngrad", dims=args.dims, cells=N, faces=F, k=k, reps=args.reps, iters=args.iters,
                       share_limiter_below_1=round(share, 3), unfused_agrees_bit_for_bit=agree, yardstick_spread=round(base_spread, 3), variants=res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
