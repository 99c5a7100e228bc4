"""The leastSquares gradient (mi_ls_grad) on the 216^3 box with the six walls as patches -- device events on the engine's stream: in each
round the scalar and the vector gradient are timed in turn with mi_gauss_grad as the yardstick, all in one process; the vectors build
(mi_ls_vectors_create, once per mesh) is timed once, for the record, with the host clock around the call (it synchronises).
Algorithmic bytes (every array once; the row tables, the owner gathers and the per-cell boundary lists not counted):
  scalar: pVectors and nVectors 48F; vf 8N, the gradient written 24N                                 -> 48F + 32N
  vector: pVectors and nVectors 48F; vf 24N, the gradient written 72N                                -> 48F + 96N
  mi_gauss_grad: Sf and ssf 32F, V 8N, g written 24N                                                 -> 32F + 32N
Prints the result as one JSON line: per variant the median us, its bytes, the fraction of 8 TB/s, and the ratio to the yardstick
(median over rounds of the per-round ratio).  `--reps 2 --iters 3` for a run under rocprofv3."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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
nx, ny, nz = args.dims
case = syn.box_case(nx, ny, nz)
N, F = case.n_cells, case.n_faces
lo, up = case.lower_addr, case.upper_addr
addr = eng.Addressing(ctx, N, lo, up)
asm = eng.Assembly(addr)
# geometry of the uniform box (spacing 1/nx), its six walls x-, x+, y-, y+, z-, z+ in that order: delta = Cf - C, half a cell
h = 1.0 / nx
c = np.arange(N)
ijk = (c % nx, (c // nx) % ny, c // (nx * ny))
fcs, bd = [], [[], [], []]
for ax, m in enumerate((nx, ny, nz)):
    for side in (0, m - 1):
        fc = np.nonzero(ijk[ax] == side)[0].astype(np.int32)
        fcs.append(fc)
        for d in range(3):
            bd[d].append(np.full(fc.shape[0], (-0.5 if side == 0 else 0.5) * h if d == ax else 0.0))
B = eng.GradBoundary(addr, fcs, ["fixesValue"] * 6)
NB = B.n_faces
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
C = [T((x + 0.5) * h) for x in ijk]
bDelta = [T(np.concatenate(x)) for x in bd]
step = up - lo
Sf = [T(np.where(step == s, h * h, 0.0)) for s in (1, nx, nx * ny)]
del bd, c, ijk
gen = torch.Generator(device=dev).manual_seed(5)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
weights, magSf, bMagSf = R(F, 0.3, 0.7), torch.full((F,), h * h, dtype=torch.float64, device=dev), torch.full((NB,), h * h, dtype=torch.float64, device=dev)
ssf, vol = R(F, -0.5, 0.5), torch.full((N,), h ** 3, dtype=torch.float64, device=dev)
gg = [torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3)]
asm.gauss_grad(Sf, ssf, vol, gg)                                # the addressing makes its row tables at its first row pass, not in the timed build
torch.cuda.synchronize()
tb = time.perf_counter()
lsv = eng.LsVectors(addr, B, C, weights, magSf, None, bMagSf, bDelta)
build_ms = (time.perf_counter() - tb) * 1e3
vf = [R(N, -0.5, 0.5) for _ in range(3)]
bv = [R(NB, -0.5, 0.5) for _ in range(3)]
grad = [torch.empty(N, dtype=torch.float64, device=dev) for _ in range(9)]

base = "Gauss linear (mi_gauss_grad)"
variants = {base: (lambda: asm.gauss_grad(Sf, ssf, vol, gg), 32 * F + 32 * N)}
for nc in (1, 3):
    variants["leastSquares " + ("vector" if nc == 3 else "scalar")] = (
        (lambda nc=nc: asm.ls_grad(lsv, vf[:nc], grad[:3 * nc], bvalue=bv[:nc])), 48 * F + (96 if nc == 3 else 32) * N)
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
res = {}
for name, (_, nbytes) in variants.items():
    us = statistics.median(times[name])
    res[name] = dict(us=round(us, 1), bytes=nbytes, frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3),
                     ratio_to_yardstick=round(statistics.median([t / t0 for t, t0 in zip(times[name], times[base])]), 3))
line = json.dumps(dict(tool="bench_ls_grad", dims=args.dims, cells=N, faces=F, boundary_faces=NB, reps=args.reps, iters=args.iters,
                       vectors_build_ms=round(build_ms, 2), variants=res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
lsv.close()
B.close()
