"""fvc::reconstruct (mi_fvc_reconstruct) for n_rhs 1, 3 and 4 on the 216^3 box renumbered into the engine's tile order (ordered addressing: the
row passes own the layout's tiles) -- device events on the engine's stream; in each round every variant is timed in turn with mi_gauss_grad, the
pass with the same skeleton, as the yardstick, all in one process.  mi_reconstruct_create (once per mesh) is timed once, for the record, with
the host clock around the call (it synchronises).  Every cell short of six internal faces gets its missing faces as boundary faces, in three
patches (6*216^2 boundary faces, as the six walls have); the geometry is seeded: the passes' time does not depend on the values.
Algorithmic bytes (every array once; the row tables and the per-cell boundary lists not counted):
  mi_fvc_reconstruct: SfHat 24F and the fluxes 8F*n_rhs; the inverse 72N, the vectors written 24N*n_rhs   -> (24 + 8 n_rhs)F + (72 + 24 n_rhs)N
                      plus (24 + 8 n_rhs) bytes per boundary face
  mi_gauss_grad:      Sf and ssf 32F, V 8N, g written 24N                                                     -> 32F + 32N
Prints the result as one JSON line: per variant the median us, the spread (max - min)/median over the rounds, its bytes, the fraction of 8 TB/s,
the ratio to the yardstick (median over rounds of the per-round ratio) beside the byte ratio.  `--reps 2 --iters 3` for a run under rocprofv3."""
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
Sf, magSf = [R(F, -0.5, 0.5) for _ in range(3)], R(F, 0.5, 1.5)
bSf, bMagSf = [R(NB, -0.5, 0.5) for _ in range(3)], R(NB, 0.5, 1.5)
ssf, bssf = [R(F, -0.5, 0.5) for _ in range(4)], [R(NB, -0.5, 0.5) for _ in range(4)]
vol = R(N, 0.5, 1.5)
gg = [E(N) for _ in range(3)]
out = [E(N) for _ in range(12)]
asm.gauss_grad(Sf, ssf[0], vol, gg)                             # the addressing makes its row tables at its first row pass, not in the timed build
torch.cuda.synchronize()
tb = time.perf_counter()
rc = eng.Reconstruct(addr, B, Sf, magSf, bSf, bMagSf)
create_ms = (time.perf_counter() - tb) * 1e3

base = "Gauss linear (mi_gauss_grad)"
variants = {base: (lambda: asm.gauss_grad(Sf, ssf[0], vol, gg), 32 * F + 32 * N)}
for n in (1, 3, 4):
    variants[f"reconstruct n_rhs={n}"] = ((lambda n=n: asm.reconstruct(rc, ssf[:n], out[:3 * n], b_ssf=bssf[:n])),
                                          (24 + 8 * n) * F + (72 + 24 * n) * N + (24 + 8 * n) * NB)
times = {k: [] for k in variants}
for fn, _ in variants.values():
    for _ in range(3):
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
    res[name] = dict(us=round(us, 1), spread=round((max(times[name]) - min(times[name])) / us, 3), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3),
                     ratio_to_yardstick=round(statistics.median([t / t0 for t, t0 in zip(times[name], times[base])]), 3),
                     byte_ratio=round(nbytes / variants[base][1], 3))
line = json.dumps(dict(tool="bench_reconstruct", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB,
                       reps=args.reps, iters=args.iters, reconstruct_create_ms=round(create_ms, 2), handle_bytes=24 * F + 72 * N + 24 * NB, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
rc.close()
B.close()
