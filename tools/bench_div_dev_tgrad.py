"""fvc::div(visc*dev(T(grad(U)))) / fvc::div(visc*dev2(T(grad(U)))) on the internal faces of the 216^3 box: the one call
(mi_fvc_div_dev_tgrad: one face pass + one three-component row pass) against the composition it replaces -- torch element-wise glue that
forms the nine X arrays (tr, ii, three diagonal differences), then three mi_flux_div(cell_scale = visc) calls.  Device events on the
engine's stream; in each round every variant is timed once, in turn, in one process.  Before anything is timed the two results (three
face arrays and three cell arrays per kind) are compared and must be bitwise equal.
Algorithmic bytes before the row sums, in doubles (F ~ 3N; addressing counted as one double per face):
  fused:       lo/up, lambda, Sf x3, three fluxes out: 7F + 1F;  visc + nine gradients: 10N                        -> ~ 31N (issue: 7F + 10N)
  composition: three times (lo/up, lambda, Sf x3, flux): 15F + 3F;  glue 19N (3 read + 1 written for tr, 1 + 1 for ii, 3 x (2 + 1) for the
               diagonal, off-diagonals untouched: ~ 15-19N by how the glue is fused) + 12N gathers (visc + 3 per call)    -> ~ 76N
The row sums read the row tables once (fused) instead of three times.
Prints one JSON line: per kind and variant the time of every window, the median, the spread between windows ((max - min)/median), and
the ratio composition / fused (median, min and max over the rounds of the per-round ratio) beside the byte ratio 76/31."""
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
ap.add_argument("--reps", type=int, default=7, help="rounds (windows per variant); each round times every variant once, in turn")
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
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
addr = eng.Addressing(ctx, N, case.lower_addr, case.upper_addr)
asm = eng.Assembly(addr)
h = 1.0 / nx
gen = torch.Generator(device=dev).manual_seed(7)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
lam = R(F, 0.4, 0.6)
sf = [R(F, -h * h, h * h) for _ in range(3)]
visc = R(N, 0.5, 1.5)
g = [R(N, -64.0, 64.0) for _ in range(9)]
vol = R(N, 0.9 * h ** 3, 1.1 * h ** 3)
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
face_a, div_a = [E(F) for _ in range(3)], [E(N) for _ in range(3)]
face_b, div_b = [E(F) for _ in range(3)], [E(N) for _ in range(3)]
COEFF = {"dev": 1.0 / 3.0, "dev2": 2.0 / 3.0}


def fused(kind):
    asm.div_dev_tgrad(kind, lam, sf, visc, g, face_a, div_a, vol)


def composition(kind):
    """today's form: the glue rounds as the reference's cell fields do, one torch pass per operator"""
    tr = (g[0] + g[4]) + g[8]
    ii = COEFF[kind] * tr
    x = [g[i] - ii if i % 4 == 0 else g[i] for i in range(9)]
    for j in range(3):
        asm.flux_div(lam, sf, [x[j], x[3 + j], x[6 + j]], face_b[j], div_b[j], cell_scale=visc, vol=vol)


for kind in eng.DEV_KINDS:                                    # bitwise agreement before any timing
    fused(kind); composition(kind)
    torch.cuda.synchronize()
    for j in range(3):
        assert torch.equal(face_a[j], face_b[j]) and torch.equal(div_a[j], div_b[j]), (kind, j)
variants = {(kind, name): (lambda fn=fn, kind=kind: fn(kind)) for kind in eng.DEV_KINDS for name, fn in (("fused", fused), ("composition", composition))}
times = {key: [] for key in variants}
for fn in variants.values():
    fn()
torch.cuda.synchronize()
for _ in range(args.reps):
    for key, fn in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.iters):
            fn()
        b.record(stream)
        b.synchronize()
        times[key].append(a.elapsed_time(b) * 1e3 / args.iters)
spread = lambda ts: (max(ts) - min(ts)) / statistics.median(ts)
res = {}
for kind in eng.DEV_KINDS:
    tf, tc = times[(kind, "fused")], times[(kind, "composition")]
    ratios = [c / f for c, f in zip(tc, tf)]
    res[kind] = dict(fused_us=round(statistics.median(tf), 1), fused_windows_us=[round(t, 1) for t in tf], fused_spread=round(spread(tf), 3),
                     composition_us=round(statistics.median(tc), 1), composition_windows_us=[round(t, 1) for t in tc],
                     composition_spread=round(spread(tc), 3), composition_over_fused=round(statistics.median(ratios), 3),
                     ratio_min=round(min(ratios), 3), ratio_max=round(max(ratios), 3))
line = json.dumps(dict(tool="bench_div_dev_tgrad", dims=args.dims, cells=N, faces=F, reps=args.reps, iters=args.iters, bitwise_equal=True,
                       byte_ratio_before_row_sums=round(76 / 31, 3), kinds=res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
