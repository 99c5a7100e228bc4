"""The thermo update on the device (mi_thermo_calculate, mi_thermo_calculate_boundary) on the 216^3 box -- device events on the engine's
stream; in each round every variant is timed in turn, all in one process, so the compared runs alternate.
  cell pass   h + hConst + const, h + hConst + sutherland and h + janaf + sutherland, from a start temperature about 1 % off (the in-loop
              case) and from one 30 % off, without rho (56 bytes per cell) and, for the 1 % start, with rho = psi*p (64 bytes per cell)
  comparator  mi_ke_epsilon_terms (nu a field), an existing pure streaming pass of 64 bytes per cell, and a copy of a cell array (16 bytes)
  boundary    mi_thermo_calculate_boundary on the box's six patches in one launch against six launches of the cell entry on the patch slices
Algorithmic bytes: every array once (he, p, T0 in; T, psi, mu, alpha [, rho] out).  Prints one JSON line, writes it to profiles/thermo.json and
puts the table of times between the marker lines of profiles/thermo.md (the rest of that file, the kernels' resource usage, is kept).
`--reps 2 --iters 3` for a run under a profiler."""
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
ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermo.json"))
ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "thermo.md"))
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
addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
asm = eng.Assembly(addr)
N = case.n_cells
c = np.arange(N, dtype=np.int32)
i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
fcs = [c[i == 0], c[i == nx - 1], c[j == 0], c[j == ny - 1], c[k == 0], c[k == nz - 1]]
kinds = [2, 1, 2, 2, 1, 2]                                 # a fixedValue inlet and outlet among patches that do not fix T
B = eng.GradBoundary(addr, fcs, ["other"] * 6)
NB = B.n_faces
cut = np.cumsum([0] + [fc.shape[0] for fc in fcs])
gen = torch.Generator(device=dev).manual_seed(13)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
MODELS = {"h hConst const": dict(energy="h", thermo="hConst", transport="const"),
          "h hConst sutherland": dict(energy="h", thermo="hConst", transport="sutherland"),
          "h janaf sutherland": dict(energy="h", thermo="janaf", transport="sutherland")}
T, p = R(N, 300.0, 2000.0), R(N, 0.8e5, 1.2e5)
sign = torch.where(R(N) < 0.5, -1.0, 1.0)
starts = {"1 %": T * (1.0 + 0.01 * sign), "30 %": T * (1.0 + 0.3 * sign)}
out = [E(N) for _ in range(5)]
iters = torch.zeros(N, dtype=torch.int32, device=dev)
Kc = eng.ke_coeffs()
G, eps, kk, nut, nu_f = R(N), R(N, 0.1, 10.0), R(N, 0.01, 1.0), R(N, 1e-4, 1e-2), R(N, 0.5e-5, 1.5e-5)
bT, bp = R(NB, 300.0, 2000.0), R(NB, 0.8e5, 1.2e5)
bsign = torch.where(R(NB) < 0.5, -1.0, 1.0)
bT0 = bT * (1.0 + 0.01 * bsign)
bout = [E(NB) for _ in range(5)]

variants, evals = {}, {}
for name, given in MODELS.items():
    K = eng.thermo_model(**given)
    he, bhe = E(N), E(NB)
    asm.thermo_he(K, p, T, he)
    asm.thermo_he(K, bp, bT, bhe)
    for start, t0 in starts.items():
        asm.thermo_calculate(K, he, p, t0, *out[:4], iters_out=iters)
        torch.cuda.synchronize()
        evals[f"{name}, start {start} off"] = round(float(iters.double().mean().item()), 3)
        variants[f"{name}, start {start} off"] = (lambda K=K, he=he, t0=t0: asm.thermo_calculate(K, he, p, t0, *out[:4]), 56 * N)
    variants[f"{name}, start 1 % off, rho = psi*p"] = (lambda K=K, he=he: asm.thermo_calculate(K, he, p, starts["1 %"], *out, rho_form=2), 64 * N)
    if name == "h janaf sutherland":
        bheK, KB = bhe, K

        def one_launch():
            asm.thermo_calculate_boundary(B, KB, kinds, bheK, bp, bT0, *bout[1:4], b_t_out=bout[0])

        def six_launches():
            for a, b in zip(cut[:-1], cut[1:]):
                asm.thermo_calculate(KB, bheK[a:b], bp[a:b], bT0[a:b], *[x[a:b] for x in bout[:4]])

        variants["boundary, six patches in one launch (h janaf sutherland)"] = (one_launch, 56 * NB)
        variants["boundary, six launches of the cell entry on patch slices"] = (six_launches, 56 * NB)
variants["ke_epsilon_terms (comparator, 64 bytes per cell)"] = (lambda: asm.ke_epsilon_terms(Kc, G, eps, kk, nut, nu_f, *out[:3]), 64 * N)
variants["copy of a cell array (16 bytes per cell)"] = (lambda: out[0].copy_(T), 16 * N)

times = {name: [] for name in variants}
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
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3))
    if name in evals:
        res[name]["mean_evaluations"] = evals[name]
line = json.dumps(dict(tool="bench_thermo", dims=args.dims, cells=N, boundary_faces=NB, reps=args.reps, iters=args.iters, variants=res))
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
BEGIN, END = "<!-- times: written by tools/bench_thermo.py -->", "<!-- end of times -->"
rows = ["| variant | us (median of %d) | spread | bytes | share of 8 TB/s | mean Newton evaluations |" % args.reps, "|---|---:|---:|---:|---:|---:|"]
rows += ["| %s | %.1f | %.3f | %d | %.3f | %s |" % (n, r["us"], r["spread"], r["bytes"], r["frac_8TBs"], r.get("mean_evaluations", "")) for n, r in res.items()]
table = "\n".join([BEGIN, "", "%d x %d x %d box, %d cells, %d boundary faces, %d calls per window." % (nx, ny, nz, N, NB, args.iters), ""] + rows + ["", END])
text = open(args.md).read() if os.path.exists(args.md) else "# The thermo update: measurements\n\n" + BEGIN + "\n" + END + "\n"
if BEGIN in text and END in text:
    text = text[:text.index(BEGIN)] + table + text[text.index(END) + len(END):]
else:
    text = text.rstrip("\n") + "\n\n" + table + "\n"
with open(args.md, "w") as f:
    f.write(text)
B.close()
