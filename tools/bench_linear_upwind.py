"""linearUpwind momentum assembly on the 216^3 box, three components, device events on the engine's stream, the variants alternated in
one process:
  (a) today's upwind assembly: mi_fvm_assemble of ddt + div(phi, U) [upwind] - laplacian(nu, U), three sources;
  (b) linearUpwind, unfused: (a) + the correction face pass (mi_linear_upwind_correction, three components) + per component
      mi_surface_integrate(t, V) + mi_vec_submul(V, ivf, source);
  (c) linearUpwind, fused: mi_fvm_assemble_corrected.
Algorithmic bytes (every array once; addressing not counted; grad(U) itself not included -- both linearUpwind variants need it):
  (a) flux, deltaCoeffs, gammaMagSf in + lower, upper out = 40F; V + 3 psi_old in, diag + 3 sources out = 64N
  (b) (a) + face pass flux + Cf in, 3 t out = 56F, C + 9 gradient components gathered = 96N; 3 x surfaceIntegrate t + V in, ivf out = 24F + 48N;
      3 x submul V, ivf, source in, source out = 96N                    -> increment 80F + 240N
  (c) (a) + Cf = 24F, C + 9 gradient components = 96N                  -> increment 24F + 96N
Prints the result as one JSON line (and writes it to --out when given); `--reps 2 --iters 3` for a run under rocprofv3."""
import argparse
import json
import os
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
addr = eng.Addressing(ctx, N, case.lower_addr, case.upper_addr)
A = eng.Assembly(addr)
gen = torch.Generator(device=dev).manual_seed(1)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
flux, vol, delta, gamma = R(F, -0.5, 0.5), R(N, 0.5, 1.5), R(F, 1.0, 2.0), R(F, 0.5, 1.5)
psi0 = [R(N, -0.5, 0.5) for _ in range(3)]
cf, C = [R(F) for _ in range(3)], [R(N) for _ in range(3)]
grads = [[R(N, -2.0, 2.0) for _ in range(3)] for _ in range(3)]
lower, upper, diag, src = E(F), E(F), E(N), [E(N) for _ in range(3)]
t, ivf = [E(F) for _ in range(3)], E(N)
ddt = dict(vol=vol, r_delta_t=1.0 / 3e-4, psi_old=psi0)
lap = dict(delta_coeffs=delta, gamma_magsf=gamma)
corr = dict(cf=cf, c=C, grad=grads)


def upwind():
    A.assemble(upper, diag, lower_out=lower, sources_out=src, ddt=ddt, div=dict(flux=flux), laplacian=lap)


def unfused():
    upwind()
    A.linear_upwind_correction(flux, cf, C, grads, t)
    for r in range(3):
        A.surface_integrate(t[r], vol, ivf)
        A.submul(vol, ivf, src[r])


def fused():
    A.assemble(upper, diag, lower_out=lower, sources_out=src, ddt=ddt, div=dict(flux=flux, correction=corr), laplacian=lap)


variants = {"a_upwind_assembly": (upwind, 40 * F + 64 * N),
            "b_linear_upwind_unfused": (unfused, 40 * F + 64 * N + 80 * F + 240 * N),
            "c_linear_upwind_fused": (fused, 40 * F + 64 * N + 24 * F + 96 * N)}

# the two linearUpwind variants compute the same bits
unfused(); ref = [s.clone() for s in src]
fused()
same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(src, ref))
assert same, "fused and unfused linearUpwind sources differ"

times = {k: [] for k in variants}
for fn, _ in variants.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rep in range(args.reps):
    for name, (fn, _) in variants.items():
        e0.record(stream)
        for _ in range(args.iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.iters)

rows = {}
for name, (_, alg) in variants.items():
    ms = sorted(times[name])
    best, med = ms[0], ms[len(ms) // 2]
    rows[name] = dict(ms_best=round(best, 4), ms_median=round(med, 4), ms_all=[round(x, 4) for x in times[name]], algorithmic_GB=round(alg / 1e9, 3),
                      frac_of_8TBps_best=round(alg / (best * 1e-3) / 8e12, 3))
    print(name, rows[name], flush=True)
a, b, c = (rows[k]["ms_median"] for k in variants)
res = dict(dims=args.dims, n_cells=N, n_faces=F, components=3, reps=args.reps, iters=args.iters, fused_equals_unfused_bitwise=same, variants=rows,
           correction_increment_ms=dict(unfused=round(b - a, 4), fused=round(c - a, 4)),
           correction_increment_GB=dict(unfused=round((80 * F + 240 * N) / 1e9, 3), fused=round((24 * F + 96 * N) / 1e9, 3)),
           fused_over_unfused_increment=round((c - a) / (b - a), 3) if b > a else None, target_ratio=0.6)
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
