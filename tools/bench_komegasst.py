"""The kOmegaSST passes on the device (mi_sst_production, mi_sst_wall_cells, mi_sst_blend, mi_sst_omega_sources, mi_sst_k_terms, mi_sst_nut) on the
216^3 box of tools/bench_turbulence.py -- renumbered into the engine's tile order, the same three wall patches, device events on the
engine's stream, every variant timed in turn in each round, all in one process.  mi_sst_blend and mi_sst_nut are set beside the same result
composed from the mi_vec_* entries the engine had before them.  Such a composition cannot form a square root, a tanh or a two-field max: those
passes are LEFT OUT of its figure (mi_vec_min stands in for each max / min of two fields, mi_vec_max_value for a max with a constant), which
flatters the yardstick.  A product is mi_vec_submul on a zeroed array (the zero fill is timed and counted), a scaling mi_vec_axpby in place:
  blend  CDkOmega: zero fill, 3 submul, axpby, div; max with 1e-10; sqr(y), omega*y and sqr(y)*omega: 3 x (zero fill, submul); the three arms
         of arg1: axpby + div, axpby + div, axpby + zero fill + submul + div; 2 min; arg2: axpby, div, min; the limiter: axpby, zero fill,
         submul, min; its product and min(S2, .): axpby, zero fill, submul, min; su, sp: 2 x (axpby, zero fill, submul); susp: axpby, zero fill,
         submul, div; DomegaEff and DkEff: 2 x (axpby, zero fill, submul, axpby)                      -- 52 passes, no sqrt, no tanh, F3 off
  nut    arg2: zero fill, submul, axpby, div, zero fill, submul (twice: y*y, then *omega), axpby, div, min; the limiter: axpby, zero fill, submul, min;
         axpby, div   -- 17 passes, no sqrt, no tanh
Algorithmic bytes (every array once): production 96N (104N with mag); blend 136N (nu a number, no optional output); omega sources 72N;
k terms 40N; nut 40N; wall cells 80w + 64b.  Prints one JSON line as tools/bench_turbulence.py does."""
import argparse
import ctypes as C
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
a0 = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr)
case = syn.renumber(case, a0.cell_perm())
addr = eng.Addressing(ctx, case.n_cells, case.lower_addr, case.upper_addr, ordered=True, tile_cell_start=a0.tile_starts())
N, F = case.n_cells, case.n_faces
lo, up = case.lower_addr, case.upper_addr
asm = eng.Assembly(addr)
missing = 6 - (np.bincount(lo, minlength=N) + np.bincount(up, minlength=N))
fcs = [np.nonzero(missing > k)[0].astype(np.int32) for k in range(3)]
B = eng.GradBoundary(addr, fcs, ["other"] * 3)
NB = B.n_faces
gen = torch.Generator(device=dev).manual_seed(12)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
K, nu = eng.sst_coeffs(), 1e-4
k, nut, V = R(N, 0.01, 1.0), R(N, 1e-4, 1e-2), R(N, 0.5e-3, 1.5e-3)
omega, y = 10.0 ** R(N, 0.0, 4.0), 10.0 ** R(N, -3.0, -1.0)                      # the ranges of tests/komegasst_support.inputs: every arm is taken
grad = [R(N, -10.0, 10.0) for _ in range(9)]
gk = [R(N, -1.0, 1.0) for _ in range(3)]
scale = 13.6 * omega * k / (y * y) * 10.0 ** R(N, -3.0, 1.0)
go = [scale * R(N, -0.5, 0.5) for _ in range(3)]
U = [R(N, -0.5, 0.5) for _ in range(3)]
bdc, bnuw, bnutw, by = R(NB, 50.0, 150.0), R(NB, 0.5e-5, 1.5e-5), R(NB, 0.0, 1e-4), 10.0 ** R(NB, -3.0, -1.0)
Uw = [R(NB, -0.1, 0.1) for _ in range(3)]
KE = eng.KEpsilon(addr, B, [True] * 3)
NW = KE.wall_cell_labels().numel()
S2, G, mag = E(N), E(N), E(N)
asm.sst_production(nut, grad, S2, G, mag)
o = [E(N) for _ in range(6)]
asm.sst_blend(K, False, gk, go, k, omega, y, nut, S2, nu, *o)
su, sp, susp = o[1].clone(), o[2].clone(), o[3].clone()
diag, source, Gw, omw, bom = R(N, 1.0, 2.0), R(N, -0.5, 0.5), G.clone(), omega.clone(), E(NB)
t = [E(N) for _ in range(9)]
lib, cx, ptr, I64 = eng.lib(), ctx.h, eng._ptr, C.c_int64(N)


def div(x, yy, out):
    eng._chk(lib.mi_vec_div(cx, I64, ptr(x), ptr(yy), ptr(out)))


def mul(x, yy, out):
    """out = -(x*yy): the one product the earlier entries can form"""
    out.zero_()
    asm.submul(x, yy, out)


def scal(a, x, out):
    asm.axpby(a, x, 0.0, x, out)


def unfused_blend():
    cd, y2, oy, y2o, a, b, c, m, p = t
    mul(gk[0], go[0], cd); asm.submul(gk[1], go[1], cd); asm.submul(gk[2], go[2], cd)
    scal(-K.twoAlphaOmega2, cd, cd); div(cd, omega, cd)
    asm.vec_max_value(cd, 1e-10, m)
    mul(y, y, y2); mul(omega, y, oy); mul(y2, omega, y2o)
    scal(K.invBetaStar, k, a); div(a, oy, a)                 # sqrt(k) left out
    scal(500.0 * nu, y2o, b); div(b, y2o, b)                 # a constant array over sqr(y)*omega: the scaling stands for forming it
    scal(K.fourAlphaOmega2, k, c); mul(m, y2, p); div(c, p, c)
    asm.vec_min(a, b, a); asm.vec_min(a, c, a)               # arg1 (pow4 and tanh left out): a stands for F1
    scal(K.twoInvBetaStar, k, c); div(c, oy, c); asm.vec_min(c, b, c)            # arg2 (sqr and tanh left out): c stands for F23
    scal(K.a1, omega, b); mul(c, S2, m); asm.vec_min(b, m, b)                    # the limiter (sqrt(S2) left out)
    scal(K.c1a1BetaStar, omega, m); mul(m, b, p); asm.vec_min(S2, p, b)
    asm.axpby(K.dGamma, a, K.gamma2, y2, m); mul(m, b, o[1])                     # su
    asm.axpby(K.dBeta, a, K.beta2, y2, m); mul(m, omega, o[2])                   # sp
    asm.axpby(1.0, a, -1.0, y2, m); mul(m, cd, p); div(p, omega, o[3])           # susp
    asm.axpby(K.dAlphaOmega, a, K.alphaOmega2, y2, m); mul(m, nut, p); asm.axpby(-1.0, p, nu, y2, o[4])
    asm.axpby(K.dAlphaK, a, K.alphaK2, y2, m); mul(m, nut, p); asm.axpby(-1.0, p, nu, y2, o[5])


def unfused_nut():
    _, y2, oy, y2o, a, b, c, m, _ = t
    mul(omega, y, oy); scal(K.twoInvBetaStar, k, c); div(c, oy, c)
    mul(y, y, y2); mul(y2, omega, y2o); scal(500.0 * nu, y2o, b); div(b, y2o, b)
    asm.vec_min(c, b, c)
    scal(K.a1, omega, b); mul(c, S2, m); asm.vec_min(b, m, b)
    scal(K.a1, k, a); div(a, b, o[0])


names = dict(bl="52 passes of zero fill / submul / axpby / vec_div / vec_min / vec_max_value", nt="17 passes of zero fill / submul / axpby / vec_div / vec_min",
             cp="copy of a cell array")
# per pass: zero fill 8N, submul 32N, axpby in place 16N or with two inputs 24N, vec_div 24N, vec_min 24N, vec_max_value 16N
yard_bytes = {names["bl"]: (12 * 8 + 14 * 32 + 7 * 16 + 7 * 24 + 6 * 24 + 5 * 24 + 16) * N, names["nt"]: (4 * 8 + 4 * 32 + 4 * 16 + 3 * 24 + 2 * 24) * N,
              names["cp"]: 16 * N}
variants = {
    names["bl"]: (unfused_blend, yard_bytes[names["bl"]], names["bl"]),
    names["nt"]: (unfused_nut, yard_bytes[names["nt"]], names["nt"]),
    names["cp"]: (lambda: t[0].copy_(k), yard_bytes[names["cp"]], names["cp"]),
    "sst_production": (lambda: asm.sst_production(nut, grad, S2, G), 96 * N, names["cp"]),
    "sst_production with mag": (lambda: asm.sst_production(nut, grad, S2, G, mag), 104 * N, names["cp"]),
    "sst_blend": (lambda: asm.sst_blend(K, False, gk, go, k, omega, y, nut, S2, nu, *o), 136 * N, names["bl"]),
    "sst_blend with F3": (lambda: asm.sst_blend(K, True, gk, go, k, omega, y, nut, S2, nu, *o), 136 * N, names["bl"]),
    "sst_omega_sources": (lambda: asm.sst_omega_sources(V, su, sp, susp, omega, diag, source), 72 * N, names["cp"]),
    "sst_k_terms": (lambda: asm.sst_k_terms(K, G, k, omega, o[0], o[1]), 40 * N, names["cp"]),
    "sst_nut": (lambda: asm.sst_nut(K, False, k, omega, y, S2, nu, o[0]), 40 * N, names["nt"]),
    "sst_nut with F3": (lambda: asm.sst_nut(K, True, k, omega, y, S2, nu, o[0]), 40 * N, names["nt"]),
    "sst_wall_cells": (lambda: asm.sst_wall_cells(KE, K, k, U, Uw, bdc, by, bnuw, bnutw, Gw, omw, bom), 80 * NW + 64 * NB, names["cp"]),
}
times = {name: [] for name in variants}
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
    res[name] = dict(us=round(us, 1), spread=round((max(times[name]) - min(times[name])) / us, 3), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3), yardstick=yard,
                     ratio_to_yardstick=round(statistics.median([x / x0 for x, x0 in zip(times[name], times[yard])]), 3),
                     byte_ratio=round(nbytes / yard_bytes[yard], 3))
line = json.dumps(dict(tool="bench_komegasst", dims=args.dims, addressing="ordered", cells=N, faces=F, boundary_faces=NB, wall_cells=NW, reps=args.reps,
                       iters=args.iters, variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
KE.close()
B.close()
