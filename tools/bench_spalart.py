"""The Spalart-Allmaras passes on the device (mi_sa_terms for RAS, DES, DDES and IDDES, mi_sa_nut, mi_sa_nut_spalding_wall) on the 216^3 box of
tools/bench_komegasst.py -- renumbered into the engine's tile order, the same three wall patches, device events on the engine's stream,
every variant timed in turn in each round, all in one process.  mi_sa_terms is set beside the RAS correct()'s expression composed from the
entries the engine had before it: mi_sst_production (its mag(symm(gradU)) stands in for mag(skew(gradU))), mi_vec_axpby, mi_vec_submul on a
zeroed array (a product; the zero fill is timed and counted), mi_vec_div, mi_vec_min, mi_vec_max_value.  Such a composition cannot form a
pow, and for the DES kinds no tanh, exp, pos / neg or two-field max: those passes are LEFT OUT, and the DES kinds are set beside the RAS
composition, which flatters the yardstick.  The bytes of the composition are counted pass by pass as it runs (zero fill 8N, submul 32N, axpby
in place 16N or with two inputs 24N, vec_div 24N, vec_min 24N, vec_max_value 16N, production with mag 104N).
Algorithmic bytes of the fused passes (every array once, nu a number, no optional output): terms RAS 152N, DES 160N, DDES 168N, IDDES 176N;
nut 24N; the wall pass 72 bytes per wall face and 24 per wall cell.  The composition is timed, not compared: a product whose
output is one of its operands works on the zeroed array.  Prints one JSON line as tools/bench_komegasst.py does."""
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
K, nu = eng.sa_coeffs(), 1e-5
# the ranges of tests/spalart_support.inputs: every arm is taken
nt, y = 10.0 ** R(N, -7.0, -2.0), 10.0 ** R(N, -4.0, 0.0)
delta, hmax, nusgs = 10.0 ** R(N, -3.0, -0.5), 10.0 ** R(N, -3.0, -0.5), 10.0 ** R(N, -6.0, -3.0)
grad = [R(N, -10.0, 10.0) for _ in range(9)]
gnt = [R(N, -5e-3, 5e-3) for _ in range(3)]
U = [R(N, -10.0, 10.0) for _ in range(3)]
Uw = [R(NB, -0.1, 0.1) for _ in range(3)]
bdc, bnuw, by, bnutw0 = R(NB, 20.0, 150.0), R(NB, 0.5e-5, 1.5e-5), 10.0 ** R(NB, -5.0, -1.0), 10.0 ** R(NB, -8.0, -1.0)
bnutw, biter = bnutw0.clone(), torch.zeros(NB, dtype=torch.int32, device=dev)
KE = eng.KEpsilon(addr, B, [True] * 3)
NW, NWF = KE.wall_cell_labels().numel(), NB
o = [E(N) for _ in range(5)]
t = [E(N) for _ in range(10)]
ones = torch.ones(N, dtype=torch.float64, device=dev)
lib, cx, ptr, I64 = eng.lib(), ctx.h, eng._ptr, C.c_int64(N)
count = [0]


def div(x, yy, out):
    count[0] += 24 * N
    eng._chk(lib.mi_vec_div(cx, I64, ptr(x), ptr(yy), ptr(out)))


def mul(x, yy, out):
    """out = -(x*yy): the one product the earlier entries can form"""
    count[0] += 40 * N
    out.zero_()
    asm.submul(x, yy, out)


def scal(a, x, out):
    count[0] += 16 * N
    asm.axpby(a, x, 0.0, x, out)


def lin(a, x, b, yy, out):
    count[0] += 24 * N
    asm.axpby(a, x, b, yy, out)


def vmin(x, yy, out):
    count[0] += 24 * N
    asm.vec_min(x, yy, out)


def unfused_ras():
    """SpalartAllmaras::correct() :437-455 as far as the earlier entries go: 79 passes, 24 of them zero fills; no pow"""
    chi, a, b, c, d, fv1, fv2, fv3, S2, mag = t
    scal(1.0 / nu, nt, chi); mul(chi, chi, a); mul(a, chi, b)                              # chi, chi3
    lin(1.0, b, K.Cv1_3, ones, a); div(b, a, fv1)
    lin(K.invCv2, chi, 1.0, ones, a); mul(a, a, b); mul(b, a, c); div(ones, c, fv2)        # fv2
    scal(K.invCv2, chi, a); lin(1.0, a, 1.0, ones, b); mul(a, a, c); lin(3.0, b, 1.0, c, c)   # fv3
    mul(chi, fv1, d); lin(K.invCv2, d, K.invCv2, ones, d); mul(d, c, c)
    mul(b, b, d); mul(d, b, d); div(c, d, fv3)
    count[0] += 104 * N
    asm.sst_production(nt, grad, S2, d, mag)                                                # mag(symm) for mag(skew)
    scal(K.sqrt2, fv3, a); mul(a, mag, a)                                                   # Stilda
    scal(K.kappa, y, b); mul(b, b, b); mul(fv2, nt, c); div(c, b, c); lin(1.0, a, 1.0, c, a)
    count[0] += 16 * N
    asm.vec_max_value(a, 1e-15, c)                                                          # r
    mul(c, b, c); div(nt, c, c); lin(10.0, ones, 0.0, ones, d); vmin(c, d, c)
    mul(c, c, d); mul(d, d, b); mul(b, d, b); lin(K.Cw2, b, -K.Cw2, c, b); lin(1.0, c, 1.0, b, b)   # g
    mul(b, b, d); mul(d, d, c); mul(c, d, c); lin(1.0, c, K.Cw3_6, ones, c); lin(K.onePlusCw3_6, ones, 0.0, ones, d); div(d, c, c)
    mul(b, c, b)                                                                            # fw (pow left out)
    mul(gnt[0], gnt[0], c); count[0] += 64 * N; asm.submul(gnt[1], gnt[1], c); asm.submul(gnt[2], gnt[2], c); scal(K.Cb2BySigmaNut, c, o[0])
    scal(K.Cb1, a, c); mul(c, nt, o[1])
    scal(K.Cw1, b, c); mul(c, nt, c); mul(y, y, d); div(c, d, o[2])
    lin(1.0 / K.sigmaNut, nt, nu / K.sigmaNut, ones, o[3])


def terms(kind):
    return lambda: asm.sa_terms(K, kind, True, nt, grad, gnt, y, nu, *o, delta=delta, nusgs=nusgs, hmax=hmax)


def wall():
    bnutw.copy_(bnutw0)
    asm.sa_nut_spalding_wall(KE, K, U, Uw, bdc, by, bnuw, bnutw)


unfused_ras()
torch.cuda.synchronize()
yard, cp, wc = "the RAS expression in passes of the earlier entries", "copy of a cell array", "copy of a boundary array"
yard_bytes = {yard: count[0], cp: 16 * N, wc: 16 * NB}
variants = {
    yard: (unfused_ras, yard_bytes[yard], yard),
    cp: (lambda: t[0].copy_(nt), 16 * N, cp),
    wc: (lambda: bnutw.copy_(bnutw0), 16 * NB, wc),
    "sa_terms RAS": (terms("RAS"), 152 * N, yard),
    "sa_terms DES": (terms("DES"), 160 * N, yard),
    "sa_terms DDES": (terms("DDES"), 168 * N, yard),
    "sa_terms IDDES": (terms("IDDES"), 176 * N, yard),
    "sa_nut (fv1 recomputed)": (lambda: asm.sa_nut(K, nt, o[0], nu=nu), 16 * N, cp),
    "sa_nut (fv1 stored)": (lambda: asm.sa_nut(K, nt, o[0], fv1=o[4]), 24 * N, cp),
    "sa_nut_spalding_wall (with the copy that resets nutw)": (wall, 16 * NB + 72 * NWF + 24 * NW, wc),
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
asm.sa_nut_spalding_wall(KE, K, U, Uw, bdc, by, bnuw, bnutw0.clone(), None, biter)
torch.cuda.synchronize()
res = {}
for name, (_, nbytes, yd) in variants.items():
    us = statistics.median(times[name])
    res[name] = dict(us=round(us, 1), spread=round((max(times[name]) - min(times[name])) / us, 3), bytes=nbytes,
                     frac_8TBs=round(nbytes / (us * 1e-6) / 8e12, 3), yardstick=yd,
                     ratio_to_yardstick=round(statistics.median([x / x0 for x, x0 in zip(times[name], times[yd])]), 3),
                     byte_ratio=round(nbytes / yard_bytes[yd], 3))
line = json.dumps(dict(tool="bench_spalart", dims=args.dims, addressing="ordered", cells=N, faces=F, boundary_faces=NB, wall_cells=NW, reps=args.reps,
                       iters=args.iters, mean_newton_steps=round(float(biter.double().mean()), 2), variants=res))
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
KE.close()
B.close()
