"""The LES block on the device (mi_les_simple_filter, the cell passes of Smagorinsky / oneEqEddy / dynOneEqEddy and the whole dynamic procedure)
on the 216^3 box renumbered into the engine's tile order (ordered addressing) -- device events on the engine's stream after a warm-up; in each
round every variant is timed in turn, all in one process, so the compared runs alternate; median of the rounds.  No counters, no trace.
  simple_filter n   n = 1, 3, 6, 9 components in one launch, against (a) n pairs of mi_face_interpolate + mi_fvc_average, the engine's own
                    unfused sequence, and (b) n single-component launches of itself
  dynamic chain     dynOneEqEddy.C:56-100 with :151-152: four cell passes and five filter launches (9 + 8, 9 + 5, 2 components) over fixed
                    boundary arrays; and the same with the boundary's part (29 mi_patch_internal_field gathers and the three maps over the
                    boundary arrays).  Yardstick: the 33 pairs of mi_face_interpolate + mi_fvc_average that filter the same 33 components --
                    what earlier entries can form of the unfused sequence; it leaves out all of the reference's cell algebra
  cell passes       beside mi_ke_epsilon_terms
Algorithmic bytes (every array once; owner / neighbour counted for the face passes; b = per boundary face):
  simple_filter n   lambda, magSf, owner / neighbour 24F; n fields read and written, surfaceSum(magSf) (16n + 8)N; (8 + 8n)b
  pair              mi_face_interpolate 24F + 8N, mi_fvc_average 16F + 16N -> 40F + 24N (+ 16b)
  a cell pass       8N per array read or written
Prints one JSON line and writes <out-dir>/les.json and les.md.  `--reps 2 --iters 3` for a run under a profiler."""
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
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--caller", action="store_true", help="the caller's numbering as it is (fixed blocks of cells) instead of ordered addressing")
ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"), help="where les.json and les.md go")
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
fc = np.repeat(np.arange(N, dtype=np.int32), np.maximum(missing, 0))       # one boundary face per missing side, in cell order: one patch
NB = fc.shape[0]
boundary = eng.GradBoundary(addr, [fc], ["other"])
patch = eng.Patch(ctx, N, fc)
gen = torch.Generator(device=dev).manual_seed(13)
R = lambda m, a=0.0, b=1.0: torch.rand(m, dtype=torch.float64, device=dev, generator=gen) * (b - a) + a
E = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
Es = lambda k, m: [E(m) for _ in range(k)]

lam, magSf, bms = R(F, 0.3, 0.7), R(F, 0.5, 1.5), R(NB, 0.5, 1.5)
av = eng.Average(addr, boundary, magSf, bms)
vf, bvf, out9 = [R(N, -0.5, 0.5) for _ in range(9)], [R(NB, -0.5, 0.5) for _ in range(9)], Es(9, N)
face, avg = E(F), E(N)


def filt(vs, bvs, outs):
    av.les_simple_filter(lam, magSf, vs, outs, bms, bvs)


def pairs(vs, bvs):
    for x, bx in zip(vs, bvs):
        asm.face_interpolate(lam, x, face)
        asm.fvc_average(av, magSf, face, avg, bms, bx)


def singles(vs, bvs, outs):
    for x, bx, o in zip(vs, bvs, outs):
        filt([x], [bx], [o])


# the dynamic procedure
U, bU = [R(N, -0.5, 0.5) for _ in range(3)], [R(NB, -0.5, 0.5) for _ in range(3)]
grad, bgrad = [R(N, -10.0, 10.0) for _ in range(9)], [R(NB, -10.0, 10.0) for _ in range(9)]
delta, bdelta = R(N, 0.01, 0.02), torch.full((NB,), 1e-15, dtype=torch.float64, device=dev)
nueff, bnueff = R(N, 1e-4, 1e-2), R(NB, 1e-4, 1e-2)
k, nusgs = R(N, 0.01, 1.0), R(N, 1e-4, 1e-2)
sq, D, mu, md = Es(6, N), Es(6, N), E(N), E(N)
bsq, bD, bmu, bmd = Es(6, NB), Es(6, NB), E(NB), E(NB)
f1 = Es(17, N)
KK, LL, MM, num, den = E(N), Es(6, N), Es(6, N), E(N), E(N)
bKK, bLL, bMM, bnum, bden = E(NB), Es(6, NB), Es(6, NB), E(NB), E(NB)
f2 = Es(14, N)
lm, mmmm, blm, bmmmm, flm, fmmmm, ck, ce = E(N), E(N), E(NB), E(NB), E(N), E(N), E(N), E(N)
zg1, zg2 = Es(17, NB), Es(12, NB)
K = eng.les_coeffs()
G, sp, dk, eps_like = E(N), E(N), E(N), R(N, 0.1, 10.0)
su_ke, sp_ke, de_ke = E(N), E(N), E(N)
Kke = eng.ke_coeffs()
V, root = R(N, 1e-6, 2e-6), E(N)


def chain(with_boundary):
    asm.les_dyn_moments(U, grad, sq, mu, D, md)
    if with_boundary:
        asm.les_dyn_moments(bU, bgrad, bsq, bmu, bD, bmd)
    filt(U + sq, bU + bsq, f1[0:9])
    filt([mu] + D + [md], [bmu] + bD + [bmd], f1[9:17])
    asm.les_dyn_level1(1, delta, nueff, f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16], KK, LL, MM, num, den)
    if with_boundary:
        for x, o in zip(f1, zg1):
            patch.internal_field(x, o)
        asm.les_dyn_level1(1, bdelta, bnueff, zg1[0:3], zg1[3:9], zg1[9], zg1[10:16], zg1[16], bKK, bLL, bMM, bnum, bden)
    filt(LL + MM[0:3], bLL + bMM[0:3], f2[0:9])
    filt(MM[3:6] + [num, den], bMM[3:6] + [bnum, bden], f2[9:14])
    asm.les_dyn_level2(f2[0:6], f2[6:12], lm, mmmm)
    if with_boundary:
        for x, o in zip(f2[0:12], zg2):
            patch.internal_field(x, o)
        asm.les_dyn_level2(zg2[0:6], zg2[6:12], blm, bmmmm)
    filt([lm, mmmm], [blm, bmmmm], [flm, fmmmm])
    asm.les_dyn_coeffs(flm, fmmmm, f2[12], f2[13], ck, ce)


comps33 = U + sq + [mu] + D + [md] + LL + MM + [num, den] + [lm, mmmm]
bcomps33 = bU + bsq + [bmu] + bD + [bmd] + bLL + bMM + [bnum, bden] + [blm, bmmmm]
chain(True)                                                                  # every array of the yardstick holds values
filt_bytes = lambda n: 24 * F + (16 * n + 8) * N + (8 + 8 * n) * NB
pair_bytes = lambda n: n * (40 * F + 24 * N + 16 * NB)
ke, p33 = "mi_ke_epsilon_terms", "33 pairs of mi_face_interpolate + mi_fvc_average"
chain_bytes = (26 + 34 + 14 + 6) * 8 * N + filt_bytes(9) + filt_bytes(8) + filt_bytes(9) + filt_bytes(5) + filt_bytes(2)
variants = {ke: (lambda: asm.ke_epsilon_terms(Kke, G, eps_like, k, nusgs, 1e-5, su_ke, sp_ke, de_ke), 56 * N, ke)}
yard_bytes = {ke: 56 * N, p33: pair_bytes(33)}
for n in (1, 3, 6, 9):
    pn, sn = "%d pairs of mi_face_interpolate + mi_fvc_average" % n, "%d single-component mi_les_simple_filter" % n
    yard_bytes[pn], yard_bytes[sn] = pair_bytes(n), n * filt_bytes(1)
    variants[pn] = (lambda n=n: pairs(vf[:n], bvf[:n]), pair_bytes(n), pn)
    variants[sn] = (lambda n=n: singles(vf[:n], bvf[:n], out9[:n]), n * filt_bytes(1), sn)
    variants["simple_filter %d (against the pairs)" % n] = (lambda n=n: filt(vf[:n], bvf[:n], out9[:n]), filt_bytes(n), pn)
    variants["simple_filter %d (against single-component calls)" % n] = (lambda n=n: filt(vf[:n], bvf[:n], out9[:n]), filt_bytes(n), sn)
variants.update({
    p33: (lambda: pairs(comps33, bcomps33), pair_bytes(33), p33),
    "dynamic chain, cells (4 cell passes + 5 filter launches)": (lambda: chain(False), chain_bytes, p33),
    "dynamic chain with the boundary's maps and gathers": (lambda: chain(True), chain_bytes + (26 + 34 + 14 + 29 * 2) * 8 * NB, p33),
    "les_delta_cube_root_vol": (lambda: asm.les_delta_cube_root_vol(1.0, 0.0, V, root), 16 * N, ke),
    "les_smagorinsky (k and nuSgs)": (lambda: asm.les_smagorinsky(K, delta, grad, G, sp), 96 * N, ke),
    "les_k_terms": (lambda: asm.les_k_terms(K.ce, nusgs, grad, k, delta, 1e-5, G, sp, dk), 120 * N, ke),
    "les_k_terms (ce per cell)": (lambda: asm.les_k_terms(ce, nusgs, grad, k, delta, 1e-5, G, sp, dk), 128 * N, ke),
    "les_nusgs": (lambda: asm.les_nusgs(K.ck, k, delta, G), 24 * N, ke),
    "les_dyn_moments": (lambda: asm.les_dyn_moments(U, grad, sq, mu, D, md), 26 * 8 * N, ke),
    "les_dyn_level1": (lambda: asm.les_dyn_level1(1, delta, nueff, f1[0:3], f1[3:9], f1[9], f1[10:16], f1[16], KK, LL, MM, num, den), 34 * 8 * N, ke),
    "les_dyn_level2": (lambda: asm.les_dyn_level2(f2[0:6], f2[6:12], lm, mmmm), 14 * 8 * N, ke),
    "les_dyn_coeffs": (lambda: asm.les_dyn_coeffs(flm, fmmmm, f2[12], f2[13], ck, ce), 6 * 8 * N, ke),
})
times = {name: [] for name in variants}
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
                     ratio_to_yardstick=round(statistics.median([x / x0 for x, x0 in zip(times[name], times[yard])]), 3),
                     byte_ratio=round(nbytes / yard_bytes[yard], 3))
result = dict(tool="bench_les", dims=args.dims, addressing="caller" if args.caller else "ordered", cells=N, faces=F, boundary_faces=NB, reps=args.reps,
              iters=args.iters, variants=res)
line = json.dumps(result)
print(line)
os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "les.json"), "w") as f:
    f.write(line + "\n")
with open(os.path.join(args.out_dir, "les.md"), "w") as f:
    f.write("# The LES block on the device: tools/bench_les.py\n\n")
    f.write("%d x %d x %d box, %s addressing: %d cells, %d internal faces, %d boundary faces in one patch.  %d rounds of %d calls a window after a\n"
            "warm-up, the variants in turn in one process; median of the rounds, spread = (max - min)/median.  The yardsticks are entries the\n"
            "engine had before this block, or single-component calls of the filter itself.\n\n"
            % (args.dims[0], args.dims[1], args.dims[2], result["addressing"], N, F, NB, args.reps, args.iters))
    f.write("| variant | us | spread | bytes | of 8 TB/s | yardstick | time / yardstick | bytes / yardstick |\n|---|---|---|---|---|---|---|---|\n")
    for name, r in res.items():
        f.write("| %s | %.1f | %.3f | %d | %.3f | %s | %.3f | %.3f |\n" % (name, r["us"], r["spread"], r["bytes"], r["frac_8TBs"], r["yardstick"],
                                                                        r["ratio_to_yardstick"], r["byte_ratio"]))
av.close()
boundary.close()
