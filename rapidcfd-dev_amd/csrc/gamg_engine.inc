// gamg_engine.inc -- GAMG solver on the engine (included at the end of engine.hip).
//
// Reference: solvers/GAMG/GAMGSolver.C:47-249 (controls, level matrices rebuilt per solver
// construction), GAMGSolverSolve.C:59-619 (solve, Vcycle, coarsest level), GAMGSolverScale.C:59-171,
// GAMGSolverAgglomerateMatrix.C:37-321, GAMGAgglomerationTemplates.C:35-153,273-308.
// MI355X form: every level is an ordinary engine matrix (tiled layout, tile_kernel for Amul and the
// Jacobi smoother); restriction / prolongation / coefficient agglomeration are segmented gathers over
// children lists precomputed in engine order; the coarsest level is solved on the device with a
// precomputed dense inverse (replaces the host LU round trip of GAMGSolverSolve.C:564-570), so a
// V-cycle never leaves the GPU; the host reads one scalar (the residual) per cycle.
#include "gamg.hpp"
#include "host_parallel.hpp"
#include <chrono>
#include <memory>
#include <thread>

namespace mi {

__global__ void k_gamg_restrict(const double* __restrict__ ff, const int32_t* __restrict__ start,
                                const int32_t* __restrict__ child, double* __restrict__ cf, int n)
{
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        double out = 0.0; // GAMGAgglomerationF.H:9-38: zero, then children in ascending fine index
        for (int k = start[c]; k < start[c + 1]; ++k) out += ff[child[k]];
        cf[c] = out;
    }
}
__global__ void k_gamg_prolong(const double* __restrict__ cf, const int32_t* __restrict__ map, double* __restrict__ ff, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) ff[i] = cf[map[i]];
}
// coarse upper/lower (caller order of the coarse level): GAMGSolverAgglomerateMatrixF.H:9-54,103-131
__global__ void k_gamg_agg_faces(const double* __restrict__ fUp, const double* __restrict__ fLow, const int32_t* __restrict__ fIdx,
                                 const uint8_t* __restrict__ flip, const int32_t* __restrict__ start, const int32_t* __restrict__ child,
                                 double* __restrict__ cUp, double* __restrict__ cLow, int n)
{
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        double uc = 0.0, lc = 0.0;
        for (int k = start[t]; k < start[t + 1]; ++k) {
            const int f = child[k];
            const int s = fIdx ? fIdx[f] : f;
            if (!fLow) uc += fUp[s];
            else if (!flip[f]) { uc += fUp[s]; lc += fLow[s]; }
            else { uc += fLow[s]; lc += fUp[s]; }
        }
        cUp[t] = uc;
        if (cLow) cLow[t] = lc;
    }
}
// coarse diag = restrict(fine diag) + sum over fine faces inside the coarse cell (2*upper | upper+lower)
__global__ void k_gamg_agg_diag(const double* __restrict__ fDiag, const int32_t* __restrict__ dIdx,
                                const int32_t* __restrict__ cStart, const int32_t* __restrict__ cChild,
                                const double* __restrict__ fUp, const double* __restrict__ fLow, const int32_t* __restrict__ fIdx,
                                const int32_t* __restrict__ iStart, const int32_t* __restrict__ iChild,
                                double* __restrict__ cDiag, int n)
{
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        double out = 0.0;
        for (int k = cStart[c]; k < cStart[c + 1]; ++k) { const int i = cChild[k]; out += fDiag[dIdx ? dIdx[i] : i]; }
        for (int k = iStart[c]; k < iStart[c + 1]; ++k) {
            const int f = iChild[k];
            const int s = fIdx ? fIdx[f] : f;
            if (!fLow) out += 2 * fUp[s];
            else out += fUp[s] + fLow[s];
        }
        cDiag[c] = out;
    }
}
// coarse interface coefficients = sum of the fine ones of the same coarse interface face, ascending fine face
// (GAMGInterface::agglomerateCoeffs, interfaces/GAMGInterface/GAMGInterface.C + GAMGInterfaceFunctors.H:8-60).
// Works on the engine's slot values (= -coeff), writes the coarse slots and a patch-ordered copy.
__global__ void k_gamg_agg_iface(const double* __restrict__ fUp, const double* __restrict__ fLow, const int32_t* __restrict__ fExtSlot,
                                 const int32_t* __restrict__ start, const int32_t* __restrict__ child,
                                 const int32_t* __restrict__ cExtSlot, double* __restrict__ cUp, double* __restrict__ cLow,
                                 double* __restrict__ ifUp, int n)
{
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        double u = 0.0, l = 0.0;
        for (int k = start[t]; k < start[t + 1]; ++k) { const int sl = fExtSlot[child[k]]; u += fUp[sl]; if (fLow) l += fLow[sl]; }
        const int cs = cExtSlot[t];
        cUp[cs] = u;
        if (cLow) cLow[cs] = l;
        ifUp[t] = u;
    }
}
// Round 4: the level matrices straight into the coarse level's ENGINE arrays (tile slots, engine-order diagonal) from the fine
// level's engine arrays, through children lists that name fine SLOTS / fine engine cells directly.  Round 3 went through the
// coarse level's caller-order arrays -- agglomerate (fine face -> slot lookup per child), write cUp / cDiag, then
// mi_matrix_set_coeffs (slot -> face lookup, gather, permute the diagonal): five launches and ~1.25 GB at the first level of
// the 10 M-cell box; this is two launches and ~0.75 GB.  Same children in the same (ascending fine face) order: same bits.
// child: fine slot | flip << 31 (asymmetric matrices: a flipped fine face contributes its lower to the coarse upper, its upper
// to the coarse lower -- GAMGSolverAgglomerateMatrixF.H:103-131).  Interface slots (slotFace <= -2) belong to k_gamg_agg_iface.
__global__ void k_gamg_agg_slots(const double* __restrict__ fUp, const double* __restrict__ fLow, const int32_t* __restrict__ slotFace,
                                 const int32_t* __restrict__ start, const uint32_t* __restrict__ child,
                                 double* __restrict__ cUp, double* __restrict__ cLow, int64_t nSlots)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nSlots; k += (int64_t)gridDim.x * blockDim.x) {
        if (slotFace[k] <= -2) continue;
        double uc = 0.0, lc = 0.0;
        for (int j = start[k]; j < start[k + 1]; ++j) {
            const uint32_t c = child[j];
            const uint32_t sl = c & 0x7FFFFFFFu;
            if (!fLow) uc += fUp[sl];
            else if (!(c >> 31)) { uc += fUp[sl]; lc += fLow[sl]; }
            else { uc += fLow[sl]; lc += fUp[sl]; }
        }
        cUp[k] = uc;
        if (cLow) cLow[k] = lc;
    }
}
// coarse diagonal, engine order of both levels: restrict(fine diag) over the restriction's own children list (ascending fine
// cell), then the fine faces inside the coarse cell (2*upper | upper + lower), by slot
__global__ void k_gamg_agg_diag_e(const double* __restrict__ fDiagE, const int32_t* __restrict__ rStart, const int32_t* __restrict__ rChild,
                                  const double* __restrict__ fUp, const double* __restrict__ fLow,
                                  const int32_t* __restrict__ iStart, const int32_t* __restrict__ iChildSlot, double* __restrict__ cDiagE, int n)
{
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        double out = 0.0;
        for (int k = rStart[c]; k < rStart[c + 1]; ++k) out += fDiagE[rChild[k]];
        for (int k = iStart[c]; k < iStart[c + 1]; ++k) {
            const int sl = iChildSlot[k];
            if (!fLow) out += 2 * fUp[sl];
            else out += fUp[sl] + fLow[sl];
        }
        cDiagE[c] = out;
    }
}
// coarsest level: local source into its block of the global vector (caller order of the coarsest level)
__global__ void k_gamg_scatter_offset(const double* __restrict__ srcE, const int32_t* __restrict__ e2c, double* __restrict__ g, int64_t off, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) g[off + e2c[i]] = srcE[i];
}
// GAMGSolverScale.C:40-57,139-170: sf = num/stabilise(den); field = sf*field + (source - sf*Acf)/D
// DIST: pNum/pDen hold the two global sums (after the all-reduce) instead of per-block partials
// addTo != nullptr (finest level): the scaled correction is added to psi in the same pass (psi += finestCorrection,
// GAMGSolverSolve.C:130-138) and not stored -- nothing reads the correction field afterwards
template <bool DIST>
__global__ __launch_bounds__(RB) void k_gamg_scale(double* __restrict__ field, const double* __restrict__ Acf,
                                                   const double* __restrict__ source, const double* __restrict__ D,
                                                   const double* __restrict__ pNum, const double* __restrict__ pDen, int64_t n,
                                                   double* __restrict__ addTo = nullptr)
{
    __shared__ double red[RB / 64];
    const double num = DIST ? pNum[0] : sum_partials(pNum, red);
    const double den = DIST ? pDen[0] : sum_partials(pDen, red);
    const double sf = num / (den >= 0 ? den + SP_VSMALL : den - SP_VSMALL);
    chunk_loop(n, [&](int64_t i) {
            const double2 f = ld2(field, i), a = ld2(Acf, i), s = ld2(source, i), d = ld2(D, i);
            const double2 v = make_double2(fma(sf, f.x, fma(-sf, a.x, s.x) / d.x), fma(sf, f.y, fma(-sf, a.y, s.y) / d.y));
            if (addTo) { const double2 p = ld2(addTo, i); st2(addTo, i, make_double2(p.x + v.x, p.y + v.y)); } // k_xpsy with s = 1: fma(1, v, p) == p + v
            else st2(field, i, v);
        },
        [&](int64_t i) { const double v = fma(sf, field[i], fma(-sf, Acf[i], source[i]) / D[i]); if (addTo) addTo[i] += v; else field[i] = v; });
}
// out = inv * src: one wavefront per row of this rank's block of the global inverse (row-major, rows in engine order);
// lanes stride over the columns, fixed-shape wave reduction => deterministic.  Replaces the host LU round trip of
// GAMGSolverSolve.C:564-570.
__global__ __launch_bounds__(256) void k_dense_matvec(const double* __restrict__ inv, const double* __restrict__ src, double* __restrict__ out, int n, int nCols)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double* r = inv + (size_t)row * nCols;
    double acc = 0.0;
    for (int j = lane; j < nCols; j += 64) acc = fma(r[j], src[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[row] = acc;
}

// ---- coarsest level on the device: assemble this rank's block rows of the global matrix, invert, keep own rows ----------
// (replaces the reference's host LU, GAMGSolver.C:144-172 + LUscalarMatrix.C, and this engine's earlier host inversion)
__global__ void k_coarsest_assemble(double* __restrict__ A, int64_t nG, int64_t off, const double* __restrict__ diag,
                                    const int32_t* __restrict__ cl, const int32_t* __restrict__ cu, const double* __restrict__ up,
                                    const double* __restrict__ low /* nullptr: symmetric */, int n, int nf,
                                    const int32_t* __restrict__ ifRow, const int64_t* __restrict__ ifCol, const double* __restrict__ ifVal, int nx)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
    for (int i = t; i < n; i += T) A[(size_t)(off + i) * nG + (size_t)(off + i)] = diag[i];
    for (int f = t; f < nf; f += T) {
        A[(size_t)(off + cl[f]) * nG + (size_t)(off + cu[f])] = up[f];
        A[(size_t)(off + cu[f]) * nG + (size_t)(off + cl[f])] = low ? low[f] : up[f];
    }
    // coupled faces: row -= interfaceBouCoeffs (the slot value is already -coeff); a few dozen entries, added in patch order
    // by ONE thread so that entries hit by several faces get their terms in a fixed order
    if (t == 0) for (int k = 0; k < nx; ++k) A[(size_t)(off + ifRow[k]) * nG + (size_t)ifCol[k]] += ifVal[k];
}
// Gauss-Jordan with partial pivoting, one workgroup; A (n x n) is destroyed, Inv receives the inverse.  status[0] = 1 when a
// pivot is exactly zero (singular).  Every rank of a decomposed case runs this on the same matrix: same code, same bits.
__global__ __launch_bounds__(1024) void k_dense_invert(double* __restrict__ A, double* __restrict__ Inv, int n, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double col[];   // n doubles: column k of A before the elimination step
    __shared__ double redV[16]; __shared__ int redI[16];
    __shared__ int pivRow; __shared__ double pivInv;
    const int tid = threadIdx.x, T = blockDim.x;
    for (size_t e = tid; e < (size_t)n * n; e += T) Inv[e] = (e / n == e % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        // pivot: largest |A[i][k]|, i >= k, the smallest i among equals
        double bv = -1.0; int bi = n;
        for (int i = k + tid; i < n; i += T) { const double v = fabs(A[(size_t)i * n + k]); if (v > bv) { bv = v; bi = i; } }
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bv, m, 64); const int oi = __shfl_xor(bi, m, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { redV[tid >> 6] = bv; redI[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            double v = redV[0]; int ix = redI[0];
            for (int w = 1; w < T / 64; ++w) if (redV[w] > v || (redV[w] == v && redI[w] < ix)) { v = redV[w]; ix = redI[w]; }
            pivRow = ix;
            if (!(v > 0.0)) { status[0] = 1; pivInv = 0.0; } else pivInv = 1.0 / A[(size_t)ix * n + k];
        }
        __syncthreads();
        const int p = pivRow;
        if (pivInv == 0.0) return;
        // swap rows k <-> p, scale row k by 1/pivot (both matrices)
        for (int j = tid; j < 2 * n; j += T) {
            double* M = j < n ? A : Inv; const int jj = j < n ? j : j - n;
            const double a = M[(size_t)k * n + jj], b = M[(size_t)p * n + jj];
            M[(size_t)p * n + jj] = a;
            M[(size_t)k * n + jj] = b * pivInv;
        }
        __syncthreads();
        for (int i = tid; i < n; i += T) col[i] = A[(size_t)i * n + k];
        __syncthreads();
        // eliminate column k from every other row
        for (size_t e = tid; e < (size_t)n * (size_t)(2 * n); e += T) {
            const int i = (int)(e / (size_t)(2 * n)), j = (int)(e % (size_t)(2 * n));
            if (i == k) continue;
            const double m = col[i];
            if (m == 0.0) continue;
            double* M = j < n ? A : Inv; const int jj = j < n ? j : j - n;
            M[(size_t)i * n + jj] -= m * M[(size_t)k * n + jj];
        }
        __syncthreads();
    }
}
// The same inversion with the matrix in REGISTERS (round 3): n <= TG TR, thread (ty, tx) of a TG x TG grid owns the elements
// (ty + TG a, tx + TG b) (TG = 32: 1 024 threads; a 16 x 16 grid of four wavefronts was tried in round 4 and is slower: 1.04 against 0.89 ms at 151 cells); per pivot step three barriers and a few hundred bytes of LDS (pivot candidates, the pivot row, the
// pivot column) instead of five dependent round trips to global memory: 151 cells 3.9 ms -> a fraction of a millisecond.
// In-place Gauss-Jordan with partial pivoting: column k of the registers holds, from step k on, the column of the inverse that
// belongs to the ORIGINAL row picked as k-th pivot (the one non-trivial column the identity half of the augmented matrix gains
// in that step); the operations on every element are those of the host's augmented elimination (gamg.cpp invert_dense:
// scale by 1/pivot, a -= m * r unfused), so both paths give the same bits, as do all ranks of a decomposed case.
template <int TR, int TG>
__global__ __launch_bounds__(TG * TG) void k_dense_invert_reg(const double* __restrict__ A, double* __restrict__ Inv, int n, int* __restrict__ status)
{
    __shared__ double rowK[TG * TR], rowP[TG * TR], colK[TG * TR], candV[TG];
    __shared__ int candI[TG], perm[TG * TR];
    const int tx = threadIdx.x % TG, ty = threadIdx.x / TG;
    double a[TR][TR];
#pragma unroll
    for (int ai = 0; ai < TR; ++ai)
#pragma unroll
        for (int bj = 0; bj < TR; ++bj) {
            const int i = ty + TG * ai, j = tx + TG * bj;
            a[ai][bj] = (i < n && j < n) ? A[(size_t)i * n + j] : (i == j ? 1.0 : 0.0);
        }
    for (int t = threadIdx.x; t < TG * TR; t += TG * TG) perm[t] = t;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        const int ka = k / TG, kt = k % TG;
        if (tx == kt) { // pivot candidates of the owners of column k: largest |A[i][k]|, i >= k, the smallest i among equals
            double bv = -1.0; int bi = 1 << 30;
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) {
                const int i = ty + TG * ai;
                double v = 0.0;
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) if (bj == ka) v = fabs(a[ai][bj]);
                if (i >= k && i < n && v > bv) { bv = v; bi = i; }
            }
            candV[ty] = bv; candI[ty] = bi;
        }
        __syncthreads();
        double bv = -1.0; int p = k;
#pragma unroll 8
        for (int q = 0; q < TG; ++q) { const double v = candV[q]; const int i = candI[q]; if (v > bv || (v == bv && i < p)) { bv = v; p = i; } }
        if (!(bv > 0.0)) { if (threadIdx.x == 0) status[0] = 1; return; }   // singular: every thread takes this exit
        const int pa = p / TG, pt = p % TG;
        if (ty == kt) {
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) if (ai == ka) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) rowK[tx + TG * bj] = a[ai][bj];
            }
        }
        if (ty == pt) {
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) if (ai == pa) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) rowP[tx + TG * bj] = a[ai][bj];
            }
        }
        if (threadIdx.x == 0) { const int t = perm[k]; perm[k] = perm[p]; perm[p] = t; }
        __syncthreads();
        const double inv = 1.0 / rowP[k];
        if (ty == pt && p != k) { // row p takes the old row k
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) if (ai == pa) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) a[ai][bj] = rowK[tx + TG * bj];
            }
        }
        if (ty == kt) { // row k = the pivot row scaled; its slot k is the identity half's 1 * (1 / pivot)
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) if (ai == ka) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) { const int j = tx + TG * bj; a[ai][bj] = (j == k ? 1.0 : rowP[j]) * inv; }
            }
        }
        if (tx == kt) { // the multipliers: column k after the swap
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) if (bj == ka) colK[ty + TG * ai] = a[ai][bj];
            }
        }
        __syncthreads();
#pragma unroll
        for (int ai = 0; ai < TR; ++ai) {
            const int i = ty + TG * ai;
            const double m = colK[i];
            if (i == k || m == 0.0) continue;
#pragma unroll
            for (int bj = 0; bj < TR; ++bj) {
                const int j = tx + TG * bj;
                const double r = (j == k ? 1.0 : rowP[j]) * inv;
                a[ai][bj] = (j == k ? 0.0 : a[ai][bj]) - m * r;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int ai = 0; ai < TR; ++ai)
#pragma unroll
        for (int bj = 0; bj < TR; ++bj) {
            const int i = ty + TG * ai, j = tx + TG * bj;
            if (i < n && j < n) Inv[(size_t)i * n + perm[j]] = a[ai][bj];
        }
}
// Round 6: the same elimination, the same operations on every element (so the same bits as the host's and as k_dense_invert_reg), with the
// pivot step's INSTRUCTION STREAM cut down -- one CU issues for 16 wavefronts, and round 4 measured that the step is bound by that, not by
// its barriers (5.7 us per pivot at 151 cells: 0.87 ms on the critical path of every pressure solve of a time step, where the prologue and
// the first restriction sweep hide 0.49 ms of it):
//   * the pivot column block ka = k / 32 is a COMPILE-TIME constant (the k loop is unrolled over it), so reading column k of the
//     register tile costs nothing instead of TR selects per row;
//   * the owners of column k publish it BEFORE the row swap (colPre) together with their pivot candidates; the multiplier of a row is
//     read from there (row p, which receives the old row k, takes colPre[k]): the third barrier of a step and the colK round trip are gone
//     (colPre / candidates are double-buffered by the parity of k, so the next step's owners may write while a slow wavefront still reads);
//   * the 32 pivot candidates are reduced by a swizzle butterfly (one candidate per lane, five steps) instead of a 32-entry scan per thread;
//   * 1 / pivot is formed once, by the thread that holds the pivot, not by 1 024 threads.
template <int TR>
__global__ __launch_bounds__(1024) void k_dense_invert_reg2(const double* __restrict__ A, double* __restrict__ Inv, int n, int* __restrict__ status)
{
    constexpr int TG = 32;
    __shared__ double rowK[TG * TR], rowP[TG * TR], colPre[2][TG * TR], candV[2][TG], invS;
    __shared__ int candI[2][TG], perm[TG * TR];
    const int tx = threadIdx.x % TG, ty = threadIdx.x / TG;
    double a[TR][TR];
#pragma unroll
    for (int ai = 0; ai < TR; ++ai)
#pragma unroll
        for (int bj = 0; bj < TR; ++bj) {
            const int i = ty + TG * ai, j = tx + TG * bj;
            a[ai][bj] = (i < n && j < n) ? A[(size_t)i * n + j] : (i == j ? 1.0 : 0.0);
        }
    for (int t = threadIdx.x; t < TG * TR; t += TG * TG) perm[t] = t;
    __syncthreads();
#pragma unroll
    for (int ka = 0; ka < TR; ++ka) {
        for (int kt = 0; kt < TG; ++kt) {
            const int k = ka * TG + kt;
            if (k >= n) break;
            const int q = kt & 1;
            if (tx == kt) { // column k before the swap, and the owners' pivot candidates: largest |A[i][k]|, i >= k, the smallest i among equals
                double bv = -1.0; int bi = 1 << 30;
#pragma unroll
                for (int ai = 0; ai < TR; ++ai) {
                    const int i = ty + TG * ai;
                    const double c = a[ai][ka];
                    colPre[q][i] = c;
                    const double v = fabs(c);
                    if (i >= k && i < n && v > bv) { bv = v; bi = i; }
                }
                candV[q][ty] = bv; candI[q][ty] = bi;
            }
            __syncthreads();
            double bv = candV[q][tx]; int p = candI[q][tx];       // lane tx of either half holds candidate tx: butterfly over the 32
#pragma unroll
            for (int sh = 0; sh < 5; ++sh) {
                double ov; int op;
                switch (sh) {
                case 0: ov = swz_xor<1>(bv); op = __builtin_amdgcn_ds_swizzle(p, 0x1f | (1 << 10)); break;
                case 1: ov = swz_xor<2>(bv); op = __builtin_amdgcn_ds_swizzle(p, 0x1f | (2 << 10)); break;
                case 2: ov = swz_xor<4>(bv); op = __builtin_amdgcn_ds_swizzle(p, 0x1f | (4 << 10)); break;
                case 3: ov = swz_xor<8>(bv); op = __builtin_amdgcn_ds_swizzle(p, 0x1f | (8 << 10)); break;
                default: ov = swz_xor<16>(bv); op = __builtin_amdgcn_ds_swizzle(p, 0x1f | (16 << 10)); break;
                }
                if (ov > bv || (ov == bv && op < p)) { bv = ov; p = op; }
            }
            if (!(bv > 0.0)) { if (threadIdx.x == 0) status[0] = 1; return; }   // singular: every thread takes this exit
            const int pa = p / TG, pt = p % TG;
            if (ty == kt) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) rowK[tx + TG * bj] = a[ka][bj];
            }
            if (ty == pt) {
#pragma unroll
                for (int ai = 0; ai < TR; ++ai) if (ai == pa) {
#pragma unroll
                    for (int bj = 0; bj < TR; ++bj) rowP[tx + TG * bj] = a[ai][bj];
                    if (tx == kt) invS = 1.0 / a[ai][ka];
                }
            }
            if (threadIdx.x == 0) { const int t = perm[k]; perm[k] = perm[p]; perm[p] = t; }
            __syncthreads();
            const double inv = invS;
            double r[TR];
#pragma unroll
            for (int bj = 0; bj < TR; ++bj) r[bj] = ((bj == ka && tx == kt) ? 1.0 : rowP[tx + TG * bj]) * inv;   // the pivot row scaled; its slot k is the identity half's 1 * (1 / pivot)
            if (ty == pt && p != k) { // row p takes the old row k
#pragma unroll
                for (int ai = 0; ai < TR; ++ai) if (ai == pa) {
#pragma unroll
                    for (int bj = 0; bj < TR; ++bj) a[ai][bj] = rowK[tx + TG * bj];
                }
            }
            if (ty == kt) {
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) a[ka][bj] = r[bj];
            }
            const double mOldK = colPre[q][k];
#pragma unroll
            for (int ai = 0; ai < TR; ++ai) {
                const int i = ty + TG * ai;
                const double m = (i == p) ? mOldK : colPre[q][i];   // column k after the swap (i == p == k is skipped below)
                if (i == k || m == 0.0) continue;
#pragma unroll
                for (int bj = 0; bj < TR; ++bj) a[ai][bj] = ((bj == ka && tx == kt) ? 0.0 : a[ai][bj]) - m * r[bj];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int ai = 0; ai < TR; ++ai)
#pragma unroll
        for (int bj = 0; bj < TR; ++bj) {
            const int i = ty + TG * ai, j = tx + TG * bj;
            if (i < n && j < n) Inv[(size_t)i * n + perm[j]] = a[ai][bj];
        }
}
// two per-tile partial arrays -> two scalars (k_fold_final's arithmetic; block b folds array b)
__global__ __launch_bounds__(1024) void k_fold_final2(const double* __restrict__ inA, const double* __restrict__ inB, int n, double* __restrict__ out)
{
    __shared__ double lds[RG + RB / 64];
    const double tot = fold_final_block<1024>(blockIdx.x == 0 ? inA : inB, n, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}
// ... and, on a communicator in peer mode, all-reduced through the windows in the same launch (one workgroup; N = 1: inB unused).
// GAMGSolverScale.C:104-107 (the 2-double reduce of the scaling factor), GAMGSolverSolve.C:146-160 (gSumMag of the finest residual)
template <int N>
__global__ __launch_bounds__(1024) void k_fold_ar(const double* __restrict__ inA, const double* __restrict__ inB, int n, double* __restrict__ out, const PeerAR ar)
{
    __shared__ double lds[RG + RB / 64];
    double v[N];
    v[0] = fold_final_block<1024>(inA, n, lds);
    if (N > 1) { __syncthreads(); v[N - 1] = fold_final_block<1024>(inB, n, lds); }
    if (threadIdx.x < 64) {
        peer_ar_wave<N>(ar, v, N);
        if (threadIdx.x == 0) { out[0] = v[0]; if (N > 1) out[N - 1] = v[N - 1]; }
    }
}
// Coarsest level of a decomposed case (GAMGSolverSolve.C:552-570: every processor's coarsest source gathered onto the master,
// LUscalarMatrix::solve, scattered back).  Here every rank holds its rows of the global inverse and needs the GLOBAL source:
// an all-gather of <= 4096 doubles.  Over peer windows it is ONE small kernel per rank -- each rank stores its block into every
// rank's gather window ([2 parities][nG] values + [2][nRanks] epoch flags, fine-grained, mapped over hipIpc like the halo
// windows) and raises its flag there -- and the matvec waits for the nRanks flags of its own window and reads the source from
// it: no collective call, so the V-cycle of a decomposed case stays stream work and replays as a hipGraph.
struct GatherDev {
    double* const* peerWin; const double* myWin; unsigned long long* epoch; int32_t* status;
    int32_t nRanks, myRank; int64_t nG; long long maxPolls;
};
__global__ __launch_bounds__(256) void k_coarsest_gather_push(const double* __restrict__ srcE, const int32_t* __restrict__ e2c, int n, int64_t off, const GatherDev W)
{
    const unsigned long long e = *W.epoch + 1;
    const int par = (int)(e & 1ull);
    for (int k = 0; k < W.nRanks; ++k) {
        double* dst = W.peerWin[k] + (size_t)par * (size_t)W.nG + (size_t)off;
        for (int i = threadIdx.x; i < n; i += blockDim.x) __hip_atomic_store(dst + e2c[i], srcE[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __threadfence_system();
    __syncthreads();
    if ((int)threadIdx.x < W.nRanks) {
        unsigned long long* flags = reinterpret_cast<unsigned long long*>(W.peerWin[threadIdx.x] + 2 * (size_t)W.nG);
        __hip_atomic_store(flags + (size_t)par * W.nRanks + W.myRank, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) *W.epoch = e;
}
// k_dense_matvec with the source read from this rank's gather window (every wave waits for the ranks' flags itself)
__global__ __launch_bounds__(256) void k_dense_matvec_win(const double* __restrict__ inv, const GatherDev W, double* __restrict__ out, int n, int nCols)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const unsigned long long e = *W.epoch;
    const int par = (int)(e & 1ull);
    if (lane < W.nRanks) {
        const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(W.myWin + 2 * (size_t)W.nG) + (size_t)par * W.nRanks + lane;
        long long polls = 0;
        const bool dead = *W.status != 0;
        while (!dead && __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != e) {
            if (++polls > W.maxPolls) { *W.status = 1; break; }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    const double* src = W.myWin + (size_t)par * (size_t)W.nG;
    const double* r = inv + (size_t)row * nCols;
    double acc = 0.0;
    for (int j = lane; j < nCols; j += 64) acc = fma(r[j], __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), acc);
    acc = wave_sum(acc);
    if (lane == 0) out[row] = acc;
}
// set-up self-test: the gathered vector as this rank sees it (one workgroup)
__global__ __launch_bounds__(256) void k_coarsest_gather_read(const GatherDev W, double* __restrict__ out)
{
    const unsigned long long e = *W.epoch;
    const int par = (int)(e & 1ull);
    if ((int)threadIdx.x < W.nRanks) {
        const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(W.myWin + 2 * (size_t)W.nG) + (size_t)par * W.nRanks + threadIdx.x;
        long long polls = 0;
        while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != e) {
            if (++polls > W.maxPolls) { *W.status = 1; break; }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    for (int64_t j = threadIdx.x; j < W.nG; j += blockDim.x) out[j] = __hip_atomic_load(W.myWin + (size_t)par * (size_t)W.nG + (size_t)j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_take_rows(const double* __restrict__ Inv, int64_t nG, int64_t off, const int32_t* __restrict__ e2c, int n, double* __restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)n * (size_t)nG; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / (size_t)nG); const int64_t j = (int64_t)(e % (size_t)nG);
        out[e] = Inv[(size_t)(off + e2c[i]) * nG + (size_t)j];   // this rank's rows, engine order
    }
}

} // namespace mi

struct GamgLevelDev {
    mi_addr_s* addr = nullptr;   // coarse level objects
    mi_matrix_s* mat = nullptr;
    int32_t nFine = 0, nCoarse = 0, nFineFaces = 0, nCoarseFaces = 0;
    DevBuf<int32_t> rStartE, rChildE, prolongE;                 // engine-order transfer maps
    DevBuf<int32_t> faceChildStart, faceChild, diagChildStart, diagChild, cellChildStart, cellChild;
    DevBuf<uint8_t> flip;
    DevBuf<double> cDiag, cUp, cLow;                            // coarse coefficients, caller order of the coarse level
    DevBuf<double> corr, src, tmp, tmp2;
    DevBuf<int32_t> slotChildStart, iStartE, iChildSlot;        // direct agglomeration (k_gamg_agg_slots / k_gamg_agg_diag_e): children by fine SLOT
    DevBuf<uint32_t> slotChild;
    bool direct = false;
    DevBuf<int32_t> ifChildStart, ifChild;                      // fine coupled-patch faces of every coarse one (ext numbering)
    DevBuf<double> ifUp;                                        // coarse interface slot values in patch order (coarsest assembly)
    int32_t nExt = 0;
    ~GamgLevelDev() { delete mat; delete addr; }
};

// gather window of the coarsest level (k_coarsest_gather_push / k_dense_matvec_win)
struct GamgGatherWin {
    void* window = nullptr; bool fineGrained = false, ready = false;
    Table<void*> mapped;
    double** peerTable = nullptr; unsigned long long* epoch = nullptr; int32_t* status = nullptr;
    int nRanks = 0, myRank = 0; int64_t nG = 0;
    ~GamgGatherWin()
    {
        for (size_t r = 0; r < mapped.size(); ++r) if (mapped[r] && (int)r != myRank) (void)hipIpcCloseMemHandle(mapped[r]);
        if (window) (void)hipFree(window);
        if (peerTable) (void)hipFree(peerTable);
        if (epoch) (void)hipFree(epoch);
        if (status) (void)hipFree(status);
    }
    GatherDev dev(long long maxPolls) const { return GatherDev{peerTable, static_cast<const double*>(window), epoch, status, nRanks, myRank, nG, maxPolls}; }
};

struct mi_gamg_s {
    mi_addr_s* fine = nullptr;
    GamgGatherWin* gather = nullptr;
    Table<GamgLevelDev*> lev;
    DevBuf<double> inv, gsrc, gA, gInv, fineScratch, foldScal;   // foldScal: {num, den} of every level's correction scaling (fused cycle)
    DevBuf<unsigned int> foldCounter;                          // arrival counter of the folding workgroup (tile_kernel_fx)
    DevBuf<int32_t> cIfRow, invStatus; DevBuf<int64_t> cIfCol;   // coarsest-level coupled faces: local row, global column
    bool invPending = false;
    bool invOnSide = false;   // the inversion of the coarsest matrix is still running on the context's side stream (gamg_wait_inverse)
    const mi_matrix_s* aggMatrix = nullptr; uint64_t aggEpoch = 0; // level matrices are those of this matrix at this epoch
    Table<int32_t> coarsestE2C;
    bool forwardOut = true;
    // decomposed case (processorGAMGInterface): communicators and, for the coarsest level, the block of every rank
    mi_comm_s *reduce = nullptr, *halo = nullptr;
    Table<int32_t> patchRank, patchNbrPatch;
    Table<GamgPatchHost> coarsestPatches;   // coarse cells on both sides of the coarsest level's coupled faces
    Table<int64_t> rankOffset;              // [nRanks+1] start of every rank's block in the global coarsest system
    int64_t nGlobalCoarsest = 0;
    // one V-cycle (incl. the finest residual and its copy to the host) as a hipGraph: ~135 launches, most of them a few
    // microseconds of work on coarse levels, replayed per cycle instead of enqueued one by one
    hipGraphExec_t aggGraph = nullptr;   // the level-matrix agglomeration of (aggGraphMatrix, aggGraphAsym) as a graph (gamg_agglomerate)
    const mi_matrix_s *aggGraphMatrix = nullptr, *aggSeenMatrix = nullptr; bool aggGraphAsym = false, aggSeenAsym = false; const void* aggBufs[3] = {nullptr, nullptr, nullptr};
    hipGraphExec_t cycleGraph = nullptr;
    struct CycleKey { const void *m = nullptr, *psi = nullptr, *src = nullptr; mi_gamg_controls ctl; bool doScale = false, asym = false; } cycleKey; // asym: the tile-kernel instantiations (and lowE) a cycle captured
    ~mi_gamg_s() { for (auto* l : lev) delete l; if (cycleGraph) (void)hipGraphExecDestroy(cycleGraph); if (aggGraph) (void)hipGraphExecDestroy(aggGraph); delete gather; }
};

namespace {
struct GamgBuildComm {
    mi_ctx_s* ctx; mi_comm_s *reduce, *halo;
    const mi_addr_s* fine; const int32_t *patchRank, *patchNbrPatch;
    std::string err;
};
// continueAgglomerating on all processors (GAMGAgglomeration.C:72-81)
bool gamg_all_and(void* user, bool v)
{
    GamgBuildComm* B = static_cast<GamgBuildComm*>(user);
    if (!B->reduce) return v;
    mi_ctx_s* c = B->ctx;
    double h = v ? 1.0 : 0.0;
    if (hipMemcpyAsync(c->scalars.p + 8, &h, sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) { B->err = "copy failed"; return false; }
    if (comm_allreduce_raw(B->reduce, c->stream, c->scalars.p + 8, 1) != MI_OK) { B->err = g_err; return false; }
    if (hipMemcpyAsync(&h, c->scalars.p + 8, sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { B->err = "copy failed"; return false; }
    return h > (double)B->reduce->nRanks - 0.5;
}
// the neighbour's restrict addressing of the patch-internal cells (GAMGAgglomerateLduAddressing.C:464-520); the ids travel
// as doubles (exact below 2^53) through the same grouped send/recv the halo uses
bool gamg_nbr_restrict(void* user, int, const Table<Table<int32_t>>& send, Table<Table<int32_t>>& recv)
{
    GamgBuildComm* B = static_cast<GamgBuildComm*>(user);
    if (!B->halo) { B->err = "processor patches need communicators (mi_gamg_create_coupled)"; return false; }
    mi_ctx_s* c = B->ctx;
    Table<mi_dpcg_comm_s::P2P> sends, recvs;
    Table<double> hs;
    int32_t off = 0;
    for (size_t p = 0; p < send.size(); ++p) {
        if (B->fine->patchIsLocal[p] || send[p].empty()) continue;
        mi_dpcg_comm_s::P2P e{(int32_t)p, B->patchRank[p], B->patchNbrPatch ? B->patchNbrPatch[p] : (int32_t)p, off, (int32_t)send[p].size()};
        sends.push_back(e); recvs.push_back(e);
        for (int32_t v : send[p]) hs.push_back((double)v);
        off += (int32_t)send[p].size();
    }
    std::stable_sort(recvs.begin(), recvs.end(), [](const mi_dpcg_comm_s::P2P& x, const mi_dpcg_comm_s::P2P& y) {
        return x.peer != y.peer ? x.peer < y.peer : x.nbrPatch < y.nbrPatch; });
    DevBuf<double> ds, dr;
    if (ds.alloc((size_t)std::max(off, 1)) != MI_OK || dr.alloc((size_t)std::max(off, 1)) != MI_OK) { B->err = "allocation failed"; return false; }
    Table<double> hr((size_t)off);
    if (off > 0) {
        if (hipMemcpyAsync(ds.p, hs.data(), sizeof(double) * (size_t)off, hipMemcpyHostToDevice, c->stream) != hipSuccess) { B->err = "copy failed"; return false; }
        if (comm_p2p_raw(B->halo, c->stream, sends, recvs, ds.p, dr.p) != MI_OK) { B->err = g_err; return false; }
        if (hipMemcpyAsync(hr.data(), dr.p, sizeof(double) * (size_t)off, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { B->err = "copy failed"; return false; }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { B->err = "exchange failed"; return false; }
    recv.assign(send.size(), Table<int32_t>());
    for (const auto& e : sends) {
        recv[(size_t)e.patch].resize((size_t)e.size);
        for (int32_t i = 0; i < e.size; ++i) recv[(size_t)e.patch][(size_t)i] = (int32_t)hr[(size_t)e.offset + (size_t)i];
    }
    return true;
}
} // namespace

extern "C" int mi_gamg_create_coupled(mi_addr_t fine, const double* face_weights_host, int32_t n_cells_in_coarsest_level,
                                      int32_t merge_levels, int forward_init, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                                      const int32_t* patch_nbr_patch, mi_gamg_t* out);

namespace {
// gather window of the coarsest level: allocate, all-gather the IPC handles over the communicator's base transport, map every
// rank's window, test gathers of known values, agreement.  Any rank that cannot -> nobody uses it (the all-reduce stays).
int gamg_gather_setup(mi_gamg_s* g, mi_comm_s* reduce)
{
    mi_ctx_s* c = g->fine->ctx;
    hipStream_t s = c->stream;
    const int nRanks = reduce->nRanks, rank = reduce->rank;
    const int64_t nG = g->nGlobalCoarsest;
    GamgGatherWin* W = new GamgGatherWin();
    struct Guard { GamgGatherWin* w; bool keep = false; ~Guard() { if (!keep) delete w; } } guard{W};
    W->nRanks = nRanks; W->myRank = rank; W->nG = nG;
    unsigned char mine[sizeof(hipIpcMemHandle_t)] = {0};
    const size_t bytes = sizeof(double) * 2 * (size_t)std::max<int64_t>(nG, 1) + sizeof(unsigned long long) * 2 * (size_t)nRanks;
    bool ok = alloc_ipc_window(bytes, &W->window, &W->fineGrained) == MI_OK, all = false;
    hipIpcMemHandle_t h;
    if (ok) ok = hipIpcGetMemHandle(&h, W->window) == hipSuccess;
    if (ok) memcpy(mine, &h, sizeof(h));
    if (ok) ok = hipMalloc(reinterpret_cast<void**>(&W->epoch), sizeof(unsigned long long)) == hipSuccess && hipMemset(W->epoch, 0, sizeof(unsigned long long)) == hipSuccess &&
                 hipMalloc(reinterpret_cast<void**>(&W->status), sizeof(int32_t)) == hipSuccess && hipMemset(W->status, 0, sizeof(int32_t)) == hipSuccess &&
                 hipMalloc(reinterpret_cast<void**>(&W->peerTable), sizeof(double*) * (size_t)nRanks) == hipSuccess;
    (void)hipGetLastError();
    MICHK(comm_agree(reduce, ok, &all));
    if (!all) return MI_OK;
    Table<unsigned char> handles;
    MICHK(comm_gather_bytes(reduce, mine, sizeof(mine), handles));
    W->mapped.assign((size_t)nRanks, nullptr);
    bool oneDevice = true;
    for (int r = 0; r < nRanks && ok; ++r) {
        if (r == rank) { W->mapped[(size_t)r] = W->window; continue; }
        hipIpcMemHandle_t hr;
        memcpy(&hr, handles.data() + (size_t)r * sizeof(hr), sizeof(hr));
        void* q = nullptr;
        if (hipIpcOpenMemHandle(&q, hr, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
        W->mapped[(size_t)r] = q;
        if (!on_my_device(c, q)) oneDevice = false;
    }
    if (ok && !W->fineGrained && !oneDevice && !env_int("MI_PEER_ALLOW_COARSE", 0)) ok = false;
    if (ok) ok = hipMemcpy(W->peerTable, W->mapped.data(), sizeof(double*) * (size_t)nRanks, hipMemcpyHostToDevice) == hipSuccess;
    MICHK(comm_agree(reduce, ok, &all));        // also: every window is mapped before anyone writes into it
    if (!all) return MI_OK;
    // test gathers: rank r contributes (r + 1)(round + 1) + i/4 for its coarsest cell i; every rank must read the WHOLE vector back
    GamgLevelDev* Lc = g->lev.back();
    const int n = Lc->nCoarse;
    const int64_t off = g->rankOffset[(size_t)rank];
    DevBuf<double> dv, probe;
    MICHK(probe.alloc((size_t)std::max<int64_t>(nG, 1)));
    ok = true;
    for (int round = 0; round < 3; ++round) {      // (every rank runs every round, also one without coarsest cells: its peers wait for its flag)
        Table<double> hv((size_t)std::max(n, 1), 0.0);
        for (int i = 0; i < n; ++i) hv[(size_t)i] = (double)((rank + 1) * (round + 1)) + 0.25 * (double)g->coarsestE2C[(size_t)i];
        MICHK(dv.upload(hv, s));
        k_coarsest_gather_push<<<1, 256, 0, s>>>(dv.p, Lc->addr->e2c.p, n, off, W->dev(4000000ll));
        k_coarsest_gather_read<<<1, 256, 0, s>>>(W->dev(4000000ll), probe.p);
        HIPCHK(hipGetLastError());
        Table<double> back((size_t)std::max<int64_t>(nG, 1));
        int32_t st = 0;
        HIPCHK(hipMemcpyAsync(back.data(), probe.p, sizeof(double) * (size_t)nG, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&st, W->status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int r = 0; r < nRanks; ++r)
            for (int64_t j = g->rankOffset[(size_t)r]; j < g->rankOffset[(size_t)r + 1]; ++j)
                if (back[(size_t)j] != (double)((r + 1) * (round + 1)) + 0.25 * (double)(j - g->rankOffset[(size_t)r])) ok = false;
        if (st != 0) { ok = false; HIPCHK(hipMemset(W->status, 0, sizeof(int32_t))); }
        bool allRound = false;
        MICHK(comm_agree(reduce, true, &allRound));   // (a barrier: nobody starts round k + 2 into a parity a slow rank still reads)
    }
    MICHK(comm_agree(reduce, ok, &all));
    if (!all) return MI_OK;
    W->ready = true;
    g->gather = W; guard.keep = true;
    return MI_OK;
}
} // namespace

// [start-up begin] -- hierarchy creation: host code that runs once per mesh.  tools/source_fingerprint.py leaves the text between
// these markers out of the hash the committed V-cycle traffic figure is tied to (what it builds is covered by the OUTPUT
// fingerprints of the layout and the hierarchy; the kernels and the cycle code outside the markers by their text).
namespace {
// The host tables of one level that depend on the tile layouts of BOTH its sides (engine-order transfer maps, coupled-patch
// children in the ext numbering, and -- direct agglomeration -- the slot-to-slot children lists).  Built by the level's own
// start-up thread right after its layout (round 4: they used to queue on the calling thread behind the whole matching).
struct LevelMaps {
    Table<int32_t> rStart, rChild, pmap, ifStart, ifChild, sStart, iStart, iChild;
    Table<uint32_t> sChild;
    bool direct = false;
};
// fineLay: layout of the level's fine side (e2c / c2e / patchOffset); fineFaceSlot: its faceSlot table or nullptr (no direct tables);
// lay: layout of the coarse side (e2c / c2e, slotFace for the direct tables); L: the level with its children lists (finish_gamg_level)
void build_level_maps(const GamgLevelHost& L, const TileLayout& fineLay, const Table<int32_t>* fineFaceSlot, const TileLayout& lay, int32_t nPatches, LevelMaps& M)
{
    const Table<int32_t>& fe2c = fineLay.e2c; const Table<int32_t>& fc2e = fineLay.c2e;
    const Table<int32_t>& ce2c = lay.e2c;     const Table<int32_t>& cc2e = lay.c2e;
    M.rStart.assign((size_t)L.nCoarse + 1, 0); M.rChild.resize((size_t)L.nFine); M.pmap.resize((size_t)L.nFine);
    parallel_for(L.nCoarse, 1 << 16, [&](int64_t ce) { const int32_t cc = ce2c[(size_t)ce]; M.rStart[(size_t)ce + 1] = L.cellChildStart[(size_t)cc + 1] - L.cellChildStart[(size_t)cc]; });
    parallel_inclusive_scan(M.rStart.data() + 1, (int64_t)L.nCoarse);
    parallel_for(L.nCoarse, 1 << 16, [&](int64_t ce) {
        const int32_t cc = ce2c[(size_t)ce];
        for (int32_t k = L.cellChildStart[(size_t)cc], o = M.rStart[(size_t)ce]; k < L.cellChildStart[(size_t)cc + 1]; ++k, ++o) M.rChild[(size_t)o] = fc2e[(size_t)L.cellChild[(size_t)k]];
    });
    parallel_for(L.nFine, 1 << 16, [&](int64_t fe) { M.pmap[(size_t)fe] = cc2e[(size_t)L.restrictMap[(size_t)fe2c[(size_t)fe]]]; });
    // coupled-patch children in the ext numbering of both levels (patch offset + face)
    M.ifStart.assign(1, 0); M.ifChild.clear();
    for (int32_t p = 0; p < nPatches; ++p) {
        const GamgPatchHost& P = L.patches[(size_t)p];
        const int32_t fOff = fineLay.patchOffset[(size_t)p];
        for (size_t k = 0; k + 1 < P.childStart.size(); ++k) {
            for (int32_t j = P.childStart[k]; j < P.childStart[k + 1]; ++j) M.ifChild.push_back(fOff + P.child[(size_t)j]);
            M.ifStart.push_back((int32_t)M.ifChild.size());
        }
    }
    M.direct = fineFaceSlot != nullptr;
    if (!M.direct) return;
    const Table<int32_t>& sf = lay.slotFace;
    const Table<int32_t>& ffs = *fineFaceSlot;
    const int64_t nS = (int64_t)sf.size();
    M.sStart.assign((size_t)nS + 1, 0);
    parallel_for(nS, 1 << 16, [&](int64_t k) { const int32_t f = sf[(size_t)k]; M.sStart[(size_t)k + 1] = f >= 0 ? L.faceChildStart[(size_t)f + 1] - L.faceChildStart[(size_t)f] : 0; });
    parallel_inclusive_scan(M.sStart.data() + 1, nS);
    M.sChild.resize((size_t)M.sStart[(size_t)nS]);
    parallel_blocks(nS, 1 << 16, [&](int64_t b, int64_t e, int) {
        for (int64_t k = b; k < e; ++k) {
            const int32_t f = sf[(size_t)k];
            if (f < 0) continue;
            int32_t o = M.sStart[(size_t)k];
            for (int32_t j = L.faceChildStart[(size_t)f]; j < L.faceChildStart[(size_t)f + 1]; ++j, ++o) {
                const int32_t ff = L.faceChild[(size_t)j];
                M.sChild[(size_t)o] = (uint32_t)ffs[(size_t)ff] | (L.faceFlip[(size_t)ff] ? 0x80000000u : 0u);
            }
        }
    });
    M.iStart.assign((size_t)L.nCoarse + 1, 0);
    parallel_for(L.nCoarse, 1 << 16, [&](int64_t ce) { const int32_t cc = ce2c[(size_t)ce]; M.iStart[(size_t)ce + 1] = L.diagChildStart[(size_t)cc + 1] - L.diagChildStart[(size_t)cc]; });
    parallel_inclusive_scan(M.iStart.data() + 1, (int64_t)L.nCoarse);
    M.iChild.resize((size_t)M.iStart[(size_t)L.nCoarse]);
    parallel_blocks(L.nCoarse, 1 << 16, [&](int64_t b, int64_t e, int) {
        for (int64_t ce = b; ce < e; ++ce) {
            const int32_t cc = ce2c[(size_t)ce];
            int32_t o = M.iStart[(size_t)ce];
            for (int32_t j = L.diagChildStart[(size_t)cc]; j < L.diagChildStart[(size_t)cc + 1]; ++j, ++o) M.iChild[(size_t)o] = ffs[(size_t)L.diagChild[(size_t)j]];
        }
    });
    if (M.sChild.empty()) M.sChild.push_back(0u);
    if (M.iChild.empty()) M.iChild.push_back(0);
}
} // namespace

extern "C" int mi_gamg_create(mi_addr_t fine, const double* face_weights_host, int32_t n_cells_in_coarsest_level,
                              int32_t merge_levels, int forward_init, mi_gamg_t* out)
{
    return mi_gamg_create_coupled(fine, face_weights_host, n_cells_in_coarsest_level, merge_levels, forward_init, nullptr, nullptr, nullptr, nullptr, out);
}

static int gamg_create_impl(mi_addr_t fine, const double* face_weights_host, int32_t n_cells_in_coarsest_level,
                            int32_t merge_levels, int forward_init, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                            const int32_t* patch_nbr_patch, int32_t dummy_levels, mi_gamg_t* out);
extern "C" int mi_gamg_create_coupled(mi_addr_t fine, const double* face_weights_host, int32_t n_cells_in_coarsest_level,
                                      int32_t merge_levels, int forward_init, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                                      const int32_t* patch_nbr_patch, mi_gamg_t* out)
{
    if (!face_weights_host) return fail(MI_ERR_ARG, "mi_gamg_create: bad argument");
    return gamg_create_impl(fine, face_weights_host, n_cells_in_coarsest_level, merge_levels, forward_init, reduce, halo, patch_rank, patch_nbr_patch, 0, out);
}
// dummyAgglomeration (GAMGAgglomerations/dummyAgglomeration/dummyAgglomeration.C:45-90): n_levels levels with identity restrict
// addressing -- the reference's debugging agglomerator ("agglomerator dummy; nLevels n;")
extern "C" int mi_gamg_create_dummy(mi_addr_t fine, int32_t n_levels, mi_gamg_t* out)
{
    if (n_levels < 1 || n_levels > 48) return fail(MI_ERR_ARG, "mi_gamg_create_dummy: nLevels out of range");
    if (fine && fine->L.nPatches > fine->nLocalPatches) return fail(MI_ERR_UNSUPPORTED, "mi_gamg_create_dummy: processor patches are not handled by the dummy agglomeration here");
    return gamg_create_impl(fine, nullptr, 1, 1, 1, nullptr, nullptr, nullptr, nullptr, n_levels, out);
}
static int gamg_create_impl(mi_addr_t fine, const double* face_weights_host, int32_t n_cells_in_coarsest_level,
                            int32_t merge_levels, int forward_init, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                            const int32_t* patch_nbr_patch, int32_t dummy_levels, mi_gamg_t* out)
{
    if (!fine || !out || n_cells_in_coarsest_level < 1 || merge_levels < 1) return fail(MI_ERR_ARG, "mi_gamg_create: bad argument");
    if ((reduce == nullptr) != (halo == nullptr)) return fail(MI_ERR_ARG, "mi_gamg_create_coupled: give both communicators or none");
    mi_ctx_s* c = fine->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int32_t nPatches = fine->L.nPatches;
    const bool remote = nPatches > fine->nLocalPatches;
    if (remote && (!reduce || !patch_rank)) return fail(MI_ERR_ARG, "mi_gamg_create: processor patches need communicators and patch_rank (mi_gamg_create_coupled)");
    GamgHierarchyHost H;
    GamgCoupling cpl;
    GamgBuildComm bc{c, reduce, halo, fine, patch_rank, patch_nbr_patch, std::string()};
    cpl.nPatches = nPatches;
    cpl.faceCells = fine->patchFaceCellsHost; cpl.nbrCells = fine->patchNbrCellsHost; cpl.isLocal = fine->patchIsLocal;
    cpl.allAnd = gamg_all_and; cpl.nbrRestrict = gamg_nbr_restrict; cpl.user = &bc;
    cpl.ami.resize((size_t)nPatches);
    for (const mi_addr_s::AmiPatch* q : fine->ami) {
        GamgCoupling::Ami& A = cpl.ami[(size_t)q->patch];
        A.nbrPatch = q->nbrPatch; A.start = q->hStart; A.addr = q->hAddr; A.w = q->hW; A.magSf = q->hMagSf;
        A.transport = q->transport; A.nPartner = q->nPartner; A.transports = q->transports; A.partCount = q->partCount;
    }
    // Start-up pipeline (round 3): the pair matching of level l+1 is sequential host code (the reference's visiting order decides
    // the maps); as soon as level l's coarse addressing is final, ANOTHER thread builds that level's tile layout and children
    // lists, so the levels' layouts no longer queue behind the whole matching (10 M cells: hierarchy + layouts 2.1 -> ~1.3 s).
    // Round 4: the same thread goes on with the level's transfer maps and slot-to-slot children lists (build_level_maps) as soon
    // as the layout of the level's FINE side -- the previous level's task, or the caller's addressing -- is there as well; the
    // calling thread is left with the uploads.
    struct LevelTask {
        std::thread th; TileLayout L; std::string err; Table<int32_t> psz; Table<const int32_t*> pfc, pnb;
        LevelMaps maps; bool haveMaps = false;
        std::mutex mu; std::condition_variable cv; bool layoutReady = false;   // (the next level's task waits for it)
    };
    const bool wantDirect = sw::get(SW_GAMG_DIRECT_SLOTS) != 0 && dummy_levels == 0;
    Table<int32_t> fineFaceSlot;   // direct agglomeration tables: the finest level's faceSlot comes back from the device once
    if (wantDirect && fine->L.nFaces > 0) {
        fineFaceSlot.resize((size_t)fine->L.nFaces);
        HIPCHK(hipMemcpy(fineFaceSlot.data(), fine->faceSlot.p, sizeof(int32_t) * fineFaceSlot.size(), hipMemcpyDeviceToHost));
    }
    Table<std::unique_ptr<LevelTask>> tasks;
    struct Joiner { Table<std::unique_ptr<LevelTask>>& t; ~Joiner() { for (auto& k : t) if (k && k->th.joinable()) k->th.join(); } } joiner{tasks};
    const bool pipeline = sw::get(SW_GAMG_PIPELINE) != 0 && merge_levels == 1;
    if (pipeline) H.onLevel = [&](int l) {
        GamgLevelHost& Lh = H.levels[(size_t)l];
        tasks.emplace_back(new LevelTask());
        LevelTask* T = tasks.back().get();
        T->psz.resize((size_t)nPatches); T->pfc.resize((size_t)nPatches); T->pnb.resize((size_t)nPatches);
        for (int32_t p = 0; p < nPatches; ++p) {
            T->psz[p] = (int32_t)Lh.patches[p].faceCells.size();
            T->pfc[p] = Lh.patches[p].faceCells.data();
            T->pnb[p] = fine->patchIsLocal[(size_t)p] == 1 ? Lh.patches[p].nbrCells.data() : nullptr;
        }
        const TileParams prm = addr_tile_params(c, Lh.nCoarse, true, false, 0, nullptr);
        LevelTask* prevT = tasks.size() >= 2 ? tasks[tasks.size() - 2].get() : nullptr;
        const bool direct = wantDirect && fine->L.nFaces > 0;
        // MI_GAMG_INHERIT_TILES=1 (opt-in at the end of round 4: validated on the host -- tests/test_host_build.py,
        // tools/exp/inherit_tiles.cpp -- but not yet on the device): the level takes its tiles from its fine side's tiles instead
        // of clustering again (csrc/tiling.hpp inherit_tiles); on the 216^3 box the first two level layouts come out table for
        // table the same, without the clustering's sequential matching that is the critical path of this function.
        const bool inherit = sw::get(SW_GAMG_INHERIT_TILES) != 0 && prm.tileCells == 1024;
        T->th = std::thread([T, prevT, &Lh, prm, nPatches, fine, direct, &fineFaceSlot, inherit] {
            TileParams lp = prm;
            Table<int32_t> inherited;
            if (inherit) {
                if (prevT) { std::unique_lock<std::mutex> lk(prevT->mu); prevT->cv.wait(lk, [prevT] { return prevT->layoutReady; }); }
                const TileLayout* fl = prevT ? (prevT->err.empty() ? &prevT->L : nullptr) : &fine->L;
                if (fl && fl->nTiles > 0 && (int32_t)fl->e2c.size() == Lh.nFine) {
                    Table<int32_t> tileOf((size_t)Lh.nFine);
                    parallel_for(fl->nTiles, 16, [&](int64_t t) { for (int32_t e = fl->tileCellStart[(size_t)t]; e < fl->tileCellStart[(size_t)t + 1]; ++e) tileOf[(size_t)fl->e2c[(size_t)e]] = (int32_t)t; });
                    int32_t nParts = 0;
                    if (inherit_tiles(Lh.nFine, Lh.restrictMap.data(), tileOf.data(), fl->nTiles, Lh.nCoarse, Lh.nCoarseFaces, Lh.cLower.data(), Lh.cUpper.data(),
                                      nPatches, T->psz.data(), T->pfc.data(), lp.tileCells, lp.slotCap, inherited, nParts).empty()) { lp.givenPart = inherited.data(); lp.nGivenParts = nParts; }
                }
            }
            T->err = build_tile_layout(Lh.nCoarse, Lh.nCoarseFaces, Lh.cLower.data(), Lh.cUpper.data(), nPatches, T->psz.data(), T->pfc.data(), lp, T->L, T->pnb.data());
            if (!T->err.empty() && lp.givenPart)   // the inherited tiles were refused (caps): cluster as before
                T->err = build_tile_layout(Lh.nCoarse, Lh.nCoarseFaces, Lh.cLower.data(), Lh.cUpper.data(), nPatches, T->psz.data(), T->pfc.data(), prm, T->L, T->pnb.data());
            { std::lock_guard<std::mutex> lk(T->mu); T->layoutReady = true; }
            T->cv.notify_all();
            finish_gamg_level(Lh);
            if (!T->err.empty()) return;
            if (prevT) { std::unique_lock<std::mutex> lk(prevT->mu); prevT->cv.wait(lk, [prevT] { return prevT->layoutReady; }); if (!prevT->err.empty()) return; }
            const TileLayout& fineLay = prevT ? prevT->L : fine->L;
            build_level_maps(Lh, fineLay, direct ? (prevT ? &prevT->L.faceSlot : &fineFaceSlot) : nullptr, T->L, nPatches, T->maps);
            T->haveMaps = true;
        });
    };
#ifdef MI_TIMING
    auto tg0__ = std::chrono::steady_clock::now();
#endif
    const std::string err = build_gamg_hierarchy(fine->L.nCells, fine->L.nFaces, fine->lowerHost.data(), fine->upperHost.data(),
                                                 face_weights_host, n_cells_in_coarsest_level, forward_init != 0, H,
                                                 (nPatches > 0 || reduce) ? &cpl : nullptr, merge_levels, dummy_levels);
#ifdef MI_TIMING
    fprintf(stderr, "[gamg] build_gamg_hierarchy (pair agglomeration + coarse addressing, host) %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tg0__).count());
    tg0__ = std::chrono::steady_clock::now();
#endif
    if (!err.empty()) return fail(MI_ERR_ARG, "mi_gamg_create: " + err + (bc.err.empty() ? "" : " (" + bc.err + ")"));
    if (H.levels.empty())
        return fail(MI_ERR_STATE, "No coarse levels created, either matrix too small for GAMG or nCellsInCoarsestLevel too large"); // GAMGSolver.C:175-190
    mi_gamg_s* g = new mi_gamg_s();
    g->fine = fine; g->forwardOut = H.forwardOut;
    g->reduce = reduce; g->halo = halo;
    if (patch_rank) g->patchRank.assign(patch_rank, patch_rank + nPatches);
    if (patch_nbr_patch) g->patchNbrPatch.assign(patch_nbr_patch, patch_nbr_patch + nPatches);
    hipStream_t s = c->stream;
    const mi_addr_s* prev = fine;
    // direct agglomeration tables (round 4): coarse slot -> fine slots, coarse engine cell -> fine slots of its interior faces.
    // They need the host copies of faceSlot (fine side) and slotFace (coarse side): the finest level's comes back from the
    // device once, the levels' are kept until used (mi_ctx_s::keepSlotTables).
    Table<int32_t> prevFaceSlot;   // (levels built on this thread: the fine side's faceSlot travels from level to level)
    if (tasks.empty()) prevFaceSlot.swap(fineFaceSlot);
    struct KeepTables { mi_ctx_s* c; explicit KeepTables(mi_ctx_s* cc, bool on) : c(cc) { c->keepSlotTables = on; } ~KeepTables() { c->keepSlotTables = false; } } keepTables(c, wantDirect && tasks.empty());
#ifdef MI_TIMING
    auto tl__ = std::chrono::steady_clock::now();
#define MI_TL(what, l) do { if ((l) < 64) { auto n__ = std::chrono::steady_clock::now(); fprintf(stderr, "[gamg]   level %d %-34s %.4f s\n", (int)(l), what, std::chrono::duration<double>(n__ - tl__).count()); tl__ = n__; } } while (0)
#else
#define MI_TL(what, l) do {} while (0)
#endif
    // Levels with a start-up task are taken COARSEST FIRST: the small levels' uploads run while the threads of the two largest
    // levels are still at work, and a level's layout is moved into its addressing only after the task of the next coarser level
    // -- the one that reads it as its fine side -- has been joined.
    g->lev.assign(H.levels.size(), nullptr);
    for (size_t step = 0; step < H.levels.size(); ++step) {
        const size_t l = tasks.empty() ? step : H.levels.size() - 1 - step;
        GamgLevelHost& L = H.levels[l];
        GamgLevelDev* D = new GamgLevelDev();
        g->lev[l] = D;
        MI_TL("(previous level's tail)", l);
        D->nFine = L.nFine; D->nCoarse = L.nCoarse; D->nFineFaces = L.nFineFaces; D->nCoarseFaces = L.nCoarseFaces;
        mi_addr_t ca = nullptr;
        Table<int32_t> psz((size_t)nPatches);
        Table<const int32_t*> pfc((size_t)nPatches), pnb((size_t)nPatches);
        for (int32_t p = 0; p < nPatches; ++p) {
            psz[p] = (int32_t)L.patches[p].faceCells.size();
            pfc[p] = L.patches[p].faceCells.data();
            pnb[p] = fine->patchIsLocal[(size_t)p] == 1 ? L.patches[p].nbrCells.data() : nullptr; // cyclicAMI: ext region + the agglomerated AMI below
        }
        int r;
        if (l < tasks.size()) { // the layout was built while the deeper levels were matched
            LevelTask* T = tasks[l].get();
            if (T->th.joinable()) T->th.join();
            MI_TL("wait for the layout task", l);
            if (T->err.empty() && !T->haveMaps) {   // its fine side's layout failed: report that one
                for (auto& k : tasks) { if (k->th.joinable()) k->th.join(); if (!k->err.empty()) { T->err = k->err; break; } }
                if (T->err.empty()) T->err = "level tables were not built";
            }
            if (!T->err.empty()) { delete g; return fail(MI_ERR_LIMIT, "mi_gamg_create: " + T->err); }
            r = addr_create_impl(c, L.nCoarse, L.nCoarseFaces, L.cLower.data(), L.cUpper.data(), nPatches, psz.data(), pfc.data(), pnb.data(), true, false, 0, nullptr, &ca, &T->L);
        } else r = addr_create_impl(c, L.nCoarse, L.nCoarseFaces, L.cLower.data(), L.cUpper.data(), nPatches, psz.data(), pfc.data(), pnb.data(), true, false, 0, nullptr, &ca, nullptr);
        if (r != MI_OK) { delete g; return r; }
        MI_TL("addressing on the device", l);
        for (const mi_addr_s::AmiPatch* q : fine->ami) {
            const GamgPatchHost& P = L.patches[(size_t)q->patch];
            if (q->transport >= 0) {   // partner on another rank: addresses as faces of this level's transport patch
                Table<int32_t> face(P.amiAddr.size()), slot(P.amiAddr.size());
                for (size_t k = 0; k < face.size(); ++k) { face[k] = P.amiSrcFace[(size_t)P.amiAddr[k]]; slot[k] = P.amiSrcSlot[(size_t)P.amiAddr[k]]; }
                r = ami_remote_impl(ca, q->patch, q->transports, P.amiPartCount, P.amiStart.data(), slot.data(), face.data(), P.amiAddr.data(), P.amiW.data(), nullptr);
            } else
            r = mi_addr_set_ami_patch(ca, q->patch, q->nbrPatch, P.amiStart.data(), P.amiAddr.data(), P.amiW.data(), nullptr); // no low-weight correction on coarse levels (AMIInterpolation.C:751)
            if (r != MI_OK) { mi_addr_destroy(ca); delete g; return r; }
        }
        D->addr = ca;
        D->nExt = ca->L.nExt;
        mi_matrix_t cm = nullptr;
        r = mi_matrix_create(ca, &cm);
        if (r != MI_OK) { delete g; return r; }
        D->mat = cm;
        if (reduce) {
            r = mi_matrix_attach_comm(cm, reduce, halo, patch_rank, patch_nbr_patch, 1);
            if (r != MI_OK) { delete g; return r; }
        }
        // transfer maps, coupled-patch children, slot-to-slot children lists: from the level's task, or built here
        LevelMaps localMaps;
        const bool fromTask = l < tasks.size() && tasks[l]->haveMaps;
        if (!fromTask) build_level_maps(L, prev->L, wantDirect ? &prevFaceSlot : nullptr, ca->L, nPatches, localMaps);
        LevelMaps& M = fromTask ? tasks[l]->maps : localMaps;
        MI_TL("transfer maps (host)", l);
        if ((int32_t)M.ifStart.size() - 1 != D->nExt) { delete g; return fail(MI_ERR_STATE, "GAMG: coupled-patch agglomeration is inconsistent"); }
#define UPG(buf, vec) if (r == MI_OK) r = D->buf.upload(vec, s)
        UPG(rStartE, M.rStart); UPG(rChildE, M.rChild); UPG(prolongE, M.pmap);
        UPG(faceChildStart, L.faceChildStart); UPG(faceChild, L.faceChild);
        UPG(diagChildStart, L.diagChildStart); UPG(diagChild, L.diagChild);
        UPG(cellChildStart, L.cellChildStart); UPG(cellChild, L.cellChild); UPG(flip, L.faceFlip);
        if (D->nExt > 0) { UPG(ifChildStart, M.ifStart); UPG(ifChild, M.ifChild); }
        MI_TL("uploads of the maps", l);
        if (M.direct) {
            UPG(slotChildStart, M.sStart); UPG(iStartE, M.iStart); UPG(iChildSlot, M.iChild);
            if (r == MI_OK) r = D->slotChild.upload(M.sChild, s);
            D->direct = true;
            if (!fromTask) {
                prevFaceSlot.swap(ca->L.faceSlot);                  // the next level's fine side
                Table<int32_t>().swap(ca->L.faceSlot);
                Table<int32_t>().swap(ca->L.slotFace);
            }
        }
        MI_TL("slot-to-slot children lists", l);
#undef UPG
        if (r == MI_OK) r = D->cDiag.alloc((size_t)L.nCoarse);
        if (r == MI_OK) r = D->cUp.alloc((size_t)L.nCoarseFaces);
        if (r == MI_OK) r = D->cLow.alloc((size_t)L.nCoarseFaces);
        if (r == MI_OK) r = D->corr.alloc((size_t)L.nCoarse + (size_t)D->nExt);
        if (r == MI_OK) r = D->src.alloc((size_t)L.nCoarse + (size_t)D->nExt);
        if (r == MI_OK) r = D->tmp.alloc((size_t)L.nCoarse + (size_t)D->nExt);
        if (r == MI_OK) r = D->tmp2.alloc((size_t)L.nCoarse + (size_t)D->nExt);
        if (r == MI_OK && D->nExt > 0) r = D->ifUp.alloc((size_t)D->nExt);
        if (r != MI_OK) { delete g; return r; }
        if (hipStreamSynchronize(s) != hipSuccess) { delete g; return fail(MI_ERR_DEVICE, "upload failed"); }
        MI_TL("allocations + synchronise", l);
        prev = ca;
    }
#ifdef MI_TIMING
    fprintf(stderr, "[gamg] level layouts + transfer maps + uploads %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tg0__).count());
#endif
    GamgLevelDev* last = g->lev.back();
    g->coarsestE2C = last->addr->L.e2c;
    g->coarsestPatches = H.levels.back().patches;
    // block of every rank in the global coarsest system (LUscalarMatrix.C:275-290 procOffsets_)
    const int nRanks = reduce ? reduce->nRanks : 1, rank = reduce ? reduce->rank : 0;
    g->rankOffset.assign((size_t)nRanks + 1, 0);
    {
        Table<double> sizes((size_t)nRanks, 0.0);
        sizes[(size_t)rank] = (double)last->nCoarse;
        if (reduce) {
            DevBuf<double> d;
            int r = d.alloc((size_t)nRanks);
            if (r != MI_OK) { delete g; return r; }
            if (hipMemcpyAsync(d.p, sizes.data(), sizeof(double) * (size_t)nRanks, hipMemcpyHostToDevice, s) != hipSuccess) { delete g; return fail(MI_ERR_DEVICE, "copy failed"); }
            r = comm_allreduce_raw(reduce, s, d.p, (size_t)nRanks);
            if (r != MI_OK) { delete g; return r; }
            if (hipMemcpyAsync(sizes.data(), d.p, sizeof(double) * (size_t)nRanks, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { delete g; return fail(MI_ERR_DEVICE, "copy failed"); }
        }
        for (int k = 0; k < nRanks; ++k) g->rankOffset[(size_t)k + 1] = g->rankOffset[k] + (int64_t)(sizes[k] + 0.5);
    }
    g->nGlobalCoarsest = g->rankOffset[(size_t)nRanks];
    if (g->nGlobalCoarsest > 4096) { delete g; return fail(MI_ERR_LIMIT, "coarsest level too large for the dense direct solve (nCellsInCoarsestLevel too big)"); }
    if (reduce && nRanks > 1 && reduce->peerReady && sw::get(SW_GAMG_GATHER_WIN)) {
        const int rg = gamg_gather_setup(g, reduce);   // collective; leaves g->gather == nullptr when any rank could not
        if (rg != MI_OK) { delete g; return rg; }
    }
    int r = g->inv.alloc((size_t)last->nCoarse * (size_t)g->nGlobalCoarsest);
    if (r == MI_OK) r = g->gsrc.alloc((size_t)g->nGlobalCoarsest);
    if (r == MI_OK) r = g->gA.alloc((size_t)g->nGlobalCoarsest * (size_t)g->nGlobalCoarsest);
    if (r != MI_OK) { delete g; return r; }
    *out = g;
    return MI_OK;
}

// [start-up end]
extern "C" int mi_gamg_destroy(mi_gamg_t g)
{
    if (g) {
        if (g->fine->ctx->sideStream) (void)hipStreamSynchronize(g->fine->ctx->sideStream);
        (void)hipStreamSynchronize(g->fine->ctx->stream);
        delete g;
    }
    return MI_OK;
}
extern "C" int32_t mi_gamg_n_levels(mi_gamg_t g) { return g ? (int32_t)g->lev.size() : 0; }
extern "C" int mi_gamg_forward_out(mi_gamg_t g) { return g && g->forwardOut ? 1 : 0; }
extern "C" int mi_gamg_level_sizes(mi_gamg_t g, int32_t level, int32_t out4[4])
{
    if (!g || level < 0 || level >= (int32_t)g->lev.size() || !out4) return fail(MI_ERR_ARG, "mi_gamg_level_sizes: bad argument");
    const GamgLevelDev* D = g->lev[(size_t)level];
    out4[0] = D->nFine; out4[1] = D->nFineFaces; out4[2] = D->nCoarse; out4[3] = D->nCoarseFaces;
    return MI_OK;
}

namespace {

int gamg_grid(int n) { int b = (n + 255) / 256; return b < 1 ? 1 : (b > 4096 ? 4096 : b); }

// level matrices from the fine matrix's current coefficients (GAMGSolver.C:88-97: every solver construction)
// the earlier host path (coefficients to the host, dense assembly, Gauss-Jordan there, rows back): kept behind
// MI_GAMG_HOST_INVERT=1 as a cross-check of the device inversion
int gamg_coarsest_host(mi_gamg_s* g, bool asym)
{
    mi_ctx_s* c = g->fine->ctx;
    hipStream_t s = c->stream;
    GamgLevelDev* Lc = g->lev.back();
    const int n = Lc->nCoarse, nf = Lc->nCoarseFaces, nx = Lc->nExt;
    const int64_t nG = g->nGlobalCoarsest;
    const int rank = g->reduce ? g->reduce->rank : 0;
    const int64_t off = g->rankOffset[(size_t)rank];
    Table<double> d((size_t)n), u((size_t)nf), lo((size_t)nf), ifc((size_t)nx);
    HIPCHK(hipMemcpyAsync(d.data(), Lc->cDiag.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (nf) HIPCHK(hipMemcpyAsync(u.data(), Lc->cUp.p, sizeof(double) * (size_t)nf, hipMemcpyDeviceToHost, s));
    if (nf && asym) HIPCHK(hipMemcpyAsync(lo.data(), Lc->cLow.p, sizeof(double) * (size_t)nf, hipMemcpyDeviceToHost, s));
    if (nx) HIPCHK(hipMemcpyAsync(ifc.data(), Lc->ifUp.p, sizeof(double) * (size_t)nx, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    Table<double> A((size_t)nG * (size_t)nG, 0.0);
    const Table<int32_t>& cl = Lc->addr->lowerHost; const Table<int32_t>& cu = Lc->addr->upperHost;
    for (int i = 0; i < n; ++i) A[(size_t)(off + i) * nG + (size_t)(off + i)] = d[i];
    for (int f = 0; f < nf; ++f) {
        A[(size_t)(off + cl[f]) * nG + (size_t)(off + cu[f])] = u[f];
        A[(size_t)(off + cu[f]) * nG + (size_t)(off + cl[f])] = asym ? lo[f] : u[f];
    }
    for (size_t p = 0; p < g->coarsestPatches.size(); ++p) { // row -= interfaceBouCoeffs: the slot value is already -coeff
        const GamgPatchHost& P = g->coarsestPatches[p];
        const int64_t nbrOff = g->fine->patchIsLocal[p] ? off : g->rankOffset[(size_t)g->patchRank[p]];
        const int32_t x0 = Lc->addr->L.patchOffset[p];
        for (size_t k = 0; k < P.faceCells.size(); ++k)
            A[(size_t)(off + P.faceCells[k]) * nG + (size_t)(nbrOff + P.nbrCells[k])] += ifc[(size_t)x0 + k];
    }
    if (g->reduce && g->reduce->nRanks > 1) {
        HIPCHK(hipMemcpyAsync(g->gA.p, A.data(), sizeof(double) * (size_t)nG * (size_t)nG, hipMemcpyHostToDevice, s));
        MICHK(comm_allreduce_raw(g->reduce, s, g->gA.p, (size_t)nG * (size_t)nG));
        HIPCHK(hipMemcpyAsync(A.data(), g->gA.p, sizeof(double) * (size_t)nG * (size_t)nG, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (!invert_dense((int)nG, A)) return fail(MI_ERR_STATE, "GAMG: coarsest-level matrix is singular");
    Table<double> Ae((size_t)n * (size_t)nG);
    const Table<int32_t>& e2c = g->coarsestE2C;
    for (int i = 0; i < n; ++i) for (int64_t j = 0; j < nG; ++j) Ae[(size_t)i * nG + (size_t)j] = A[(size_t)(off + e2c[i]) * nG + (size_t)j]; // this rank's rows, engine order
    HIPCHK(hipMemcpyAsync(g->inv.p, Ae.data(), sizeof(double) * (size_t)n * (size_t)nG, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return MI_OK;
}

// the engine's stream waits for the inversion that gamg_agglomerate put on the side stream (no-op otherwise)
int gamg_wait_inverse(mi_gamg_s* g)
{
    if (!g->invOnSide) return MI_OK;
    mi_ctx_s* c = g->fine->ctx;
    HIPCHK(hipStreamWaitEvent(c->stream, c->evSideDone, 0));
    g->invOnSide = false;
    return MI_OK;
}
// after a host synchronisation that follows gamg_agglomerate: was the coarsest matrix singular?
int gamg_check_inverse(mi_gamg_s* g)
{
    if (!g->invPending) return MI_OK;
    if (g->invOnSide) { MICHK(gamg_wait_inverse(g)); HIPCHK(hipStreamSynchronize(g->fine->ctx->stream)); }
    g->invPending = false;
    int32_t st = 0;
    HIPCHK(hipMemcpy(&st, g->invStatus.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (st != 0) {
        HIPCHK(hipMemset(g->invStatus.p, 0, sizeof(int32_t)));
        g->aggMatrix = nullptr;
        return fail(MI_ERR_STATE, "GAMG: coarsest-level matrix is singular");
    }
    return MI_OK;
}

int gamg_agglomerate(mi_gamg_s* g, mi_matrix_s* fineM, bool callerArrays = false)   // callerArrays: every level's cDiag / cUp / cLow as well (mi_gamg_level_coeffs)
{
    mi_ctx_s* c = g->fine->ctx;
    hipStream_t s = c->stream;
    const bool asym = fineM->asym;
    MICHK(gamg_wait_inverse(g));   // (an inversion nobody consumed yet still reads the global matrix this call is about to rewrite)
    const double *fDiag = fineM->diagE.p, *fUp = fineM->upE.p, *fLow = asym ? fineM->lowE.p : nullptr;
    const int32_t *dIdx = g->fine->c2e.p, *fIdx = g->fine->faceSlot.p; // level 0 reads the engine's slot / diag arrays
    const mi_matrix_s* fineMat = fineM; const mi_addr_s* fineAddr = g->fine;
    bool direct = !callerArrays;
    for (GamgLevelDev* D : g->lev) if (!D->direct) direct = false;
    if (direct) {
        // engine arrays to engine arrays (k_gamg_agg_slots / k_gamg_agg_diag_e); only the coarsest level's caller-order
        // arrays are formed as well (its dense system is assembled from them)
        // Round 6: the ~35 launches of this loop (two per level, most of them a few microseconds of work) cost ~13 us each when they are
        // enqueued one by one -- 0.3 ms of every pressure solve of a time step, whose coefficients are re-bound every step.  Their
        // arguments only depend on (matrix, symmetric or not): the SECOND agglomeration of the same matrix is captured into a hipGraph
        // and replayed from then on (the first one runs eagerly: it allocates the levels' lower arrays).
        const bool canGraph = c->gamgGraph != 0;
        // (the key holds the matrix AND its coefficient buffers: a matrix destroyed and another created at the same address must not replay stale pointers)
        const void* bufs[3] = {fineM->diagE.p, fineM->upE.p, asym ? fineM->lowE.p : nullptr};
        const bool sameBufs = g->aggBufs[0] == bufs[0] && g->aggBufs[1] == bufs[1] && g->aggBufs[2] == bufs[2];
        const bool replay = canGraph && g->aggGraph && g->aggGraphMatrix == fineM && g->aggGraphAsym == asym && sameBufs;
        const bool capture = canGraph && !replay && g->aggSeenMatrix == fineM && g->aggSeenAsym == asym && sameBufs;
        if (!replay && !capture && g->aggGraph) { (void)hipGraphExecDestroy(g->aggGraph); g->aggGraph = nullptr; }
        g->aggSeenMatrix = fineM; g->aggSeenAsym = asym; g->aggBufs[0] = bufs[0]; g->aggBufs[1] = bufs[1]; g->aggBufs[2] = bufs[2];
        if (capture) {
            if (g->aggGraph) { (void)hipGraphExecDestroy(g->aggGraph); g->aggGraph = nullptr; }
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        }
        const double* fD = fineM->diagE.p;
        for (size_t l = 0; l < g->lev.size(); ++l) {
            GamgLevelDev* D = g->lev[l];
            mi_matrix_s* cm = D->mat;
            mi_addr_s* ca = D->addr;
            if (asym && cm->lowE.n != (size_t)ca->L.totalSlots) {
                if (capture || replay) { if (capture) { hipGraph_t gr = nullptr; (void)hipStreamEndCapture(s, &gr); if (gr) (void)hipGraphDestroy(gr); } return fail(MI_ERR_STATE, "gamg_agglomerate: level storage changed under a captured agglomeration"); }
                MICHK(cm->lowE.alloc((size_t)ca->L.totalSlots));
            }
            cm->asym = asym;
            if (!replay) {
            k_gamg_agg_slots<<<gamg_grid((int)std::min<int64_t>(ca->L.totalSlots, 1 << 30)), 256, 0, s>>>(fUp, fLow, ca->slotFace.p, D->slotChildStart.p, D->slotChild.p,
                                                                                                       cm->upE.p, asym ? cm->lowE.p : nullptr, ca->L.totalSlots);
            k_gamg_agg_diag_e<<<gamg_grid(D->nCoarse), 256, 0, s>>>(fD, D->rStartE.p, D->rChildE.p, fUp, fLow, D->iStartE.p, D->iChildSlot.p, cm->diagE.p, D->nCoarse);
            if (D->nExt > 0)
                k_gamg_agg_iface<<<gamg_grid(D->nExt), 256, 0, s>>>(fineMat->upE.p, asym ? fineMat->lowE.p : nullptr, fineAddr->extSlot.p,
                                                                     D->ifChildStart.p, D->ifChild.p, ca->extSlot.p,
                                                                     cm->upE.p, asym ? cm->lowE.p : nullptr, D->ifUp.p, D->nExt);
            }
            cm->bound = true; cm->rDValid = false; cm->sumAValid = false; cm->epoch = next_epoch();
            cm->patchFactor = fineM->patchFactor;
            comm_inherit_factor_flag(cm, fineM);
            if (l + 1 == g->lev.size() && !replay) {   // coarsest: caller-order coefficients for the dense assembly (a few hundred cells)
                if (D->nCoarseFaces > 0)
                    k_gamg_agg_faces<<<gamg_grid(D->nCoarseFaces), 256, 0, s>>>(fUp, fLow, l == 0 ? g->fine->faceSlot.p : g->lev[l - 1]->addr->faceSlot.p, D->flip.p,
                                                                                 D->faceChildStart.p, D->faceChild.p, D->cUp.p, asym ? D->cLow.p : nullptr, D->nCoarseFaces);
                k_gamg_agg_diag<<<gamg_grid(D->nCoarse), 256, 0, s>>>(fD, l == 0 ? g->fine->c2e.p : g->lev[l - 1]->addr->c2e.p, D->cellChildStart.p, D->cellChild.p, fUp, fLow,
                                                                        l == 0 ? g->fine->faceSlot.p : g->lev[l - 1]->addr->faceSlot.p,
                                                                        D->diagChildStart.p, D->diagChild.p, D->cDiag.p, D->nCoarse);
            }
            fineMat = cm; fineAddr = ca;
            fD = cm->diagE.p; fUp = cm->upE.p; fLow = asym ? cm->lowE.p : nullptr;
        }
        if (capture) {
            hipGraph_t gr = nullptr;
            HIPCHK(hipStreamEndCapture(s, &gr));
            const hipError_t eI = hipGraphInstantiate(&g->aggGraph, gr, nullptr, nullptr, 0);
            (void)hipGraphDestroy(gr);
            HIPCHK(eI);
            g->aggGraphMatrix = fineM; g->aggGraphAsym = asym;
        }
        if (capture || replay) HIPCHK(hipGraphLaunch(g->aggGraph, s));
        HIPCHK(hipGetLastError());
    } else
    for (size_t l = 0; l < g->lev.size(); ++l) {
        GamgLevelDev* D = g->lev[l];
        if (D->nCoarseFaces > 0)
            k_gamg_agg_faces<<<gamg_grid(D->nCoarseFaces), 256, 0, s>>>(fUp, fLow, fIdx, D->flip.p, D->faceChildStart.p, D->faceChild.p,
                                                                         D->cUp.p, asym ? D->cLow.p : nullptr, D->nCoarseFaces);
        k_gamg_agg_diag<<<gamg_grid(D->nCoarse), 256, 0, s>>>(fDiag, dIdx, D->cellChildStart.p, D->cellChild.p, fUp, fLow, fIdx,
                                                                D->diagChildStart.p, D->diagChild.p, D->cDiag.p, D->nCoarse);
        HIPCHK(hipGetLastError());
        MICHK(mi_matrix_set_coeffs(D->mat, D->cDiag.p, D->cUp.p, asym ? D->cLow.p : nullptr));
        if (D->nExt > 0) { // interfaceLevelsBouCoeffs / IntCoeffs (GAMGSolverAgglomerateMatrix.C:74-216)
            k_gamg_agg_iface<<<gamg_grid(D->nExt), 256, 0, s>>>(fineMat->upE.p, asym ? fineMat->lowE.p : nullptr, fineAddr->extSlot.p,
                                                                 D->ifChildStart.p, D->ifChild.p, D->addr->extSlot.p,
                                                                 D->mat->upE.p, asym ? D->mat->lowE.p : nullptr, D->ifUp.p, D->nExt);
            HIPCHK(hipGetLastError());
        }
        D->mat->patchFactor = fineM->patchFactor; // doTransform_ / rank_ of a GAMG interface field are the fine interface's (cyclicGAMGInterfaceField.C:77-84)
        comm_inherit_factor_flag(D->mat, fineM);
        fineMat = D->mat; fineAddr = D->addr;
        fDiag = D->cDiag.p; fUp = D->cUp.p; fLow = asym ? D->cLow.p : nullptr; dIdx = nullptr; fIdx = nullptr;
    }
    // cyclicAMI: no dense coarsest system -- the reference's LUscalarMatrix casts every interface to a cyclic one
    // (LUscalarMatrix.C:246-251), so such a case runs with directSolveCoarsest off (ICCG / BICCG on the coarsest level)
    // (decomposed case: cyclicAMI patches on ANY rank -- agreed when the matrix was attached --, or the ranks without them would
    //  enter the all-reduce of the global coarsest matrix alone)
    if (!g->fine->ami.empty() || comm_any_ami(fineM)) return MI_OK;
    // dense inverse of the coarsest level.  Decomposed case: the GLOBAL coarsest system, like the reference's
    // LUscalarMatrix gathers every processor's coarsest matrix and interface coefficients (LUscalarMatrix.C:57-150,
    // convert :275-400); every rank assembles its block rows, one all-reduce replicates the matrix, every rank inverts it
    // (same code, same bits) and keeps the rows of its own cells.
    GamgLevelDev* Lc = g->lev.back();
    const int n = Lc->nCoarse, nf = Lc->nCoarseFaces, nx = Lc->nExt;
    const int64_t nG = g->nGlobalCoarsest;
    const int rank = g->reduce ? g->reduce->rank : 0;
    const int64_t off = g->rankOffset[(size_t)rank];
    // Measured on the 216^3 box (151 coarsest cells): host path 2.1 ms per re-agglomeration (two synchronisations + 1.3 ms of
    // Gauss-Jordan on one core), device path 3.9 ms (151 pivot steps of a single workgroup, ~25 us each: five dependent
    // L2 round trips per step).  The host cost grows with n^3 (17 ms at 300, 102 ms at 600 cells), the device cost with
    // n * max(1, n^2/1e5): the device path takes over above 256 global coarsest cells (decomposed cases with a large
    // nCellsInCoarsestLevel).  MI_GAMG_DEVICE_INVERT=0|1 forces one of them.
    // Round 3: up to 192 global coarsest cells the matrix is inverted in the REGISTERS of one workgroup (k_dense_invert_reg, same
    // bits as the host elimination) -- the default there; between 193 and 256 cells the host stays cheaper than the
    // global-memory kernel.
    const int wantDev = g->fine->ctx->gamgDeviceInvert;
    const bool regPath = nG <= 192 && env_int("MI_GAMG_REG_INVERT", 1) != 0;
    if (wantDev == 0 || (wantDev < 0 && !regPath && nG <= 256)) return gamg_coarsest_host(g, asym);
    mi_addr_s* ca = Lc->addr;
    if (ca->lowerAddr.n != (size_t)nf) { MICHK(ca->lowerAddr.upload(ca->lowerHost, s)); MICHK(ca->upperAddr.upload(ca->upperHost, s)); }
    if (g->cIfRow.n != (size_t)nx || g->invStatus.n == 0) {     // once per hierarchy
        Table<int32_t> row((size_t)nx, 0); Table<int64_t> colv((size_t)nx, 0);
        for (size_t p = 0; p < g->coarsestPatches.size(); ++p) {
            const GamgPatchHost& P = g->coarsestPatches[p];
            const int64_t nbrOff = g->fine->patchIsLocal[p] ? off : g->rankOffset[(size_t)g->patchRank[p]];
            const int32_t x0 = ca->L.patchOffset[p];
            for (size_t k = 0; k < P.faceCells.size(); ++k) { row[(size_t)x0 + k] = P.faceCells[k]; colv[(size_t)x0 + k] = nbrOff + P.nbrCells[k]; }
        }
        MICHK(g->cIfRow.upload(row, s)); MICHK(g->cIfCol.upload(colv, s));
        MICHK(g->invStatus.upload(Table<int32_t>(1, 0), s));
        if (g->gInv.n != (size_t)nG * (size_t)nG) MICHK(g->gInv.alloc((size_t)nG * (size_t)nG));
    }
    HIPCHK(hipMemsetAsync(g->gA.p, 0, sizeof(double) * (size_t)nG * (size_t)nG, s));
    k_coarsest_assemble<<<gamg_grid(n > nf ? n : nf), 256, 0, s>>>(g->gA.p, nG, off, Lc->cDiag.p, ca->lowerAddr.p, ca->upperAddr.p, Lc->cUp.p,
                                                                  asym ? Lc->cLow.p : nullptr, n, nf, g->cIfRow.p, g->cIfCol.p, Lc->ifUp.p, nx);
    if (g->reduce && g->reduce->nRanks > 1) MICHK(comm_allreduce_raw(g->reduce, s, g->gA.p, (size_t)nG * (size_t)nG));
    // Round 4: the inversion (0.9 ms at 151 global coarsest cells -- one workgroup, 151 dependent pivot steps) is needed by the
    // FIRST coarsest-level solve only, a prologue and a whole down-sweep later: it runs on the context's side stream meanwhile
    // (gamg_wait_inverse makes the engine's stream wait where the inverse is first read).  MI_GAMG_INVERT_OVERLAP=0: in line.
    hipStream_t si = s;
    if (env_int("MI_GAMG_INVERT_OVERLAP", 1)) {
        if (!c->sideStream) {
            HIPCHK(hipStreamCreateWithFlags(&c->sideStream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->evSideGo, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->evSideDone, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(c->evSideGo, s));
        HIPCHK(hipStreamWaitEvent(c->sideStream, c->evSideGo, 0));
        si = c->sideStream;
    }
    if (regPath && env_int("MI_GAMG_INVERT_V2", 1)) {
        switch (((int)nG + 31) / 32) {
        case 1: k_dense_invert_reg2<1><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 2: k_dense_invert_reg2<2><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 3: k_dense_invert_reg2<3><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 4: k_dense_invert_reg2<4><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 5: k_dense_invert_reg2<5><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        default: k_dense_invert_reg2<6><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        }
    } else if (regPath) {   // MI_GAMG_INVERT_V2=0: round 3's kernel (same bits; the A/B of the round-6 rewrite)
        switch (((int)nG + 31) / 32) {
        case 1: k_dense_invert_reg<1, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 2: k_dense_invert_reg<2, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 3: k_dense_invert_reg<3, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 4: k_dense_invert_reg<4, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        case 5: k_dense_invert_reg<5, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        default: k_dense_invert_reg<6, 32><<<1, 1024, 0, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p); break;
        }
    } else
    k_dense_invert<<<1, 1024, sizeof(double) * (size_t)nG, si>>>(g->gA.p, g->gInv.p, (int)nG, g->invStatus.p);
    k_take_rows<<<gamg_grid((int)((size_t)n * (size_t)nG > 1000000 ? 1000000 : (size_t)n * (size_t)nG)), 256, 0, si>>>(g->gInv.p, nG, off, ca->e2c.p, n, g->inv.p);
    HIPCHK(hipGetLastError());
    if (si != s) { HIPCHK(hipEventRecord(c->evSideDone, si)); g->invOnSide = true; }
    g->invPending = true;   // the singular flag is read at the solve's next host synchronisation
    return MI_OK;
}

// Jacobi sweeps with ping-pong; on return *x points at the smoothed field, *t at the scratch
int gamg_smooth(mi_matrix_s* m, double** x, double** t, const double* b, double omega, int sweeps)
{
    for (int sw = 0; sw < sweeps; ++sw) {
        MICHK(tile_op<OP_JACOBI>(m, false, *x, b, nullptr, *t, omega));
        double* q = *x; *x = *t; *t = q;
    }
    return MI_OK;
}

// per-tile partial sums of a level matrix: two arrays of cap = max(nTiles, RG) doubles, zeroed once -- a level with at most
// RG tiles is read by the consumers as the RG block partials directly (slots >= nTiles are never written, so they stay 0)
int tile_partials(mi_matrix_s* m, double** p0, double** p1)
{
    const size_t cap = std::max((size_t)m->addr->L.nTiles, (size_t)RG);
    if (m->tilePartial.n < 2 * cap) {
        MICHK(m->tilePartial.alloc(2 * cap));
        HIPCHK(hipMemsetAsync(m->tilePartial.p, 0, sizeof(double) * 2 * cap, m->addr->ctx->stream));
    }
    *p0 = m->tilePartial.p; *p1 = m->tilePartial.p + cap;
    return MI_OK;
}

int gamg_scale(mi_matrix_s* m, double* field, double* Acf, const double* source, double* addTo = nullptr)
{
    mi_ctx_s* c = m->addr->ctx;
    hipStream_t s = c->stream;
    const int64_t n = m->addr->L.nCells;
    if (!comm_attached(m)) {
        // Amul with BOTH sums of the scaling factor fused (GAMGSolverScale.C:59-107: gSumProd(source, field), gSumProd(Acf, field))
        double *pDen, *pNum;
        MICHK(tile_partials(m, &pDen, &pNum));
        const int nT = m->addr->L.nTiles;
        MICHK(tile_op<OP_AMUL>(m, false, field, source, nullptr, Acf, 0.0, pDen, pNum));
        if (nT > RG) {
            k_fold_partials2<<<2, 1024, 0, s>>>(pNum, pDen, nT, c->partial.p, c->partial.p + RG);
            pNum = c->partial.p; pDen = c->partial.p + RG;
        }
        k_gamg_scale<false><<<RG, RB, 0, s>>>(field, Acf, source, m->diagE.p, pNum, pDen, n, addTo);
        HIPCHK(hipGetLastError());
        return MI_OK;
    }
    // decomposed case (round 4: the same fused form as above -- it used to be an Amul, a separate dot-product pass, three
    // one-workgroup kernels, the all-reduce, the scaling pass and a separate psi update): both local sums come out of the Amul
    // tile pass, ONE workgroup folds them and -- on a communicator in peer mode -- all-reduces them through the windows in the
    // same launch (GAMGSolverScale.C:104-107: the 2-double reduce), the scaling pass adds to psi on the finest level
    double *pDen, *pNum;
    MICHK(tile_partials(m, &pDen, &pNum));
    const int nT = m->addr->L.nTiles;
    MICHK(tile_op<OP_AMUL>(m, false, field, source, nullptr, Acf, 0.0, pDen, pNum));
    double* sc = c->scalars.p + 4;
    if (m->dpc->reduce->peerReady) k_fold_ar<2><<<1, 1024, 0, s>>>(pNum, pDen, nT, sc, peer_ar(m->dpc->reduce));
    else {
        k_fold_final2<<<2, 1024, 0, s>>>(pNum, pDen, nT, sc);
        MICHK(comm_allreduce(m, sc, 2));
    }
    k_gamg_scale<true><<<RG, RB, 0, s>>>(field, Acf, source, m->diagE.p, sc, sc + 1, n, addTo);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

int imin2(int a, int b) { return a < b ? a : b; }
// the controls that decide which kernels a V-cycle enqueues and with which arguments (tolerances / iteration limits do not)
bool same_cycle_shape(const mi_gamg_controls& a, const mi_gamg_controls& b)
{
    return a.nPreSweeps == b.nPreSweeps && a.preSweepsLevelMultiplier == b.preSweepsLevelMultiplier && a.maxPreSweeps == b.maxPreSweeps &&
           a.nPostSweeps == b.nPostSweeps && a.postSweepsLevelMultiplier == b.postSweepsLevelMultiplier && a.maxPostSweeps == b.maxPostSweeps &&
           a.nFinestSweeps == b.nFinestSweeps && a.omega == b.omega && a.directSolveCoarsest == b.directSolveCoarsest;
}

} // namespace



extern "C" int mi_gamg_solve(mi_gamg_t g, mi_matrix_t m, double* psi_io, const double* source,
                             const mi_gamg_controls* ctl, mi_solver_perf* perf, double* hist_host, int32_t hist_len)
{
    if (!g || !m || !psi_io || !source || !ctl) return fail(MI_ERR_ARG, "mi_gamg_solve: bad argument");
    if (m->addr != g->fine) return fail(MI_ERR_ARG, "mi_gamg_solve: matrix does not belong to the hierarchy's addressing");
    if ((g->reduce != nullptr) != comm_attached(m)) return fail(MI_ERR_STATE, "mi_gamg_solve: hierarchy and matrix must both be (or both not be) attached to communicators");
    if (!m->bound) return fail(MI_ERR_STATE, "matrix coefficients not bound");
    if (m->addr->ctx->session) return fail(MI_ERR_STATE, "mi_gamg_solve: a PCG session (mi_pcg_begin) is active on this context; call mi_pcg_end first");
    if ((!g->fine->ami.empty() || comm_any_ami(m)) && ctl->directSolveCoarsest)
        return fail(MI_ERR_UNSUPPORTED, "mi_gamg_solve: cyclicAMI patches need directSolveCoarsest = 0 (the reference's direct coarsest solver only knows cyclic interfaces, LUscalarMatrix.C:246-251)");
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = a->L.nCells;
    const int nL = (int)g->lev.size();
    const int coarsest = nL - 1;
    const bool doScale = ctl->scaleCorrection < 0 ? !m->asym : (ctl->scaleCorrection != 0);
    // GAMGSolver.C:88-172 rebuilds the level matrices for every solver object; the result only depends on the fine
    // coefficients, so they are kept while those have not been re-bound (second corrector / non-orthogonal correctors of a step)
    if (g->aggMatrix != m || g->aggEpoch != m->epoch || c->gamgAlwaysAgglomerate) {
        // (round 6, measured and dropped: the whole agglomeration chain on the side stream beside the prologue -- its ~35 short dependent
        //  launches crawl when they share the device with the prologue's saturating tile pass: pressure solve 7.03 -> 7.13 ms)
        MICHK(gamg_agglomerate(g, m));
        g->aggMatrix = m; g->aggEpoch = m->epoch;
    }

    double *psi, *src, *Apsi, *fcorr, *fres, *tmpv;
    MICHK(m->vec(3, &psi)); MICHK(m->vec(4, &src)); MICHK(m->vec(5, &fcorr)); MICHK(m->vec(6, &Apsi)); MICHK(m->vec(7, &fres)); MICHK(m->vec(8, &tmpv));
    k_gather_perm<<<RG, RB, 0, s>>>(psi_io, a->perm(), psi, a->L.nCells);
    k_gather_perm<<<RG, RB, 0, s>>>(source, a->perm(), src, a->L.nCells);
    mi_solver_controls base; base.tolerance = ctl->tolerance; base.relTol = ctl->relTol; base.maxIter = ctl->maxIter; base.minIter = ctl->minIter;
    HostPerf hp; Table<double> hist;
    MICHK(host_prologue(m, &base, psi, src, Apsi, fres, fcorr, hp, hist)); // Apsi = A psi, fres = src - Apsi, normFactor
    if (!g->invOnSide) MICHK(gamg_check_inverse(g));                        // in-line inversion: the prologue synchronised, it has run (side stream: checked after the first cycle)

    if (hp.minIter > 0 || !hp.checkConvergence()) {
        Table<double*> corr((size_t)nL), csrc((size_t)nL), ctmp((size_t)nL);
        for (int l = 0; l < nL; ++l) { corr[l] = g->lev[l]->corr.p; csrc[l] = g->lev[l]->src.p; ctmp[l] = g->lev[l]->tmp.p; }
        // one V-cycle + finest residual; leaves sum|rA| in c->hostScal[0] once the stream has drained (non-attached matrices)
        double* const psi0 = psi; double* const tmpv0 = tmpv;
        // fused transfers (MI_GAMG_FUSE, default on): default cycle shape (no pre-smoothing), single rank; a level with coupled patches
        // or compact row entries keeps the separate kernels (tile_fx_usable)
        const bool fuse = c->gamgFuse != 0 && !ctl->nPreSweeps && !comm_attached(m);
        if (fuse && g->foldScal.n < 2 * ((size_t)nL + 1)) {
            MICHK(g->foldScal.alloc(2 * ((size_t)nL + 1))); MICHK(g->foldCounter.alloc(1));
            HIPCHK(hipMemsetAsync(g->foldCounter.p, 0, sizeof(unsigned int), s));
        }
        auto enqueue_cycle = [&](double* smOut) -> int {
            // every cycle starts from the same buffers whatever the parity of the sweep counts (the smoothers ping-pong two
            // buffers per level): the coarse corrections are rebuilt from scratch each cycle, so only the pointers need
            // resetting -- a captured cycle then replays with identical kernel arguments for ANY sweep schedule, the
            // reference's defaults (2, 3, 4, 4 ... post sweeps) included
            for (int l = 0; l < nL; ++l) { corr[l] = g->lev[l]->corr.p; ctmp[l] = g->lev[l]->tmp.p; }
            // ---- V-cycle (GAMGSolverSolve.C:181-474) ----
            {
                GamgLevelDev* D = g->lev[0];
                k_gamg_restrict<<<gamg_grid(D->nCoarse), 256, 0, s>>>(fres, D->rStartE.p, D->rChildE.p, csrc[0], D->nCoarse);
            }
            for (int l = 0; l < coarsest; ++l) {
                GamgLevelDev* D = g->lev[l];
                const int nl = D->nCoarse;
                if (ctl->nPreSweeps) {
                    HIPCHK(hipMemsetAsync(corr[l], 0, sizeof(double) * (size_t)nl, s));
                    MICHK(gamg_smooth(D->mat, &corr[l], &ctmp[l], csrc[l], ctl->omega,
                                      imin2(ctl->nPreSweeps + ctl->preSweepsLevelMultiplier * l, ctl->maxPreSweeps)));
                    if (doScale && l < coarsest - 1) MICHK(gamg_scale(D->mat, corr[l], ctmp[l], csrc[l]));
                    MICHK(tile_op<OP_AMUL>(D->mat, false, corr[l], nullptr, nullptr, ctmp[l], 0.0));
                    k_xpsy<<<RG, RB, 0, s>>>(csrc[l], csrc[l], -1.0, ctmp[l], nl); // coarseSources -= ACf
                }
                GamgLevelDev* N = g->lev[(size_t)l + 1];
                k_gamg_restrict<<<gamg_grid(N->nCoarse), 256, 0, s>>>(csrc[l], N->rStartE.p, N->rChildE.p, csrc[(size_t)l + 1], N->nCoarse);
            }
            if (!ctl->directSolveCoarsest) {
                // GAMGSolverSolve.C:572-613: ICCG (PCG + DIC) / BICCG (PBiCG + DILU) on the coarsest level matrix, zero start,
                // GAMG's own tolerance / relTol, default maxIter; on a decomposed case the level matrix is attached, so
                // this is the global coarsest system as well
                GamgLevelDev* D = g->lev[(size_t)coarsest];
                k_scatter_perm<<<RG, RB, 0, s>>>(csrc[(size_t)coarsest], D->addr->e2c.p, D->tmp2.p, D->nCoarse);
                HIPCHK(hipMemsetAsync(D->tmp.p, 0, sizeof(double) * (size_t)D->nCoarse, s));
                mi_solver_controls cc; cc.tolerance = ctl->tolerance; cc.relTol = ctl->relTol; cc.maxIter = 1000; cc.minIter = 0;
                mi_solver_perf pp;
                if (m->asym) MICHK(mi_pbicg_solve(D->mat, D->tmp.p, D->tmp2.p, &cc, MI_PRECOND_AINV, &pp, nullptr, 0));
                else MICHK(mi_pcg_solve(D->mat, D->tmp.p, D->tmp2.p, &cc, MI_PRECOND_AINV, &pp, nullptr, 0));
                k_gather_perm<<<RG, RB, 0, s>>>(D->tmp.p, D->addr->e2c.p, corr[(size_t)coarsest], D->nCoarse);
            } else {
                GamgLevelDev* D = g->lev[(size_t)coarsest];
                // coarsest level (GAMGSolverSolve.C:552-570): every rank's source into the global vector, one all-reduce,
                // then the rows of the global inverse that belong to this rank
                const int64_t nG = g->nGlobalCoarsest;
                const int64_t off = g->rankOffset[(size_t)(g->reduce ? g->reduce->rank : 0)];
                MICHK(gamg_wait_inverse(g));
                if (g->gather && g->gather->ready) {   // all-gather through the peers' windows: two small launches, no collective call
                    k_coarsest_gather_push<<<1, 256, 0, s>>>(csrc[(size_t)coarsest], D->addr->e2c.p, D->nCoarse, off, g->gather->dev(PEER_POLLS));
                    if (D->nCoarse > 0) k_dense_matvec_win<<<(D->nCoarse + 3) / 4, 256, 0, s>>>(g->inv.p, g->gather->dev(PEER_POLLS), corr[(size_t)coarsest], D->nCoarse, (int)nG);
                } else {
                if (g->reduce && g->reduce->nRanks > 1) HIPCHK(hipMemsetAsync(g->gsrc.p, 0, sizeof(double) * (size_t)nG, s));
                k_gamg_scatter_offset<<<gamg_grid(D->nCoarse), 256, 0, s>>>(csrc[(size_t)coarsest], D->addr->e2c.p, g->gsrc.p, off, D->nCoarse);
                if (g->reduce && g->reduce->nRanks > 1) MICHK(comm_allreduce_raw(g->reduce, s, g->gsrc.p, (size_t)nG));
                k_dense_matvec<<<(D->nCoarse + 3) / 4, 256, 0, s>>>(g->inv.p, g->gsrc.p, corr[(size_t)coarsest], D->nCoarse, (int)nG);
                }
            }
            for (int l = coarsest - 1; l >= 0; --l) {
                GamgLevelDev* D = g->lev[l];
                GamgLevelDev* N = g->lev[(size_t)l + 1];
                const int nl = D->nCoarse;
                const int postSweeps = imin2(ctl->nPostSweeps + ctl->postSweepsLevelMultiplier * l, ctl->maxPostSweeps);
                if (fuse && postSweeps >= 1 && tile_fx_usable(D->mat)) {
                    // round 6: the prolongation is formed in the staging of the pass that consumes it, the scaling pass in the staging of
                    // the first smoothing sweep -- prolong + Amul + [fold] + scale + sweep  ->  Amul + sweep, same arithmetic
                    FxArgs fx; fx.map = N->prolongE.p; fx.coarse = corr[(size_t)l + 1];
                    double* first = D->tmp2.p;       // the first sweep's result: neither the field nor Acf (other tiles still read them)
                    if (doScale && l < coarsest - 1) {
                        double *pDen, *pNum;
                        MICHK(tile_partials(D->mat, &pDen, &pNum));
                        fx.out = corr[l]; fx.foldCounter = g->foldCounter.p; fx.foldOut = g->foldScal.p + 2 * (size_t)l;
                        MICHK((launch_tile_fx<OP_AMUL, 1>(D->mat, fx, csrc[l], ctmp[l], 0.0, pDen, pNum)));
                        FxArgs f2; f2.field = corr[l]; f2.acf = ctmp[l]; f2.src = csrc[l]; f2.scal = fx.foldOut;
                        MICHK((launch_tile_fx<OP_JACOBI, 2>(D->mat, f2, csrc[l], first, ctl->omega)));
                    } else MICHK((launch_tile_fx<OP_JACOBI, 1>(D->mat, fx, csrc[l], first, ctl->omega)));
                    double* other = corr[l];
                    corr[l] = first; ctmp[l] = other;
                    MICHK(gamg_smooth(D->mat, &corr[l], &ctmp[l], csrc[l], ctl->omega, postSweeps - 1));
                    continue;
                }
                double* pre = D->tmp2.p;
                if (ctl->nPreSweeps) HIPCHK(hipMemcpyAsync(pre, corr[l], sizeof(double) * (size_t)nl, hipMemcpyDeviceToDevice, s));
                k_gamg_prolong<<<gamg_grid(nl), 256, 0, s>>>(corr[(size_t)l + 1], N->prolongE.p, corr[l], nl);
                if (doScale && l < coarsest - 1) MICHK(gamg_scale(D->mat, corr[l], ctmp[l], csrc[l]));
                if (ctl->nPreSweeps) k_xpsy<<<RG, RB, 0, s>>>(corr[l], corr[l], 1.0, pre, nl);
                MICHK(gamg_smooth(D->mat, &corr[l], &ctmp[l], csrc[l], ctl->omega, postSweeps));
            }
            if (fuse && doScale && ctl->nFinestSweeps >= 1 && tile_fx_usable(m)) {
                // finest level the same way: Amul of the prolonged correction (written to fcorr) with both sums, then the first sweep on
                // psi + scaled correction formed in its staging (psi += finestCorrection never goes through memory)
                double *pDen, *pNum;
                MICHK(tile_partials(m, &pDen, &pNum));
                FxArgs fx; fx.map = g->lev[0]->prolongE.p; fx.coarse = corr[0]; fx.out = fcorr; fx.foldCounter = g->foldCounter.p; fx.foldOut = g->foldScal.p + 2 * (size_t)nL;
                MICHK((launch_tile_fx<OP_AMUL, 1>(m, fx, fres, Apsi, 0.0, pDen, pNum)));
                FxArgs f3; f3.field = fcorr; f3.acf = Apsi; f3.src = fres; f3.scal = fx.foldOut; f3.add = psi;
                MICHK((launch_tile_fx<OP_JACOBI, 3>(m, f3, src, tmpv, ctl->omega)));
                { double* q = psi; psi = tmpv; tmpv = q; }
                MICHK(gamg_smooth(m, &psi, &tmpv, src, ctl->omega, ctl->nFinestSweeps - 1));
            } else {
            k_gamg_prolong<<<gamg_grid((int)n), 256, 0, s>>>(corr[0], g->lev[0]->prolongE.p, fcorr, (int)n);
            if (doScale) MICHK(gamg_scale(m, fcorr, Apsi, fres, psi));                 // ... + psi += finestCorrection in the same pass
            else k_xpsy<<<RG, RB, 0, s>>>(psi, psi, 1.0, fcorr, n);                  // psi += finestCorrection
            MICHK(gamg_smooth(m, &psi, &tmpv, src, ctl->omega, ctl->nFinestSweeps));
            }
            if (psi != psi0) { // odd nFinestSweeps: psi carries over to the next cycle, so it goes back to its own buffer
                HIPCHK(hipMemcpyAsync(psi0, psi, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
                psi = psi0; tmpv = tmpv0;
            }
            // ---- finest residual (GAMGSolverSolve.C:146-160): rA = source - A psi and gSumMag(rA) in one tile pass ----
            (void)smOut;
            {
                double *pMag, *unused;
                MICHK(tile_partials(m, &pMag, &unused));
                MICHK(tile_op<OP_RESIDUAL>(m, false, psi, src, nullptr, fres, 0.0, pMag));   // (exchanges psi's halo on a decomposed case)
                if (comm_attached(m) && m->dpc->reduce->peerReady) k_fold_ar<1><<<1, 1024, 0, s>>>(pMag, nullptr, a->L.nTiles, c->scalars.p, peer_ar(m->dpc->reduce));
                else {
                    k_fold_final<<<1, 1024, 0, s>>>(pMag, a->L.nTiles, c->scalars.p);
                    if (comm_attached(m)) MICHK(comm_allreduce(m, c->scalars.p, 1));   // gSumMag: Foam::reduce
                }
                HIPCHK(hipMemcpyAsync(c->hostScal, c->scalars.p, sizeof(double), hipMemcpyDeviceToHost, s));
            }
            return MI_OK;
        };
        // graph replay needs identical kernel arguments every cycle (enqueue_cycle resets its buffers, above) and a cycle that is
        // stream work only: direct coarsest solve (the iterative one is a host loop); on a decomposed case every exchange of the
        // cycle through peer windows -- the halo of the finest and of every level matrix (k_halo_push + window-reading tiles:
        // their labels are device counters, so a replay issues the next exchange), the scaling factor's and the residual's
        // all-reduce (k_fold_ar), the coarsest level's gather (k_coarsest_gather_push) -- round 4; with RCCL or the caller's
        // transport the cycle is enqueued call by call as before
        bool commStream = true;
        if (comm_attached(m)) {
            commStream = c->gamgGraphAttached != 0 && m->dpc->reduce->peerReady && (!comm_remote(m) || peer_halo_ready(m)) &&
                         (!(g->reduce && g->reduce->nRanks > 1) || (g->gather && g->gather->ready));
            for (int l = 0; l < nL && commStream; ++l) {
                const mi_matrix_s* lm = g->lev[(size_t)l]->mat;
                if (comm_remote(lm) && !peer_halo_ready(lm)) commStream = false;
            }
        }
        const bool graphable = commStream && ctl->directSolveCoarsest && c->gamgGraph;
        bool first = true;
        do {
            double sm = 0;
            if (graphable && !first) {
                auto& K = g->cycleKey;
                if (!g->cycleGraph || K.m != m || K.psi != psi || K.src != src || K.doScale != doScale || K.asym != m->asym || !same_cycle_shape(K.ctl, *ctl)) {
                    if (g->cycleGraph) { (void)hipGraphExecDestroy(g->cycleGraph); g->cycleGraph = nullptr; }
                    hipGraph_t gr = nullptr;
                    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                    const int rcE = enqueue_cycle(&sm);
                    const hipError_t eE = hipStreamEndCapture(s, &gr);
                    MICHK(rcE);
                    HIPCHK(eE);
                    const hipError_t eI = hipGraphInstantiate(&g->cycleGraph, gr, nullptr, nullptr, 0);
                    (void)hipGraphDestroy(gr);
                    HIPCHK(eI);
                    K.m = m; K.psi = psi; K.src = src; K.doScale = doScale; K.asym = m->asym; K.ctl = *ctl;
                }
                HIPCHK(hipGraphLaunch(g->cycleGraph, s));
                if (comm_attached(m)) c->stats[3] += 1;   // mi_ctx_stat(3): V-cycles of a decomposed case replayed as a hipGraph
            } else MICHK(enqueue_cycle(&sm));           // the first cycle runs eagerly: it also sizes every scratch buffer
            HIPCHK(hipStreamSynchronize(s));
            sm = c->hostScal[0];
            if (comm_attached(m) && !(sm == sm && sm < 1e300)) MICHK(peer_check(m));   // (a window wait that ran out voids the sums)
            if (first) MICHK(gamg_check_inverse(g));   // the first cycle waited for the inversion and the stream has drained: singular?
            first = false;
            hp.finalResidual = sm / hp.normFactor;
            hist.push_back(hp.finalResidual);
        } while ((++hp.nIterations < hp.maxIter && !hp.checkConvergence()) || hp.nIterations < hp.minIter);
        if (comm_attached(m)) {
            MICHK(peer_check(m));
            if (g->gather && g->gather->ready) {
                int32_t st = 0;
                HIPCHK(hipMemcpy(&st, g->gather->status, sizeof(int32_t), hipMemcpyDeviceToHost));
                if (st != 0) return fail(MI_ERR_DEVICE, "GAMG coarsest-level gather: a rank never arrived (window wait ran out of polls); the results of this solve are not valid");
            }
        }
    }
    return finish_host(m, hp, hist, psi, psi_io, perf, hist_host, hist_len);
}

// ---- unit-test hooks: level transfer operators and level coefficients -------------------------
extern "C" int mi_gamg_level_coeffs(mi_gamg_t g, mi_matrix_t m, int32_t level, double* diag_out, double* upper_out, double* lower_out)
{
    if (!g || !m || level < 0 || level >= (int32_t)g->lev.size() || !diag_out || !upper_out) return fail(MI_ERR_ARG, "mi_gamg_level_coeffs: bad argument");
    MICHK(gamg_agglomerate(g, m, true));
    g->aggMatrix = nullptr;                    // (the next solve re-agglomerates on its own path)
    GamgLevelDev* D = g->lev[(size_t)level];
    hipStream_t s = g->fine->ctx->stream;
    HIPCHK(hipMemcpyAsync(diag_out, D->cDiag.p, sizeof(double) * (size_t)D->nCoarse, hipMemcpyDeviceToDevice, s));
    if (D->nCoarseFaces) HIPCHK(hipMemcpyAsync(upper_out, D->cUp.p, sizeof(double) * (size_t)D->nCoarseFaces, hipMemcpyDeviceToDevice, s));
    if (lower_out && m->asym && D->nCoarseFaces) HIPCHK(hipMemcpyAsync(lower_out, D->cLow.p, sizeof(double) * (size_t)D->nCoarseFaces, hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

// restrict / prolong between level `level` (fine side) and level+1, vectors in the CALLER order of each level
namespace {
// engine-order scratch of the fine and the coarse side of a level for the caller-order transfer entry points: the level's own
// work vectors (not in use outside mi_gamg_solve), for the finest side a buffer the hierarchy keeps
int gamg_transfer_scratch(mi_gamg_s* g, int32_t level, double** fe, double** ce)
{
    GamgLevelDev* D = g->lev[(size_t)level];
    if (level == 0) {
        if (g->fineScratch.n < (size_t)D->nFine) MICHK(g->fineScratch.alloc((size_t)D->nFine));
        *fe = g->fineScratch.p;
    } else *fe = g->lev[(size_t)level - 1]->tmp2.p;
    *ce = D->tmp.p;
    return MI_OK;
}
} // namespace
// diagnostic / test hook: the dense inversions of the coarsest level on a matrix of the CALLER's (row-major n x n, device memory) --
// which = 0: the host elimination (gamg.cpp invert_dense), 1: k_dense_invert_reg (n <= 192), 2: k_dense_invert_reg2 (n <= 192),
// 3: k_dense_invert (global memory).  The GAMG coarsest matrices are diagonally dominant and never swap rows: this is how the tests
// reach the pivoting paths.  *singular_out = 1 when the elimination met a zero pivot column (inv_dev is unspecified then).
extern "C" int mi_debug_dense_invert(mi_ctx_t c, const double* a_dev, int32_t n, double* inv_dev, int32_t which, int32_t* singular_out)
{
    if (!c || !a_dev || !inv_dev || n < 1 || !singular_out || which < 0 || which > 3) return fail(MI_ERR_ARG, "mi_debug_dense_invert: bad argument");
    if ((which == 1 || which == 2) && n > 192) return fail(MI_ERR_LIMIT, "mi_debug_dense_invert: the register-resident kernels take n <= 192");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    *singular_out = 0;
    if (which == 0) {
        Table<double> A((size_t)n * (size_t)n, 0.0);
        HIPCHK(hipMemcpyAsync(A.data(), a_dev, sizeof(double) * A.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!invert_dense((int)n, A)) { *singular_out = 1; return MI_OK; }
        HIPCHK(hipMemcpyAsync(inv_dev, A.data(), sizeof(double) * A.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return MI_OK;
    }
    DevBuf<double> work; DevBuf<int32_t> st;
    MICHK(work.alloc((size_t)n * (size_t)n)); MICHK(st.alloc(1));
    HIPCHK(hipMemcpyAsync(work.p, a_dev, sizeof(double) * (size_t)n * (size_t)n, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(st.p, 0, sizeof(int32_t), s));
    const int blk = ((int)n + 31) / 32;
    if (which == 1) {
        switch (blk) {
        case 1: k_dense_invert_reg<1, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 2: k_dense_invert_reg<2, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 3: k_dense_invert_reg<3, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 4: k_dense_invert_reg<4, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 5: k_dense_invert_reg<5, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        default: k_dense_invert_reg<6, 32><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        }
    } else if (which == 2) {
        switch (blk) {
        case 1: k_dense_invert_reg2<1><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 2: k_dense_invert_reg2<2><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 3: k_dense_invert_reg2<3><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 4: k_dense_invert_reg2<4><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        case 5: k_dense_invert_reg2<5><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        default: k_dense_invert_reg2<6><<<1, 1024, 0, s>>>(work.p, inv_dev, (int)n, st.p); break;
        }
    } else k_dense_invert<<<1, 1024, sizeof(double) * (size_t)n, s>>>(work.p, inv_dev, (int)n, st.p);
    HIPCHK(hipGetLastError());
    int32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, st.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *singular_out = flag;
    return MI_OK;
}

extern "C" int mi_gamg_restrict(mi_gamg_t g, int32_t level, const double* fine_dev, double* coarse_dev)
{
    if (!g || level < 0 || level >= (int32_t)g->lev.size() || !fine_dev || !coarse_dev) return fail(MI_ERR_ARG, "mi_gamg_restrict: bad argument");
    GamgLevelDev* D = g->lev[(size_t)level];
    const mi_addr_s* fa = level == 0 ? g->fine : g->lev[(size_t)level - 1]->addr;
    HIPCHK(hipSetDevice(g->fine->ctx->device));
    hipStream_t s = g->fine->ctx->stream;
    double *fe, *ce;
    MICHK(gamg_transfer_scratch(g, level, &fe, &ce));
    k_gather_perm<<<RG, RB, 0, s>>>(fine_dev, fa->perm(), fe, D->nFine);
    k_gamg_restrict<<<gamg_grid(D->nCoarse), 256, 0, s>>>(fe, D->rStartE.p, D->rChildE.p, ce, D->nCoarse);
    k_scatter_perm<<<RG, RB, 0, s>>>(ce, D->addr->e2c.p, coarse_dev, D->nCoarse);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_gamg_prolong(mi_gamg_t g, int32_t level, const double* coarse_dev, double* fine_dev)
{
    if (!g || level < 0 || level >= (int32_t)g->lev.size() || !fine_dev || !coarse_dev) return fail(MI_ERR_ARG, "mi_gamg_prolong: bad argument");
    GamgLevelDev* D = g->lev[(size_t)level];
    const mi_addr_s* fa = level == 0 ? g->fine : g->lev[(size_t)level - 1]->addr;
    HIPCHK(hipSetDevice(g->fine->ctx->device));
    hipStream_t s = g->fine->ctx->stream;
    double *fe, *ce;
    MICHK(gamg_transfer_scratch(g, level, &fe, &ce));
    k_gather_perm<<<RG, RB, 0, s>>>(coarse_dev, D->addr->e2c.p, ce, D->nCoarse);
    k_gamg_prolong<<<gamg_grid(D->nFine), 256, 0, s>>>(ce, D->prolongE.p, fe, D->nFine);
    k_scatter_perm<<<RG, RB, 0, s>>>(fe, fa->perm(), fine_dev, D->nFine);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// ---- the pieces of the V-cycle as operators (level-1 integration: the reference keeps GAMGSolverSolve.C and swaps the
//      primitives; tests/ref_dropin runs exactly that) ------------------------------------------------------------------
// GAMGSolver constructor work (GAMGSolver.C:88-172): agglomerateMatrix for every level from the matrix's CURRENT
// coefficients + the coarsest direct solver.  mi_gamg_solve does this itself; call it before using the level operators.
extern "C" int mi_gamg_update(mi_gamg_t g, mi_matrix_t m)
{
    if (!g || !m) return fail(MI_ERR_ARG, "mi_gamg_update: bad argument");
    if (m->addr != g->fine) return fail(MI_ERR_ARG, "mi_gamg_update: matrix does not belong to the hierarchy's addressing");
    if (!m->bound) return fail(MI_ERR_STATE, "matrix coefficients not bound");
    HIPCHK(hipSetDevice(g->fine->ctx->device));
    MICHK(gamg_agglomerate(g, m));
    g->aggMatrix = m; g->aggEpoch = m->epoch;
    MICHK(gamg_wait_inverse(g));
    HIPCHK(hipStreamSynchronize(g->fine->ctx->stream));
    return gamg_check_inverse(g);
}
// matrixLevels_[level] (GAMGSolver.H:120-135): a BORROWED handle (owned by the hierarchy, valid until it is destroyed;
// its coefficients are those of the last mi_gamg_update / mi_gamg_solve).  Vectors are in that level's caller order,
// i.e. the hierarchy's coarse-cell numbering, as mi_gamg_restrict / mi_gamg_prolong use it.
extern "C" int mi_gamg_level_matrix(mi_gamg_t g, int32_t level, mi_matrix_t* out)
{
    if (!g || !out || level < 0 || level >= (int32_t)g->lev.size()) return fail(MI_ERR_ARG, "mi_gamg_level_matrix: bad argument");
    *out = g->lev[(size_t)level]->mat;
    return MI_OK;
}
// GAMGSolver::scale (GAMGSolverScale.C:59-171): Acf = A field; sf = sum(source*field)/stabilise(sum(Acf*field));
// field = sf*field + (source - sf*Acf)/diag.  Caller order; the same kernels (and bits) as inside mi_gamg_solve.
extern "C" int mi_gamg_scale(mi_matrix_t m, double* field, double* Acf, const double* source)
{
    if (!m || !field || !Acf || !source) return fail(MI_ERR_ARG, "mi_gamg_scale: bad argument");
    if (!m->bound) return fail(MI_ERR_STATE, "matrix coefficients not bound");
    mi_addr_s* a = m->addr;
    HIPCHK(hipSetDevice(a->ctx->device));
    hipStream_t s = a->ctx->stream;
    double *f, *A, *b;
    MICHK(m->vec(0, &f)); MICHK(m->vec(1, &A)); MICHK(m->vec(2, &b));
    k_gather_perm<<<RG, RB, 0, s>>>(field, a->perm(), f, a->L.nCells);
    k_gather_perm<<<RG, RB, 0, s>>>(source, a->perm(), b, a->L.nCells);
    MICHK(gamg_scale(m, f, A, b));
    k_scatter_perm<<<RG, RB, 0, s>>>(f, a->perm(), field, a->L.nCells);
    k_scatter_perm<<<RG, RB, 0, s>>>(A, a->perm(), Acf, a->L.nCells);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// GAMGSolver::solveCoarsestLevel with directSolveCoarsest (GAMGSolverSolve.C:552-570): corr = A_coarsest^-1 source on the
// device (dense inverse built by mi_gamg_update), caller order of the coarsest level; all ranks call together.
extern "C" int mi_gamg_solve_coarsest(mi_gamg_t g, const double* source_dev, double* corr_dev)
{
    if (!g || !source_dev || !corr_dev || g->lev.empty()) return fail(MI_ERR_ARG, "mi_gamg_solve_coarsest: bad argument");
    if (!g->fine->ami.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_gamg_solve_coarsest: no direct coarsest solver with cyclicAMI patches (LUscalarMatrix.C:246-251)");
    if (g->inv.n == 0) return fail(MI_ERR_STATE, "mi_gamg_solve_coarsest: no level matrices yet (mi_gamg_update)");
    mi_ctx_s* c = g->fine->ctx;
    HIPCHK(hipSetDevice(c->device));
    MICHK(gamg_wait_inverse(g));
    hipStream_t s = c->stream;
    GamgLevelDev* D = g->lev.back();
    const int64_t nG = g->nGlobalCoarsest;
    const int64_t off = g->rankOffset[(size_t)(g->reduce ? g->reduce->rank : 0)];
    k_gather_perm<<<RG, RB, 0, s>>>(source_dev, D->addr->e2c.p, D->src.p, D->nCoarse);
    if (g->reduce && g->reduce->nRanks > 1) HIPCHK(hipMemsetAsync(g->gsrc.p, 0, sizeof(double) * (size_t)nG, s));
    k_gamg_scatter_offset<<<gamg_grid(D->nCoarse), 256, 0, s>>>(D->src.p, D->addr->e2c.p, g->gsrc.p, off, D->nCoarse);
    if (g->reduce && g->reduce->nRanks > 1) MICHK(comm_allreduce_raw(g->reduce, s, g->gsrc.p, (size_t)nG));
    k_dense_matvec<<<(D->nCoarse + 3) / 4, 256, 0, s>>>(g->inv.p, g->gsrc.p, D->corr.p, D->nCoarse, (int)nG);
    k_scatter_perm<<<RG, RB, 0, s>>>(D->corr.p, D->addr->e2c.p, corr_dev, D->nCoarse);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// ---- host-only hierarchy inspection (no device; CPU tests compare it with the oracle's) --------
extern "C" int mi_gamg_host_build(int32_t n_cells, int32_t n_faces, const int32_t* lower, const int32_t* upper,
                                  const double* face_weights, int32_t n_cells_in_coarsest_level, int32_t merge_levels, int forward_init, void** out)
{
    if (!out) return fail(MI_ERR_ARG, "mi_gamg_host_build: out is NULL");
    GamgHierarchyHost* H = new GamgHierarchyHost();
    const std::string err = build_gamg_hierarchy(n_cells, n_faces, lower, upper, face_weights, n_cells_in_coarsest_level, forward_init != 0, *H, nullptr, merge_levels);
    if (!err.empty()) { delete H; return fail(MI_ERR_ARG, "mi_gamg_host_build: " + err); }
    *out = H;
    return MI_OK;
}
// All domains of a decomposed case in ONE process, one thread per domain running the same per-rank builder a real rank runs
// (build_gamg_hierarchy with coupling callbacks); the "communicator" is a barrier and a shared table.  Lets CPU tests compare the
// per-rank hierarchies (agglomeration of the processor patches included) with the oracle's multi-domain builder.
namespace {
struct HostDomainsExchange {
    int nDomains = 0;
    std::mutex mu; std::condition_variable cv; int waiting = 0; long generation = 0;
    bool andAcc = true, andResult = true;
    Table<Table<Table<int32_t>>> board;   // [domain][patch] -> values published for the neighbour
    Table<Table<int32_t>> nbrDomain, nbrPatch;
    void barrier(const std::function<void()>& last = nullptr)
    {
        std::unique_lock<std::mutex> lk(mu);
        const long gen = generation;
        if (++waiting == nDomains) { if (last) last(); waiting = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen; });
    }
};
struct HostDomainCtx { HostDomainsExchange* X; int d; };
bool hd_all_and(void* user, bool v)
{
    HostDomainCtx* c = static_cast<HostDomainCtx*>(user);
    { std::lock_guard<std::mutex> lk(c->X->mu); c->X->andAcc = c->X->andAcc && v; }
    c->X->barrier([&] { c->X->andResult = c->X->andAcc; c->X->andAcc = true; });
    const bool r = c->X->andResult;
    c->X->barrier();
    return r;
}
bool hd_nbr_restrict(void* user, int, const Table<Table<int32_t>>& send, Table<Table<int32_t>>& recv)
{
    HostDomainCtx* c = static_cast<HostDomainCtx*>(user);
    HostDomainsExchange& X = *c->X;
    X.board[(size_t)c->d] = send;
    X.barrier();
    recv.assign(send.size(), Table<int32_t>());
    for (size_t p = 0; p < send.size(); ++p) {
        const int nd = X.nbrDomain[(size_t)c->d][p], np = X.nbrPatch[(size_t)c->d][p];
        if (nd >= 0) recv[p] = X.board[(size_t)nd][(size_t)np];
    }
    X.barrier();
    return true;
}
} // namespace

extern "C" int mi_gamg_host_build_domains(int32_t n_domains, const int32_t* n_cells, const int32_t* n_faces, const int32_t* const* lower,
                                          const int32_t* const* upper, const double* const* face_weights, const int32_t* n_patches,
                                          const int32_t* const* patch_sizes, const int32_t* const* const* patch_face_cells,
                                          const int32_t* const* patch_nbr_domain, const int32_t* const* patch_nbr_patch,
                                          int32_t n_cells_in_coarsest_level, int32_t merge_levels, int forward_init, void** out)
{
    if (n_domains < 1 || !n_cells || !n_faces || !lower || !upper || !face_weights || !n_patches || !out) return fail(MI_ERR_ARG, "mi_gamg_host_build_domains: bad argument");
    HostDomainsExchange X;
    X.nDomains = n_domains;
    X.board.resize((size_t)n_domains); X.nbrDomain.resize((size_t)n_domains); X.nbrPatch.resize((size_t)n_domains);
    Table<GamgHierarchyHost*> H((size_t)n_domains, nullptr);
    Table<GamgCoupling> cpl((size_t)n_domains);
    Table<HostDomainCtx> ctxs((size_t)n_domains);
    Table<std::string> errs((size_t)n_domains);
    for (int d = 0; d < n_domains; ++d) {
        GamgCoupling& c = cpl[(size_t)d];
        c.nPatches = n_patches[d];
        for (int p = 0; p < n_patches[d]; ++p) {
            c.faceCells.emplace_back(patch_face_cells[d][p], patch_face_cells[d][p] + patch_sizes[d][p]);
            c.nbrCells.emplace_back();
            c.isLocal.push_back(0);
            X.nbrDomain[(size_t)d].push_back(patch_nbr_domain[d][p]); X.nbrPatch[(size_t)d].push_back(patch_nbr_patch[d][p]);
        }
        ctxs[(size_t)d] = HostDomainCtx{&X, d};
        c.allAnd = hd_all_and; c.nbrRestrict = hd_nbr_restrict; c.user = &ctxs[(size_t)d];
        H[(size_t)d] = new GamgHierarchyHost();
    }
    Table<std::thread> th;
    for (int d = 0; d < n_domains; ++d)
        th.emplace_back([&, d] {
            errs[(size_t)d] = build_gamg_hierarchy(n_cells[d], n_faces[d], lower[d], upper[d], face_weights[d], n_cells_in_coarsest_level,
                                                   forward_init != 0, *H[(size_t)d], &cpl[(size_t)d], merge_levels);
        });
    for (auto& t : th) t.join();
    for (int d = 0; d < n_domains; ++d)
        if (!errs[(size_t)d].empty()) { for (auto* h : H) delete h; return fail(MI_ERR_ARG, "mi_gamg_host_build_domains: " + errs[(size_t)d]); }
    for (int d = 0; d < n_domains; ++d) out[d] = H[(size_t)d];
    return MI_OK;
}
// One domain whose coupled patches are all cyclicAMI (host only: CPU tests compare the agglomerated AMI of every level with
// the oracle's).  ami_start / ami_addr / ami_w / ami_mag_sf: per patch, as mi_addr_set_ami_patch / mi_addr_set_ami_face_areas take them.
extern "C" int mi_gamg_host_build_ami(int32_t n_cells, int32_t n_faces, const int32_t* lower, const int32_t* upper, const double* face_weights,
                                      int32_t n_cells_in_coarsest_level, int32_t n_patches, const int32_t* patch_sizes,
                                      const int32_t* const* patch_face_cells, const int32_t* patch_nbr_patch, const int32_t* const* ami_start,
                                      const int32_t* const* ami_addr, const double* const* ami_w, const double* const* ami_mag_sf, void** out)
{
    if (!out || n_patches < 1 || !patch_sizes || !patch_face_cells || !patch_nbr_patch || !ami_start || !ami_addr || !ami_w || !ami_mag_sf)
        return fail(MI_ERR_ARG, "mi_gamg_host_build_ami: bad argument");
    GamgCoupling c;
    c.nPatches = n_patches;
    c.ami.resize((size_t)n_patches);
    for (int p = 0; p < n_patches; ++p) {
        c.faceCells.emplace_back(patch_face_cells[p], patch_face_cells[p] + patch_sizes[p]);
        c.nbrCells.emplace_back();
        c.isLocal.push_back(2);
        GamgCoupling::Ami& A = c.ami[(size_t)p];
        A.nbrPatch = patch_nbr_patch[p];
        A.start.assign(ami_start[p], ami_start[p] + patch_sizes[p] + 1);
        A.addr.assign(ami_addr[p], ami_addr[p] + A.start.back());
        A.w.assign(ami_w[p], ami_w[p] + A.start.back());
        A.magSf.assign(ami_mag_sf[p], ami_mag_sf[p] + patch_sizes[p]);
    }
    GamgHierarchyHost* H = new GamgHierarchyHost();
    const std::string err = build_gamg_hierarchy(n_cells, n_faces, lower, upper, face_weights, n_cells_in_coarsest_level, true, *H, &c, 1);
    if (!err.empty()) { delete H; return fail(MI_ERR_ARG, "mi_gamg_host_build_ami: " + err); }
    *out = H;
    return MI_OK;
}
// coupled patch p of a level of a hierarchy built with coupling: faceRestrict (fine patch faces -> coarse interface face), faceCells
extern "C" int mi_gamg_host_patch_array(void* h, int32_t level, int32_t patch, const char* name, const void** data, int64_t* len)
{
    if (!h || !name || !data || !len) return fail(MI_ERR_ARG, "mi_gamg_host_patch_array: bad argument");
    GamgHierarchyHost* H = static_cast<GamgHierarchyHost*>(h);
    if (level < 0 || level >= (int32_t)H->levels.size() || patch < 0 || patch >= (int32_t)H->levels[(size_t)level].patches.size()) return fail(MI_ERR_ARG, "mi_gamg_host_patch_array: bad level / patch");
    GamgPatchHost& P = H->levels[(size_t)level].patches[(size_t)patch];
    const std::string n(name);
    if (n == "faceRestrict") { *data = P.faceRestrict.data(); *len = (int64_t)P.faceRestrict.size(); return MI_OK; }
    if (n == "faceCells") { *data = P.faceCells.data(); *len = (int64_t)P.faceCells.size(); return MI_OK; }
    if (n == "nbrCells") { *data = P.nbrCells.data(); *len = (int64_t)P.nbrCells.size(); return MI_OK; }
    if (n == "amiStart") { *data = P.amiStart.data(); *len = (int64_t)P.amiStart.size(); return MI_OK; }
    if (n == "amiAddr") { *data = P.amiAddr.data(); *len = (int64_t)P.amiAddr.size(); return MI_OK; }
    if (n == "amiW") { *data = P.amiW.data(); *len = (int64_t)P.amiW.size(); return MI_OK; }         // doubles
    if (n == "amiMagSf") { *data = P.amiMagSf.data(); *len = (int64_t)P.amiMagSf.size(); return MI_OK; } // doubles
    return fail(MI_ERR_ARG, "mi_gamg_host_patch_array: unknown array " + n);
}
extern "C" int32_t mi_gamg_host_n_levels(void* h) { return h ? (int32_t)static_cast<GamgHierarchyHost*>(h)->levels.size() : 0; }
extern "C" int mi_gamg_host_array(void* h, int32_t level, const char* name, const void** data, int64_t* len, int32_t* elem_size)
{
    if (!h || !name || !data || !len || !elem_size) return fail(MI_ERR_ARG, "mi_gamg_host_array: bad argument");
    GamgHierarchyHost* H = static_cast<GamgHierarchyHost*>(h);
    if (level < 0 || level >= (int32_t)H->levels.size()) return fail(MI_ERR_ARG, "mi_gamg_host_array: bad level");
    GamgLevelHost& L = H->levels[(size_t)level];
    const std::string n(name);
#define ARR(field) if (n == #field) { *data = L.field.data(); *len = (int64_t)L.field.size(); *elem_size = (int32_t)sizeof(L.field[0]); return MI_OK; }
    ARR(restrictMap) ARR(faceRestrict) ARR(faceFlip) ARR(cLower) ARR(cUpper) ARR(cellChildStart) ARR(cellChild)
    ARR(faceChildStart) ARR(faceChild) ARR(diagChildStart) ARR(diagChild)
#undef ARR
    return fail(MI_ERR_ARG, "mi_gamg_host_array: unknown array " + n);
}
extern "C" int mi_gamg_host_free(void* h) { delete static_cast<GamgHierarchyHost*>(h); return MI_OK; }
