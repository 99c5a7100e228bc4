// assembly.inc -- fvMatrix assembly sweeps on caller-order arrays (included by engine.hip).
//
// The reference builds a matrix with 3-6 separate Thrust passes and temporaries per scheme
// (SURVEY.md 3.5: lower = -w*phi; upper = lower + phi; negSumDiag(); ...).  Here every scheme is
// ONE row-parallel pass: a thread owns a cell, walks its own faces (contiguous in the caller's
// upper-triangular order => coalesced) and its neighbour faces through losort, writes the face
// coefficients it owns and the finished diagonal.  Row sums keep the reference's order
// (lduAddressingFunctors.H:10-64: own faces ascending, then losort), so results are bit-identical
// to the oracle.  Boundary (patch) contributions use per-patch unique-cell segments
// (lduAddressing.C:38-167 patchSortCells/Addr/StartAddr) -- race free and deterministic.
namespace mi {

enum { ROW_SUMDIAG = 0, ROW_NEGSUMDIAG = 1, ROW_SUMMAGOFFDIAG = 2 };
enum { M_PLUS = 0, M_MINUS = 1, M_MAG = 2 };

template <int MODE> __device__ __forceinline__ double face_term(double v) { return MODE == M_PLUS ? v : MODE == M_MINUS ? -v : fabs(v); }
// A streaming pass states its formula ONCE: f(x, o) sees one element -- x[k] its value in input stream k, o[k] what goes to output stream k --
// and runs for both lanes of a 16-byte pair and for the unpaired last element of an odd chunk.  Every load of an element precedes its
// stores, so a stream updated in place stands in both lists.  UNROLL 4: chunk_loop, 2: chunk_loop2 (kernels.hip.hpp).
template <int UNROLL, int NIN, int NOUT, class F>
__device__ __forceinline__ void cell_map(int64_t n, const double* const (&in)[NIN], double* const (&out)[NOUT], F f)
{
    auto pair = [&](int64_t i) {
        double x[NIN], y[NIN], ox[NOUT], oy[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; ++k) { const double2 v = ld2(in[k], i); x[k] = v.x; y[k] = v.y; }
        f(x, ox); f(y, oy);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) st2(out[k], i, make_double2(ox[k], oy[k]));
    };
    auto one = [&](int64_t i) {
        double x[NIN], o[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; ++k) x[k] = in[k][i];
        f(x, o);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) out[k][i] = o[k];
    };
    if (UNROLL == 4) chunk_loop(n, pair, one); else chunk_loop2(n, pair, one);
}

// Row sum over faces: out[c] = (init ? init[c] : 0) + sum_{own faces} f(ownArr[j]) + sum_{neighbour faces} g(neiArr[losort])
// [/ vol[c]].  A workgroup owns RS consecutive cells; their own faces are one contiguous range in the
// owner-sorted order, so they are read with coalesced loads into LDS and each cell then adds its segment in
// ascending face order (the reference's order, lduAddressingFunctors.H:10-64); neighbour-side faces are
// gathered through losort (they are nearby in memory: L2 hits).
// XCD-aware block -> cell-range mapping (as in tile_kernel): hardware places block b on XCD b % 8; giving every XCD a contiguous
// run of cell ranges lets the neighbour-side gathers (faces owned by cells one row / one plane back) hit that XCD's own L2
__device__ __forceinline__ int xcd_block()
{
    const int b = blockIdx.x, per = gridDim.x >> 3;
    return (b < (per << 3)) ? (b & 7) * per + (b >> 3) : b;
}
// contiguous chunk of [0, n) for this block (XCD-aware when xcd != 0): face passes that gather cell values keep the cells of
// neighbouring faces in one XCD's L2
__device__ __forceinline__ void block_chunk(int n, int xcd, int& i0, int& i1)
{
    const int G = gridDim.x, lb = xcd ? xcd_block() : (int)blockIdx.x;
    const int chunk = (((n + G - 1) / G) + 255) & ~255;
    i0 = lb * chunk < n ? lb * chunk : n;
    i1 = i0 + chunk < n ? i0 + chunk : n;
}
// ---- row pass over blocks of consecutive cells -----------------------------------------------------------------------
// One workgroup owns the cells [c0, cEnd): a fixed range of BS cells, or -- when the addressing keeps the caller's numbering
// tile-contiguous (mi_addr_create_ordered, mi_addr_s::identity) -- one tile of the layout, so that most neighbour-side faces
// of its cells are owned by cells of the same block.  The block's own faces are one contiguous range [f0, f1) of the
// owner-sorted face order: their values (or, for the fused scheme passes, the face coefficients computed from them) go to
// LDS once; each cell then adds its own segment in ascending face order and its neighbour-side faces in losort order (the
// reference's order, lduAddressingFunctors.H:10-64).  A neighbour-side face f of cell c is owned by a cell < c, so it lies in
// the block's range exactly when f >= f0: those come from LDS, the rest (faces cut by the block boundary) are gathered --
// and, for the fused passes, recomputed from the scheme's inputs with the same roundings.
//   RP_SUM        out = [init] + sum_own f(a0) + sum_nei g(a1)  [/ vol]     (sumDiag, negSumDiag, sumMagOffDiag, surfaceIntegrate)
//   RP_LAPLACIAN  upper = a0*a1 (deltaCoeffs * gammaMagSf); diag = -sum_own upper - sum_nei upper   (gaussLaplacianScheme.C:44-88)
//   RP_DIV        lower = -a0*a1 (weights * faceFlux), upper = lower + a1; diag = -sum_own lower - sum_nei upper
//                                                                                                 (gaussConvectionScheme.C:74-115)
enum { RP_SUM = 0, RP_LAPLACIAN = 1, RP_DIV = 2 };
// R16 (round 4: 10 of the 20 table bytes a cell costs): block-local 16-bit row tables.  row16[c] = {own-face end, neighbour-list
// end} of cell c relative to the block's first own face / first neighbour-list entry (a cell's starts are the previous cell's
// ends); losort16 holds the neighbour-side faces as 16-bit indices into the block's own faces (the ones staged in LDS), or --
// top bit set -- as an index into the block's list of CUT faces (esc: global face ids, owned by cells of earlier blocks).
struct RowPassArgs {
    const uint32_t* row16; const uint16_t* losort16; const int32_t *esc, *escStart;
    const int32_t *os, *ls, *losort, *blockStart; // blockStart: [nBlocks+1] tile starts, or nullptr: fixed ranges of BS cells
    const double *a0, *a1;
    double *f0out, *f1out;                        // face outputs of the fused passes (upper | lower, upper)
    const double *init, *vol;                     // init may alias out (in-place row ops)
    double* out;
    int n, cap, xcd;                              // cap: doubles per LDS array
    // flux passes (k_face_flux, k_ddt_phi_corr): caller-order face addressing, face area vectors, the cell vector (and its optional cell scale), the optional added face term
    const int32_t *lo, *up;
    const double *sx, *sy, *sz, *vx, *vy, *vz, *sc, *addA, *addB;
};
// one face of k_face_flux / k_ddt_phi_corr: the interpolate is one fma per component (surfaceInterpolationScheme.C:275-280), the dot
// product x*x' + y*y' + z*z' = fma(z, z', fma(x, x', y*y')) (of two products the first is fused: pinned by the compiled reference), the scaled cell vector rounded per cell (it is a cell field in the reference), the added term
// a rounded field product -- the oracle's flux_face (oracle/fvm_oracle.c), operation for operation
__device__ __forceinline__ double flux_face(const RowPassArgs& a, int f)
{
    const int P = a.lo[f], N = a.up[f];
    const double l = a.a0[f];
    double px = a.vx[P], py = a.vy[P], pz = a.vz[P], nx = a.vx[N], ny = a.vy[N], nz = a.vz[N];
    if (a.sc) { const double sp = a.sc[P], sn = a.sc[N]; px = sp * px; py = sp * py; pz = sp * pz; nx = sn * nx; ny = sn * ny; nz = sn * nz; }
    const double ix = fma(l, px - nx, nx), iy = fma(l, py - ny, ny), iz = fma(l, pz - nz, nz);
    double d = fma(iz, a.sz[f], fma(ix, a.sx[f], iy * a.sy[f]));   // Vector operator& as the compiled reference rounds it (oracle/_ref/libref_fvm.so)
    if (a.addA) d = d + (a.addB ? a.addA[f] * a.addB[f] : a.addA[f]);
    return d;
}
template <int KIND, int OM, int NM, int BS, bool R16>
__global__ __launch_bounds__(BS) void k_row_pass(const RowPassArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    const int lb = a.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.blockStart) { c0 = a.blockStart[lb]; cEnd = a.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.os[c0], nf = a.os[cEnd] - f0;
    const bool staged = nf <= a.cap;
    const bool two = KIND == RP_DIV || (KIND == RP_SUM && a.a1 != a.a0); // owner side and neighbour side read different arrays
    double* sOwn = rp_smem;
    double* sNei = two ? rp_smem + a.cap : rp_smem;
    if (KIND == RP_SUM) {
        if (staged) { stage_dma8<BS>(a.a0 + f0, sOwn, nf, tid); if (two) stage_dma8<BS>(a.a1 + f0, sNei, nf, tid); }
    } else { // the face pass of the scheme over the block's own faces: coalesced, every face written exactly once
#pragma unroll 4
        for (int j = tid; j < nf; j += BS) {
            const double u = a.a0[f0 + j], v = a.a1[f0 + j];
            if (KIND == RP_LAPLACIAN) { const double p = u * v; a.f0out[f0 + j] = p; if (staged) sOwn[j] = p; }
            else { const double lo = -u * v, up = lo + v; a.f0out[f0 + j] = lo; a.f1out[f0 + j] = up; if (staged) { sOwn[j] = lo; sNei[j] = up; } }
        }
    }
    auto nei_global = [&](int f) -> double {
        if (KIND == RP_SUM) return a.a1[f];
        const double u = a.a0[f], v = a.a1[f];
        if (KIND == RP_LAPLACIAN) return u * v;
        const double lo = -u * v; return lo + v;
    };
    auto own_global = [&](int f) -> double {
        if (KIND == RP_SUM) return a.a0[f];
        const double u = a.a0[f], v = a.a1[f];
        return KIND == RP_LAPLACIAN ? u * v : -u * v;
    };
    double acc = 0.0;
    int nb = 0, ne = 0, ob = 0, oe = 0;
    const int escBase = R16 ? a.escStart[lb] : 0;
    if (live) {
        acc = a.init ? a.init[c] : 0.0;
        if (R16) {
            const uint32_t w1 = a.row16[c], w0 = tid ? a.row16[c - 1] : 0u;
            const int lsBase = a.ls[c0];
            ob = f0 + (int)(w0 & 0xFFFFu); oe = f0 + (int)(w1 & 0xFFFFu); nb = lsBase + (int)(w0 >> 16); ne = lsBase + (int)(w1 >> 16);
        } else { nb = a.ls[c]; ne = a.ls[c + 1]; ob = a.os[c]; oe = a.os[c + 1]; }
    }
    auto nei_face = [&](int j) -> int {
        if (!R16) return a.losort[j];
        const unsigned e = a.losort16[j];
        return (e & 0x8000u) ? a.esc[escBase + (int)(e & 0x7FFFu)] : f0 + (int)e;
    };
    // cut neighbour-side faces are fetched before the barrier (independent of the staged data)
    const int cnt = ne - nb;
    int nfk[4]; double nv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nfk[k] = (k < cnt) ? nei_face(nb + k) : 0;
        nv[k] = (k < cnt && (!staged || nfk[k] < f0)) ? nei_global(nfk[k]) : 0.0;
    }
    __syncthreads();
    if (!live) return;
    if (staged) for (int j = ob - f0; j < oe - f0; ++j) acc += face_term<OM>(sOwn[j]);
    else for (int j = ob; j < oe; ++j) acc += face_term<OM>(own_global(j));
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) acc += face_term<NM>((staged && nfk[k] >= f0) ? sNei[nfk[k] - f0] : nv[k]);
    for (int j = nb + 4; j < ne; ++j) { const int f = nei_face(j); acc += face_term<NM>((staged && f >= f0) ? sNei[f - f0] : nei_global(f)); }
    a.out[c] = a.vol ? acc / a.vol[c] : acc;
}


// ---- explicit correction of the corrected convection schemes (linearUpwind, LUST) ---------------------------------------------
// gaussConvectionScheme<Type>::fvmDiv adds fvc::surfaceIntegrate(faceFlux*correction(vf)) to the matrix (gaussConvectionScheme.C:109-112).
// linearUpwind<Type>::correction (linearUpwind.C:33-47, functor on the internal faces): the cell is the owner when faceFlux > 0 -- STRICT,
// while the weights use pos() (>= 0) -- the neighbour otherwise, and corr = (Cf - C[cell]) & grad[cell], the three differences formed
// first.  For a vector field `vector & tensor` gives component r as the same scalar expression on component r's gradient; the dot
// product is contracted as flux_face's and k_limited_linear_weights' are.  LUST scales it (0.25*correction, a stored field: rounded,
// LUST.H:120-126); the face term faceFlux*(scale*corr) is a second stored field.  Gradients: grad[3*r + k] = d(vf_r)/dx_k.
struct CorrIn {
    const double *cf[3], *cc[3], *grad[12];
    double scale;
};
__device__ __forceinline__ double lu_dot(double dx, double dy, double dz, double gx, double gy, double gz) { return fma(dz, gz, fma(dx, gx, dy * gy)); }
__device__ __forceinline__ void lu_face(const CorrIn& q, int nRhs, const int32_t* lo, const int32_t* up, const double* flux, int f, double t[4])
{
    const double fl = flux[f];
    const int c = fl > 0 ? lo[f] : up[f];
    const double dx = q.cf[0][f] - q.cc[0][c], dy = q.cf[1][f] - q.cc[1][c], dz = q.cf[2][f] - q.cc[2][c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < nRhs) t[r] = fl * (q.scale * lu_dot(dx, dy, dz, q.grad[3 * r][c], q.grad[3 * r + 1][c], q.grad[3 * r + 2][c]));
}

// ---- fused matrix assembly: [fvm::ddt] + [fvm::div] - [fvm::laplacian] [+- fvm::Sp] [+- explicit terms] in ONE row pass ----------
// (SURVEY 8f rank 1; fvMatrix::operator+= / -= / == on fvMatrix.C:1693-2030, lduMatrix::operator+= / -= on lduMatrixOperations.C:235-396.)
// The reference forms every scheme's matrix with its own passes and temporaries and then combines them coefficient array by
// coefficient array; here a block computes, per own face, lB = -w*flux, uB = lB + flux (gaussConvectionScheme.C:94-95) and
// uL = deltaCoeffs*gammaMagSf (gaussLaplacianScheme.C:63), writes lower = lB - uL and upper = uB - uL ONCE, keeps lB / uB / uL in LDS
// and every cell forms its two negSumDiag row sums (lduMatrixOperations.C:61-83: own faces ascending, then losort order) side by side,
// then diag = ((ddt + sumB) - sumL) [+- V*sp] and the sources.  Every intermediate is rounded exactly where the unfused sequence
// rounds it, so the outputs are bit-identical to mi_fvm_ddt_euler* + mi_fvm_div + mi_fvm_laplacian + the mi_vec_axpby combinations.
struct AsmArgs {
    const uint32_t* row16; const uint16_t* losort16; const int32_t *esc, *escStart;
    const int32_t *os, *ls, *losort, *blockStart;
    int n, cap, xcd;
    const double *flux, *w, *delta, *gam;          // w == nullptr: upwind, w = pos(flux)
    double *lowerOut, *upperOut;                  // lowerOut may be nullptr when there is no convection (symmetric result)
    int ddt; double rdt, rhoValue; const double *rho, *rhoOld, *vol;
    const double* sp; int spMinus;
    int nRhs, nSu;
    const double* psiOld[4]; double* sourceOut[4]; const double* su[16]; int suMinus[4];   // su[k * nRhs + r]
    double *diagOut, *sumMagOut;
};
struct AsmCorrArgs : AsmArgs { const int32_t *lo, *up; CorrIn corr; };   // CORR: caller-order face addressing and the correction's inputs
// BACK: the backward time derivative in place of Euler's (backwardDdtScheme.C:456-607, static mesh): cA = coefft*rDeltaT (a host product,
// as the reference forms it), the old-old fields; rdt / rhoValue / rho / rhoOld / psiOld of AsmArgs keep their meaning
struct BackIn { double cA, c0, c00; const double* rhoOldOld; const double* psiOldOld[4]; };
struct AsmBackArgs : AsmArgs { BackIn bw; };
struct AsmCorrBackArgs : AsmCorrArgs { BackIn bw; };
// CN: the CrankNicolson time derivative (CrankNicolsonDdtScheme.C:755-1003, static mesh): rdt carries rDtCoef, the diagonal is Euler's with it,
// and every source starts ((rdt*rho0)*psi0 + off(ddt0))*V -- ONE more cell array per right-hand side (ddt0, already updated for this time
// step by mi_ddt_cn_update); off(x) = oc*x when offc (oc < 1, decided on the host: wave-uniform), else x (offCentre_, :250-267)
struct CnIn { double oc; int offc; const double* ddt0[4]; };
struct AsmCnArgs : AsmArgs { CnIn cn; };
struct AsmCorrCnArgs : AsmCorrArgs { CnIn cn; };
// LOCAL: the local-time-step derivative (localEulerDdtScheme.C:339-445, CoEulerDdtScheme.C:459-606, static mesh) and / or the bounded Gauss
// convection (boundedConvectionScheme.C:69-92).  rdt given: Euler's expressions with rDeltaT read per cell, a.rdt ignored; rdt null: a.ddt
// decides between Euler and no time derivative (steadyState), as in TF_EULER.  divPhi given: sumB - V*divPhi (fvm::Sp(divPhi, vf) subtracted
// from the convection matrix, the product rounded first: fvmSup.C:118) before sumB meets the time part.  Both are wave-uniform tests.
struct LocalIn { const double *rdt, *divPhi; };
struct AsmLocalArgs : AsmArgs { LocalIn loc; };
struct AsmCorrLocalArgs : AsmCorrArgs { LocalIn loc; };
// the time form of a row pass: TF_EULER (or no time derivative: a.ddt), TF_BACK, TF_CN, TF_LOCAL; each form's kernels take the arguments of that form only
enum { TF_EULER = 0, TF_BACK = 1, TF_CN = 2, TF_LOCAL = 3 };
template <bool CORR, int TF> struct AsmSel { typedef typename std::conditional<CORR, AsmCorrArgs, AsmArgs>::type type; };
template <> struct AsmSel<false, TF_BACK> { typedef AsmBackArgs type; };
template <> struct AsmSel<true, TF_BACK> { typedef AsmCorrBackArgs type; };
template <> struct AsmSel<false, TF_CN> { typedef AsmCnArgs type; };
template <> struct AsmSel<true, TF_CN> { typedef AsmCorrCnArgs type; };
template <> struct AsmSel<false, TF_LOCAL> { typedef AsmLocalArgs type; };
template <> struct AsmSel<true, TF_LOCAL> { typedef AsmCorrLocalArgs type; };
// fvm::ddt, backward: every product and difference rounded on its own (the reference's field operators; DESIGN 3.5d).  Constant density:
// rho_value joins the (rDeltaT*V) factor; a density field: rho0 / rho00 join the coefficients inside the bracket.
__device__ __forceinline__ double back_diag(double cA, double rho, double V) { return (cA * rho) * V; }
__device__ __forceinline__ double back_source(double rdt, double rhoValue, double c0, double c00, double V, double p0, double p00)
{
    return ((rdt * V) * rhoValue) * ((c0 * p0) - (c00 * p00));
}
__device__ __forceinline__ double back_source_rho(double rdt, double c0, double c00, double V, double r0, double p0, double r00, double p00)
{
    return (rdt * V) * (((c0 * r0) * p0) - ((c00 * r00) * p00));
}
// fvm::ddt / fvc::ddt / the ddt0 update, CrankNicolson: every operator rounded on its own (DESIGN 3.5g).  cr = rDtCoef*rho_value (a host
// product) or rDtCoef*rho0 of the cell; offd = cn_off(ddt0)
__device__ __forceinline__ double cn_off(int offc, double oc, double x) { return offc ? oc * x : x; }
__device__ __forceinline__ double cn_source(double cr, double p0, double offd, double V) { return ((cr * p0) + offd) * V; }
// CORR: each own face's t_r = faceFlux*(scale*corr_r) is formed once in the face pass and staged in LDS after lB / uB / uL; every cell
// forms its n_rhs surfaceIntegrate row sums in mi_surface_integrate's order, ivf = sum/V, and subtracts the rounded V*ivf from the source
// right after the ddt part (the div matrix's own source, fvMatrix.C:1819-1826), before the explicit terms
template <bool DIV, bool LAP, int BS, bool R16, bool CORR = false, int TF = TF_EULER>
__global__ __launch_bounds__(BS) void k_row_assemble(const typename AsmSel<CORR, TF>::type a)
{
    constexpr bool BACK = TF == TF_BACK, CN = TF == TF_CN, LOCAL = TF == TF_LOCAL;
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    const int lb = a.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.blockStart) { c0 = a.blockStart[lb]; cEnd = a.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.os[c0], nf = a.os[cEnd] - f0;
    const bool staged = nf <= a.cap;
    double* sLB = rp_smem;                               // DIV: lB, uB; LAP: uL
    double* sUB = rp_smem + a.cap;
    double* sUL = rp_smem + (DIV ? 2 : 0) * a.cap;
    double* sT = rp_smem + ((DIV ? 2 : 0) + (LAP ? 1 : 0)) * a.cap;   // CORR: t_r at sT[r * cap + j]
    const bool mag = a.sumMagOut != nullptr;
    struct FaceC { double lB, uB, uL; };
    auto face = [&](int f) -> FaceC {
        FaceC r{0.0, 0.0, 0.0};
        if (DIV) { const double v = a.flux[f]; const double u = a.w ? a.w[f] : (v >= 0 ? 1.0 : 0.0); r.lB = -u * v; r.uB = r.lB + v; }
        if (LAP) r.uL = a.delta[f] * a.gam[f];
        return r;
    };
    auto lowerF = [&](const FaceC& r) -> double { return DIV ? (LAP ? r.lB - r.uL : r.lB) : -r.uL; };
    auto upperF = [&](const FaceC& r) -> double { return DIV ? (LAP ? r.uB - r.uL : r.uB) : -r.uL; };
#pragma unroll 2
    for (int j = tid; j < nf; j += BS) {                 // the face pass over the block's own faces: coalesced, every face written once
        const FaceC r = face(f0 + j);
        if (a.lowerOut) a.lowerOut[f0 + j] = lowerF(r);
        a.upperOut[f0 + j] = upperF(r);
        if (staged) { if (DIV) { sLB[j] = r.lB; sUB[j] = r.uB; } if (LAP) sUL[j] = r.uL; }
    }
    if constexpr (CORR) if (staged) {                    // a loop of its own: fewer pointers live at once (no SGPR spills)
        for (int j = tid; j < nf; j += BS) {
            double t[4]; lu_face(a.corr, a.nRhs, a.lo, a.up, a.flux, f0 + j, t);
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < a.nRhs) sT[q * a.cap + j] = t[q];
        }
    }
    int nb = 0, ne = 0, ob = 0, oe = 0;
    const int escBase = R16 ? a.escStart[lb] : 0;
    if (live) {
        if (R16) {
            const uint32_t w1 = a.row16[c], w0 = tid ? a.row16[c - 1] : 0u;
            const int lsBase = a.ls[c0];
            ob = f0 + (int)(w0 & 0xFFFFu); oe = f0 + (int)(w1 & 0xFFFFu); nb = lsBase + (int)(w0 >> 16); ne = lsBase + (int)(w1 >> 16);
        } else { nb = a.ls[c]; ne = a.ls[c + 1]; ob = a.os[c]; oe = a.os[c + 1]; }
    }
    auto nei_face = [&](int j) -> int {
        if (!R16) return a.losort[j];
        const unsigned e = a.losort16[j];
        return (e & 0x8000u) ? a.esc[escBase + (int)(e & 0x7FFFu)] : f0 + (int)e;
    };
    // CORR: a face's t_r from LDS when the block staged it, else recomputed from the inputs (the cut faces after the barrier)
    double sumC[4] = {0.0, 0.0, 0.0, 0.0};
    auto corr_add = [&](int f, bool own) {
        if constexpr (CORR) {
            double t[4];
            if (staged && f >= f0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (q < a.nRhs) t[q] = sT[q * a.cap + f - f0];
            } else lu_face(a.corr, a.nRhs, a.lo, a.up, a.flux, f, t);
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < a.nRhs) sumC[q] += own ? t[q] : -t[q];
        }
    };
    // cut neighbour-side faces are recomputed from the schemes' inputs (same roundings) before the barrier
    const int cnt = ne - nb;
    int nfk[3]; FaceC nv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nfk[k] = (k < cnt) ? nei_face(nb + k) : 0;
        nv[k] = (k < cnt && (!staged || nfk[k] < f0)) ? face(nfk[k]) : FaceC{0.0, 0.0, 0.0};
    }
    __syncthreads();
    if (!live) return;
    double sumB = 0.0, sumL = 0.0, sumM = 0.0;
    for (int j = ob; j < oe; ++j) {
        FaceC r;
        if (staged) { const int q = j - f0; r.lB = DIV ? sLB[q] : 0.0; r.uB = DIV ? sUB[q] : 0.0; r.uL = LAP ? sUL[q] : 0.0; } else r = face(j);
        if (DIV) sumB += -r.lB;
        if (LAP) sumL += -r.uL;
        if (mag) sumM += fabs(upperF(r));
    }
    auto nei_term = [&](const FaceC& r) { if (DIV) sumB += -r.uB; if (LAP) sumL += -r.uL; if (mag) sumM += fabs(lowerF(r)); };
    auto nei_get = [&](int f) -> FaceC {
        if (staged && f >= f0) { const int q = f - f0; return FaceC{DIV ? sLB[q] : 0.0, DIV ? sUB[q] : 0.0, LAP ? sUL[q] : 0.0}; }
        return face(f);
    };
#pragma unroll
    for (int k = 0; k < 3; ++k) if (k < cnt) nei_term((staged && nfk[k] >= f0) ? nei_get(nfk[k]) : nv[k]);
    for (int j = nb + 3; j < ne; ++j) nei_term(nei_get(nei_face(j)));
    const double V = a.vol ? a.vol[c] : 0.0;
    double rdt = a.rdt;
    if constexpr (LOCAL) {
        if (a.loc.rdt) rdt = a.loc.rdt[c];
        if (DIV && a.loc.divPhi) { const double t = V * a.loc.divPhi[c]; sumB = sumB - t; }
    }
    double d = 0.0;
    if constexpr (BACK) { const double dA = back_diag(a.bw.cA, a.rho ? a.rho[c] : a.rhoValue, V); d = DIV ? dA + sumB : dA; }
    else if (CN || a.ddt) { const double dA = (rdt * (a.rho ? a.rho[c] : a.rhoValue)) * V; d = DIV ? dA + sumB : dA; }
    else if (DIV) d = sumB;
    if (LAP) d = (BACK || CN || a.ddt || DIV) ? d - sumL : -sumL;
    if (a.sp) { const double t = V * a.sp[c]; d = a.spMinus ? d - t : d + t; }
    a.diagOut[c] = d;
    if (mag) a.sumMagOut[c] = sumM;
    auto source = [&](int r, double vIvf) {
        double s;
        if constexpr (BACK)
            s = a.rhoOld ? back_source_rho(a.rdt, a.bw.c0, a.bw.c00, V, a.rhoOld[c], a.psiOld[r][c], a.bw.rhoOldOld[c], a.bw.psiOldOld[r][c])
                         : back_source(a.rdt, a.rhoValue, a.bw.c0, a.bw.c00, V, a.psiOld[r][c], a.bw.psiOldOld[r][c]);
        else if constexpr (CN) s = cn_source(rdt * (a.rhoOld ? a.rhoOld[c] : a.rhoValue), a.psiOld[r][c], cn_off(a.cn.offc, a.cn.oc, a.cn.ddt0[r][c]), V);
        else s = a.ddt ? ((rdt * (a.rhoOld ? a.rhoOld[c] : a.rhoValue)) * a.psiOld[r][c]) * V : 0.0;
        if (CORR) s = s - vIvf;
        for (int k = 0; k < a.nSu; ++k) { const double t = V * a.su[k * a.nRhs + r][c]; s = a.suMinus[k] ? s + t : s - t; }
        a.sourceOut[r][c] = s;
    };
    if constexpr (CORR) {   // the surfaceIntegrate row sums after the matrix's: own faces ascending, then losort order (as mi_surface_integrate)
        for (int j = ob; j < oe; ++j) corr_add(j, true);
        for (int j = nb; j < ne; ++j) corr_add(nei_face(j), false);
#pragma unroll
        for (int r = 0; r < 4; ++r) if (r < a.nRhs) { const double ivf = sumC[r] / V; source(r, V * ivf); }
    } else for (int r = 0; r < a.nRhs; ++r) source(r, 0.0);
}

// linear-type face interpolation (surfaceInterpolationScheme.C:337-352)
__global__ void k_face_interpolate(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const double* __restrict__ lambda,
                                   const double* __restrict__ phi, double* __restrict__ sf, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) { // grid-stride: measured faster here than per-block chunks (152 vs 162 us)
        const double pn = phi[up[f]];
        sf[f] = fma(lambda[f], phi[lo[f]] - pn, pn);
    }
}

// gaussConvectionScheme::flux (gaussConvectionScheme.C:62-70): faceFlux * interpolate(faceFlux, vf) on the internal faces -- the interpolate one
// fma (surfaceInterpolationScheme.C:273-279, weights w or pos(faceFlux) for upwind), the product a separate field operation (rounded)
__global__ void k_face_conv_flux(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const double* __restrict__ w, const double* __restrict__ flux,
                                 const double* __restrict__ vf, double* __restrict__ out, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        const double fl = flux[f], pn = vf[up[f]];
        const double l = w ? w[f] : (fl >= 0 ? 1.0 : 0.0);
        const double itp = fma(l, vf[lo[f]] - pn, pn);
        out[f] = fl * itp;
    }
}

// non-orthogonal correction of the face gradient (correctedSnGrad.C:45-65 fullGradCorrection, gaussLaplacianSchemes.C:64-90):
//   flux[f] = gammaMagSf[f] * ( nonOrthCorrectionVectors[f] & linear.interpolate(grad(vf))[f] )
// The reference builds three fields one after the other (interpolated gradient, dot product, product with gammaMagSf); the
// values are rounded where its temporaries are, so one pass gives the same bits: interpolation lambda*(g[P]-g[N]) + g[N] as
// one fma per component (surfaceInterpolationScheme.C:275-280), a & b = ax*bx + ay*by + az*bz contracted left to right.
// (the two interpolate-and-dot forms are device functions: the limited passes below form exactly the same value)
__device__ __forceinline__ double sngrad_face_corr(int P, int N, double l, double cx, double cy, double cz, const double* __restrict__ gx,
                                                   const double* __restrict__ gy, const double* __restrict__ gz)
{
    const double nx = gx[N], ny = gy[N], nz = gz[N];
    const double fx = fma(l, gx[P] - nx, nx), fy = fma(l, gy[P] - ny, ny), fz = fma(l, gz[P] - nz, nz);
    return fma(cz, fz, fma(cx, fx, cy * fy));
}
__global__ void k_sngrad_corr_flux(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const double* __restrict__ cvx,
                                   const double* __restrict__ cvy, const double* __restrict__ cvz, const double* __restrict__ lambda,
                                   const double* __restrict__ gx, const double* __restrict__ gy, const double* __restrict__ gz,
                                   const double* __restrict__ gammaMagSf, double* __restrict__ flux, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        const double corr = sngrad_face_corr(lo[f], up[f], lambda[f], cvx[f], cvy[f], cvz[f], gx, gy, gz);
        flux[f] = gammaMagSf ? gammaMagSf[f] * corr : corr;
    }
}
// the same on a COUPLED patch (processor / cyclic): the interpolate is pLambda*patchInternalField + (1 - pLambda)*patchNeighbourField,
// written as separate field operations in the reference (surfaceInterpolationScheme.C:360-365), hence no contraction here
__device__ __forceinline__ double sngrad_patch_corr(int c, int i, double l, double cx, double cy, double cz, const double* __restrict__ gx,
                                                    const double* __restrict__ gy, const double* __restrict__ gz, const double* __restrict__ nx,
                                                    const double* __restrict__ ny, const double* __restrict__ nz)
{
    const double m = 1.0 - l;
    const double ax = l * gx[c], ay = l * gy[c], az = l * gz[c];
    const double bx = m * nx[i], by = m * ny[i], bz = m * nz[i];
    const double fx = ax + bx, fy = ay + by, fz = az + bz;
    return fma(cz, fz, fma(cx, fx, cy * fy));
}
__global__ void k_patch_sngrad_corr_flux(const int32_t* __restrict__ faceCells, const double* __restrict__ cvx, const double* __restrict__ cvy,
                                         const double* __restrict__ cvz, const double* __restrict__ w, const double* __restrict__ gx,
                                         const double* __restrict__ gy, const double* __restrict__ gz, const double* __restrict__ nx,
                                         const double* __restrict__ ny, const double* __restrict__ nz, const double* __restrict__ gammaMagSf,
                                         double* __restrict__ flux, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double corr = sngrad_patch_corr(faceCells[i], i, w[i], cvx[i], cvy[i], cvz[i], gx, gy, gz, nx, ny, nz);
    flux[i] = gammaMagSf ? gammaMagSf[i] * corr : corr;
}

// ---- the `limited` snGrad scheme (snGradSchemes/limitedSnGrad/limitedSnGrad.C:58-84): correction(vf) = limiter*corr with
//   corr    = correctedSnGrad::correction(vf)                       (per component, the value of the passes above)
//   limiter = min( k*mag(snGrad(vf)) / ((1 - k)*mag(corr) + SMALL), 1 )
// The reference runs about ten field passes with temporaries; here one face pass.  Every temporary is rounded where the reference
// rounds it: snGrad = nonOrthDeltaCoeffs*(vf[N] - vf[P]) (snGradScheme.C:103-108), mag = fabs (scalar) | sqrt(magSqr) with magSqr the
// engine's dot rule fma(z, z, fma(x, x, y*y)) (vector: ONE limiter from the magnitudes of the vector snGrad and the vector correction),
// the products, the sum with SMALL, the quotient and limiter*corr one operation each, then gammaMagSf*(limiter*corr)
// (gaussLaplacianSchemes.C:64-90).  min(q, 1) = (q < 1) ? q : 1 as Foam::min: a NaN quotient gives 1.  k = 0 and k = 1 take the same path.
template <int NCOMP>
struct SnGradLimArgs {
    const double *cvx, *cvy, *cvz, *lambda, *deltaCoeffs, *gammaMagSf;   // gammaMagSf may be null
    const double* vf[NCOMP];
    const double* g[3 * NCOMP];                                          // g[3*j + d] = d(vf_j)/dx_d
    double* flux[NCOMP];
    double* limiter;                                                     // may be null
    double k, oneMinusK;
    int n;
};
template <int NCOMP>
__device__ __forceinline__ double sngrad_limiter(double k, double oneMinusK, const double (&sn)[NCOMP], const double (&corr)[NCOMP])
{
    double magSn, magCorr;
    if constexpr (NCOMP == 1) { magSn = fabs(sn[0]); magCorr = fabs(corr[0]); }
    else {
        magSn = sqrt(fma(sn[2], sn[2], fma(sn[0], sn[0], sn[1] * sn[1])));
        magCorr = sqrt(fma(corr[2], corr[2], fma(corr[0], corr[0], corr[1] * corr[1])));
    }
    const double num = k * magSn;
    const double den = (oneMinusK * magCorr) + 1e-15;                    // + SMALL
    const double q = num / den;
    return (q < 1.0) ? q : 1.0;
}
template <int NCOMP>
__device__ __forceinline__ void sngrad_limited_store(const SnGradLimArgs<NCOMP>& a, int f, double lim, const double (&corr)[NCOMP])
{
    const bool scaled = a.gammaMagSf != nullptr;
    const double gm = scaled ? a.gammaMagSf[f] : 0.0;
#pragma unroll
    for (int j = 0; j < NCOMP; ++j) {
        const double lc = lim * corr[j];
        a.flux[j][f] = scaled ? gm * lc : lc;
    }
    if (a.limiter) a.limiter[f] = lim;
}
template <int NCOMP>
__global__ void k_sngrad_limited_flux(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const SnGradLimArgs<NCOMP> a)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < a.n; f += gridDim.x * blockDim.x) {
        const int P = lo[f], N = up[f];
        const double l = a.lambda[f], cx = a.cvx[f], cy = a.cvy[f], cz = a.cvz[f], dc = a.deltaCoeffs[f];
        double corr[NCOMP], sn[NCOMP];
#pragma unroll
        for (int j = 0; j < NCOMP; ++j) {
            corr[j] = sngrad_face_corr(P, N, l, cx, cy, cz, a.g[3 * j], a.g[3 * j + 1], a.g[3 * j + 2]);
            const double d = a.vf[j][N] - a.vf[j][P];
            sn[j] = dc * d;
        }
        sngrad_limited_store<NCOMP>(a, f, sngrad_limiter<NCOMP>(a.k, a.oneMinusK, sn, corr), corr);
    }
}
// COUPLED patch: corr as k_patch_sngrad_corr_flux forms it, snGrad = deltaCoeffs*(patchNeighbourField - patchInternalField)
// (snGradScheme.C:165-169, coupledFvPatchField::snGrad); g holds the cell gradients, nbrVf / nbrG the patchNeighbourFields
template <int NCOMP>
struct SnGradNbrArgs { const double* vf[NCOMP]; const double* g[3 * NCOMP]; };
template <int NCOMP>
__global__ void k_patch_sngrad_limited_flux(const int32_t* __restrict__ faceCells, const SnGradLimArgs<NCOMP> a, const SnGradNbrArgs<NCOMP> nbr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int c = faceCells[i];
    const double l = a.lambda[i], cx = a.cvx[i], cy = a.cvy[i], cz = a.cvz[i], dc = a.deltaCoeffs[i];
    double corr[NCOMP], sn[NCOMP];
#pragma unroll
    for (int j = 0; j < NCOMP; ++j) {
        corr[j] = sngrad_patch_corr(c, i, l, cx, cy, cz, a.g[3 * j], a.g[3 * j + 1], a.g[3 * j + 2], nbr.g[3 * j], nbr.g[3 * j + 1], nbr.g[3 * j + 2]);
        const double d = nbr.vf[j][i] - a.vf[j][c];
        sn[j] = dc * d;
    }
    sngrad_limited_store<NCOMP>(a, i, sngrad_limiter<NCOMP>(a.k, a.oneMinusK, sn, corr), corr);
}

// ---- fvc::div(nuEff*dev(T(fvc::grad(U)))) / fvc::div(muEff*dev2(T(fvc::grad(U)))): the explicit term of divDevReff / divDevRhoReff --
// (incompressible laminar.C:202-225, compressible laminar.C:197, eddyViscosity.C:132).  The reference forms four cell tensor fields
// (grad, T, dev, the product), interpolates nine components and contracts with Sf; here a face gathers the ten cell values (viscosity,
// g[3*j + k] = d(U_j)/dx_k) of each of its two cells ONCE, forms Y in registers and writes the three flux components.  Per cell, each
// operation rounded as the reference's cell fields round it:
//   tr = (g[0] + g[4]) + g[8]                    TensorI.H:465-468 (the transposition keeps the diagonal)
//   ii = coeff*tr                                SphericalTensor(coeff)*tr, coeff 1.0/3.0 (dev) | 2.0/3.0 (dev2): TensorI.H:534-546
//   X_kj = g[3*k + j] - (k == j ? ii : 0)        T(...), TensorI.H:699-707; off-diagonals untouched
//   Y_kj = visc*X_kj
// y[3*k + j] = Y_kj: the storage of g, because T(gradU)_kj = gradU_jk = d(U_k)/dx_j = g[3*k + j].
// Per face and component j: I_kj = fma(lambda, Y_kj[P] - Y_kj[N], Y_kj[N]) and flux_j = fma(I_zj, Sf_z, fma(I_xj, Sf_x, I_yj*Sf_y)) --
// flux_face with v = column j of X and the viscosity as its cell scale, operation for operation (`Vector & Tensor` contracted per
// column as `Vector & Vector` is: the standing assumption of DESIGN 3.5a, restated in 3.5f).
template <int KIND>
__device__ __forceinline__ void dev_tgrad_cell(double visc, const double (&g)[9], double (&y)[9])
{
    constexpr double coeff = KIND == MI_DEV ? 1.0 / 3.0 : 2.0 / 3.0;
    const double tr = (g[0] + g[4]) + g[8];
    const double ii = coeff * tr;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double x = (i % 4 == 0) ? g[i] - ii : g[i];
        y[i] = visc * x;
    }
}
// flux_j = Sf & column j of the face tensor t (t[3*k + j])
__device__ __forceinline__ double dev_tgrad_dot(const double (&t)[9], int j, double sx, double sy, double sz)
{
    return fma(t[6 + j], sz, fma(t[j], sx, t[3 + j] * sy));
}
struct DevTGradArgs {
    const int32_t *lo, *up;
    const double *lam, *s[3], *visc, *g[9];
    double* out[3];
    int nf, xcd;
};
// XCD-aware chunks as the other gathering face passes (k_limited_weights, k_ddt_phi_corr_backward)
template <int KIND>
__global__ void k_face_dev_tgrad_flux(const DevTGradArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        const double l = a.lam[f], sx = a.s[0][f], sy = a.s[1][f], sz = a.s[2][f];
        double gP[9], gN[9], yP[9], yN[9], t[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { gP[i] = a.g[i][P]; gN[i] = a.g[i][N]; }
        dev_tgrad_cell<KIND>(a.visc[P], gP, yP);
        dev_tgrad_cell<KIND>(a.visc[N], gN, yN);
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = fma(l, yP[i] - yN[i], yN[i]);
#pragma unroll
        for (int j = 0; j < 3; ++j) a.out[j][f] = dev_tgrad_dot(t, j, sx, sy, sz);
    }
}
// the same on one patch.  COUPLED (processor; cyclic without rotation): the cell side through faceCells from the cell arrays, the
// other side the caller's patchNeighbourFields (nine gradient arrays and the viscosity per patch face), Y formed on each side,
// I = (w*Y_P) + ((1 - w)*Y_N) uncontracted (separate field operations in the reference: sngrad_patch_corr's rule).  Not COUPLED: the
// patch's own boundary values visc_b and G_b (mi_patch_gauss_grad_correct), no interpolation.
struct PatchDevTGradArgs {
    const int32_t* fc;
    const double *w, *s[3], *visc, *g[9], *nvisc, *ng[9];
    double* out[3];
    int n;
};
template <int KIND, bool COUPLED>
__global__ void k_patch_dev_tgrad_flux(const PatchDevTGradArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int c = COUPLED ? a.fc[i] : i;
    double g[9], t[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) g[q] = a.g[q][c];
    dev_tgrad_cell<KIND>(a.visc[c], g, t);
    if (COUPLED) {
        double yN[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) g[q] = a.ng[q][i];
        dev_tgrad_cell<KIND>(a.nvisc[i], g, yN);
        const double l = a.w[i], m = 1.0 - l;
#pragma unroll
        for (int q = 0; q < 9; ++q) { const double p = l * t[q], n = m * yN[q]; t[q] = p + n; }
    }
    const double sx = a.s[0][i], sy = a.s[1][i], sz = a.s[2][i];
#pragma unroll
    for (int j = 0; j < 3; ++j) a.out[j][i] = dev_tgrad_dot(t, j, sx, sy, sz);
}
// gaussGrad::correctBoundaryConditions on a patch that is not coupled (gaussGrad.C:277-303):
//   gGradbf += n*(vsf.boundaryField().snGrad() - (n & gGradbf)),   n = Sf/magSf (each component rounded),
// gGradbf the zeroGradient value gGrad.correctBoundaryConditions() leaves = the cell gradient through faceCells.  Per component j
//   gb_k = g_k + n_k*(sn_j - fma(n_z, g_z, fma(n_x, g_x, n_y*g_y))):  product, difference and sum each rounded.
template <int NCOMP>
struct PatchGradCorrArgs {
    const int32_t* fc;
    const double *s[3], *magSf, *sn[NCOMP], *g[3 * NCOMP];
    double* out[3 * NCOMP];
    int n;
};
template <int NCOMP>
__global__ void k_patch_gauss_grad_correct(const PatchGradCorrArgs<NCOMP> a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int c = a.fc[i];
    const double m = a.magSf[i];
    const double nx = a.s[0][i] / m, ny = a.s[1][i] / m, nz = a.s[2][i] / m;
#pragma unroll
    for (int j = 0; j < NCOMP; ++j) {
        const double gx = a.g[3 * j][c], gy = a.g[3 * j + 1][c], gz = a.g[3 * j + 2][c];
        const double d = a.sn[j][i] - fma(nz, gz, fma(nx, gx, ny * gy));
        const double cx = nx * d, cy = ny * d, cz = nz * d;
        a.out[3 * j][i] = gx + cx; a.out[3 * j + 1][i] = gy + cy; a.out[3 * j + 2][i] = gz + cz;
    }
}
// fvPatchField::patchInternalField: out[i] = psi[faceCells[i]]
__global__ void k_patch_internal_field(const int32_t* __restrict__ faceCells, const double* __restrict__ psi, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = psi[faceCells[i]];
}
// inout -= x*y with the product rounded first (`source -= V*div(...)`: a temporary field, then operator-=)
__global__ __launch_bounds__(RB) void k_submul(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ io, int64_t n)
{
    cell_map<4>(n, {x, y, io}, {io}, [](const double (&v)[3], double (&o)[1]) { const double t = v[0] * v[1]; o[0] = v[2] - t; });
}

// patch contribution per unique patch cell, ascending patch-face order (fvMatrix.C:38-75,978-1085)
template <int FN, bool PROD = false>
__global__ void k_patch_add(const int32_t* __restrict__ cells, const int32_t* __restrict__ start, const int32_t* __restrict__ sort,
                            const double* __restrict__ pf, double* __restrict__ intf, int nU, const double* __restrict__ q = nullptr)
{
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nU; u += gridDim.x * blockDim.x) {
        const int c = cells[u];
        double out = intf[c];
        for (int k = start[u]; k < start[u + 1]; ++k) {
            if (PROD) { out = FN == 0 ? fma(pf[sort[k]], q[sort[k]], out) : fma(-pf[sort[k]], q[sort[k]], out); continue; } // out += cmptMultiply(pbc, pnf) inside fvMatrixAddBoundarySourceFunctor (fvMatrix.C:245-286): one fma
            const double v = pf[sort[k]];
            out += FN == 0 ? v : FN == 1 ? -v : fabs(v);
        }
        intf[c] = out;
    }
}

// cell = max(cell, patch face values) per unique patch cell (matrixPatchOperation with maxOp: CoEulerDdtScheme.C:99-114); (a > b) ? a : b
__global__ void k_patch_max(const int32_t* __restrict__ cells, const int32_t* __restrict__ start, const int32_t* __restrict__ sort,
                            const double* __restrict__ pf, double* __restrict__ intf, int nU)
{
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nU; u += gridDim.x * blockDim.x) {
        const int c = cells[u];
        double out = intf[c];
        for (int k = start[u]; k < start[u + 1]; ++k) { const double v = pf[sort[k]]; out = v > out ? v : out; }
        intf[c] = out;
    }
}

__global__ __launch_bounds__(RB) void k_relax_dominance(double* __restrict__ D, const double* __restrict__ sumOff, double alpha, int64_t n)
{
    cell_map<4>(n, {D, sumOff}, {D}, [&](const double (&v)[2], double (&o)[1]) { o[0] = fmax(fabs(v[0]), v[1]) / alpha; });
}
__global__ __launch_bounds__(RB) void k_relax_source(double* __restrict__ S, const double* __restrict__ D, const double* __restrict__ D0,
                                                     const double* __restrict__ psi, int64_t n)
{
    cell_map<4>(n, {D, D0, psi, S}, {S}, [](const double (&v)[4], double (&o)[1]) {
        const auto& [d, d0, p, s] = v;
        o[0] = s + (d - d0) * p;                             // S += (D - D0)*psi: three field operations (fvMatrix.C:1344), three roundings
    });
}

// fvm::ddt, Euler (EulerDdtScheme.C fvmDdt): diag = rDeltaT*rho*V, source = rDeltaT*rho*psi0*V
__global__ __launch_bounds__(RB) void k_ddt_euler(double rr, const double* __restrict__ vol, const double* __restrict__ psi0,
                                                  double* __restrict__ diag, double* __restrict__ source, int64_t n)
{
    cell_map<4>(n, {vol, psi0}, {diag, source}, [&](const double (&x)[2], double (&o)[2]) {
        const auto& [v, p] = x;
        o[0] = rr * v; o[1] = (rr * p) * v;
    });
}
// fvm::ddt(rho, vf) with a density FIELD (EulerDdtScheme.C:403-440): diag = rDeltaT*rho*V, source = rDeltaT*rho0*psi0*V
__global__ __launch_bounds__(RB) void k_ddt_euler_rho(double r, const double* __restrict__ rho, const double* __restrict__ rho0, const double* __restrict__ vol,
                                                      const double* __restrict__ psi0, double* __restrict__ diag, double* __restrict__ source, int64_t n)
{
    cell_map<4>(n, {rho, rho0, vol, psi0}, {diag, source}, [&](const double (&x)[4], double (&o)[2]) {
        const auto& [q, q0, v, p] = x;
        o[0] = (r * q) * v; o[1] = ((r * q0) * p) * v;
    });
}
// fvm::Su / fvm::Sp / fvm::SuSp (fvmSup.C:34-54, 100-170, 190-214); the product with V is rounded before it is added
__global__ __launch_bounds__(RB) void k_fvm_su(const double* __restrict__ vol, const double* __restrict__ su, double* __restrict__ source, int64_t n)
{
    cell_map<4>(n, {vol, su, source}, {source}, [](const double (&x)[3], double (&o)[1]) { o[0] = x[2] - x[0] * x[1]; });
}
__global__ __launch_bounds__(RB) void k_fvm_sp(const double* __restrict__ vol, const double* __restrict__ sp, double spValue, double* __restrict__ diag, int64_t n)
{
    if (sp) cell_map<4>(n, {vol, sp, diag}, {diag}, [](const double (&x)[3], double (&o)[1]) { o[0] = x[2] + x[0] * x[1]; });
    else cell_map<4>(n, {vol, diag}, {diag}, [&](const double (&x)[2], double (&o)[1]) { o[0] = x[1] + x[0] * spValue; });
}
__global__ __launch_bounds__(RB) void k_fvm_susp(const double* __restrict__ vol, const double* __restrict__ susp, const double* __restrict__ vf,
                                                 double* __restrict__ diag, double* __restrict__ source, int64_t n)
{
    cell_map<4>(n, {vol, susp, vf, diag, source}, {diag, source}, [](const double (&x)[5], double (&o)[2]) {
        const auto& [v, q, f, d, s] = x;
        const double mx = q > 0 ? q : 0.0, mn = q < 0 ? q : 0.0;
        o[0] = d + v * mx; o[1] = s - (v * mn) * f;
    });
}
// phi = Sf & interpolate([sc *] V) [+ addA [* addB]] as a plain face pass (mi_flux_div's default form: this pass + the row sum of
// fvc::surfaceIntegrate; measured faster than the one-row-pass form of round 5, whose cut faces each cost eight scattered gathers; that form was removed in round 6)
__global__ void k_face_flux(const RowPassArgs a, double* __restrict__ out, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) out[f] = flux_face(a, f);
}
// fvcDdtPhiCoeff (ddtScheme.C:139-174): 1 - min(|phiCorr| / (|phi0| + SMALL), 1), min(q, 1) = (q < 1) ? q : 1
__device__ __forceinline__ double ddt_phi_coeff(double phi0, double phiCorr)
{
    const double q = fabs(phiCorr) / (fabs(phi0) + 1e-15);
    return 1.0 - (q < 1.0 ? q : 1.0);
}
// fvc::ddtCorr(rho, U, phi), Euler, internal faces (EulerDdtScheme.C:663-720 / :523-551; fvcDdtPhiCoeff: ddtScheme.C:139-174) in ONE
// face pass (the reference: rhoU0, three interpolates, the dot product, phiCorr, the coefficient's five field operations, two products)
__global__ void k_ddt_phi_corr(const RowPassArgs a, double rDeltaT, const double* __restrict__ phi0, double* __restrict__ out, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        const double p0 = phi0[f];
        const double phiCorr = p0 - flux_face(a, f);
        out[f] = (ddt_phi_coeff(p0, phiCorr) * rDeltaT) * phiCorr;
    }
}
// fvm::ddt, backward (backwardDdtScheme.C:456-607, static mesh): the constant-density form (rho_value 1: fvm::ddt(vf)) and the density-field
// form; the roundings are back_diag / back_source[_rho]'s
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvm_ddt_backward(double rdt, double cA, double c0, double c00, double rhoValue, const double* __restrict__ rho,
                                                         const double* __restrict__ rho0, const double* __restrict__ rho00, const double* __restrict__ vol,
                                                         const double* __restrict__ psi0, const double* __restrict__ psi00, double* __restrict__ diag,
                                                         double* __restrict__ source, int64_t n)
{
    if (RHO) cell_map<2>(n, {vol, psi0, psi00, rho, rho0, rho00}, {diag, source}, [&](const double (&x)[6], double (&o)[2]) {
        const auto& [v, p0, p00, q, q0, q00] = x;
        o[0] = back_diag(cA, q, v); o[1] = back_source_rho(rdt, c0, c00, v, q0, p0, q00, p00);
    });
    else cell_map<2>(n, {vol, psi0, psi00}, {diag, source}, [&](const double (&x)[3], double (&o)[2]) {
        const auto& [v, p0, p00] = x;
        o[0] = back_diag(cA, rhoValue, v); o[1] = back_source(rdt, rhoValue, c0, c00, v, p0, p00);
    });
}
// fvc::ddt, backward (backwardDdtScheme.C:196-207, :268-280, :343-355): rr = rDeltaT*rho_value (a host product) without a density field
__device__ __forceinline__ double back_fvc(double rr, double c, double c0, double c00, double f, double f0, double f00)
{
    return rr * (((c * f) - (c0 * f0)) + (c00 * f00));
}
__device__ __forceinline__ double back_fvc_rho(double rdt, double c, double c0, double c00, double r, double f, double r0, double f0, double r00, double f00)
{
    return rdt * ((((c * r) * f) - ((c0 * r0) * f0)) + ((c00 * r00) * f00));
}
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvc_ddt_backward(double rr, double c, double c0, double c00, const double* __restrict__ rho,
                                                         const double* __restrict__ rho0, const double* __restrict__ rho00, const double* __restrict__ vf,
                                                         const double* __restrict__ vf0, const double* __restrict__ vf00, double* __restrict__ out, int64_t n)
{
    if (RHO) cell_map<2>(n, {vf, vf0, vf00, rho, rho0, rho00}, {out}, [&](const double (&x)[6], double (&o)[1]) {
        const auto& [f, f0, f00, q, q0, q00] = x;
        o[0] = back_fvc_rho(rr, c, c0, c00, q, f, q0, f0, q00, f00);
    });
    else cell_map<2>(n, {vf, vf0, vf00}, {out}, [&](const double (&x)[3], double (&o)[1]) { o[0] = back_fvc(rr, c, c0, c00, x[0], x[1], x[2]); });
}
// ---- CrankNicolson (CrankNicolsonDdtScheme.C, static mesh; DESIGN 3.5g) ----
// the ddt0 update (:417-418, :507-508, :603-607; the same statements in fvmDdt :818-822, :900-904, :987-994): c0 = rDtCoef0*rho_value (a host
// product) without a density field
__device__ __forceinline__ double cn_ddt0(double c0, double p0, double p00, double offd) { return (c0 * (p0 - p00)) - offd; }
__device__ __forceinline__ double cn_ddt0_rho(double rdt0, double r0, double p0, double r00, double p00, double offd)
{
    return (rdt0 * ((r0 * p0) - (r00 * p00))) - offd;
}
// up to four fields (the components of a vector) in ONE launch, in place: element i of ddt0[k] is read and written by the same thread only.
// The field pointers travel in one by-value block and are indexed by compile-time constants (the unrolled k), so they stay in SGPRs.
struct CnUpdateArgs {
    double* ddt0[4]; const double *psi0[4], *psi00[4];
    const double *rho0, *rho00;
    double c0, oc; int offc, nFields; int64_t n;
};
template <bool RHO>
__global__ __launch_bounds__(RB) void k_ddt_cn_update(const CnUpdateArgs a)
{
    auto one = [&](double r0, double p0, double r00, double p00, double d) {
        const double offd = cn_off(a.offc, a.oc, d);
        return RHO ? cn_ddt0_rho(a.c0, r0, p0, r00, p00, offd) : cn_ddt0(a.c0, p0, p00, offd);
    };
    chunk_loop2(a.n, [&](int64_t i) {
            double2 q0 = make_double2(0.0, 0.0), q00 = q0;
            if (RHO) { q0 = ld2(a.rho0, i); q00 = ld2(a.rho00, i); }
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < a.nFields) {
                const double2 p0 = ld2(a.psi0[k], i), p00 = ld2(a.psi00[k], i), d = ld2(a.ddt0[k], i);
                st2(a.ddt0[k], i, make_double2(one(q0.x, p0.x, q00.x, p00.x, d.x), one(q0.y, p0.y, q00.y, p00.y, d.y)));
            }
        },
        [&](int64_t i) {
            const double r0 = RHO ? a.rho0[i] : 0.0, r00 = RHO ? a.rho00[i] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < a.nFields) a.ddt0[k][i] = one(r0, a.psi0[k][i], r00, a.psi00[k][i], a.ddt0[k][i]);
        });
}
// fvm::ddt (:755-832, :837-913, :919-1003): diag = (rDtCoef*rho)*V (Euler's with rDtCoef); source = cn_source.  cr = rDtCoef*rho_value
// (a host product) without a density field, else rdt = rDtCoef
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvm_ddt_cn(double rdt, double cr, double oc, int offc, const double* __restrict__ rho, const double* __restrict__ rho0,
                                                   const double* __restrict__ vol, const double* __restrict__ psi0, const double* __restrict__ ddt0,
                                                   double* __restrict__ diag, double* __restrict__ source, int64_t n)
{
    if (RHO) cell_map<2>(n, {vol, psi0, ddt0, rho, rho0}, {diag, source}, [&](const double (&x)[5], double (&o)[2]) {
        const auto& [v, p0, d, q, q0] = x;
        o[0] = (rdt * q) * v; o[1] = cn_source(rdt * q0, p0, cn_off(offc, oc, d), v);
    });
    else cell_map<2>(n, {vol, psi0, ddt0}, {diag, source}, [&](const double (&x)[3], double (&o)[2]) {
        const auto& [v, p0, d] = x;
        o[0] = cr * v; o[1] = cn_source(cr, p0, cn_off(offc, oc, d), v);
    });
}
// fvc::ddt (:426, :516, :615-616)
__device__ __forceinline__ double cn_fvc(double cr, double f, double f0, double offd) { return (cr * (f - f0)) - offd; }
__device__ __forceinline__ double cn_fvc_rho(double rdt, double r, double f, double r0, double f0, double offd) { return (rdt * ((r * f) - (r0 * f0))) - offd; }
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvc_ddt_cn(double cr, double oc, int offc, const double* __restrict__ rho, const double* __restrict__ rho0,
                                                   const double* __restrict__ vf, const double* __restrict__ vf0, const double* __restrict__ ddt0,
                                                   double* __restrict__ out, int64_t n)
{
    if (RHO) cell_map<2>(n, {vf, vf0, ddt0, rho, rho0}, {out}, [&](const double (&x)[5], double (&o)[1]) {
        const auto& [f, f0, d, q, q0] = x;
        o[0] = cn_fvc_rho(cr, q, f, q0, f0, cn_off(offc, oc, d));
    });
    else cell_map<2>(n, {vf, vf0, ddt0}, {out}, [&](const double (&x)[3], double (&o)[1]) { o[0] = cn_fvc(cr, x[0], x[1], cn_off(offc, oc, x[2])); });
}
// fvc::ddtCorr, backward, internal faces (backwardDdtScheme.C:724-765, :868-950 first branch; fvcDdtPhiCoeff: ddtScheme.C:139-174) in ONE face
// pass: a face gathers U0, U00 [rho0, rho00] of its two cells once and forms both fluxes from them -- flux(U0) for the coefficient (the OLD
// fields only) and flux(W), W = coefft0*U0 - coefft00*U00 rounded per cell and component as the cell field it is in the reference; each flux
// is flux_face's, operation for operation.  XCD-aware chunks as the gathering face passes (k_limited_weights, k_linear_upwind_corr).
struct DdtCorrBackArgs {
    const int32_t *lo, *up;
    const double *lam, *s[3], *u0[3], *u00[3], *rho0, *rho00, *phi0, *phi00;
    double* out;
    double rdt, c0, c00;
    int nf, xcd;
};
__global__ void k_ddt_phi_corr_backward(const DdtCorrBackArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        const double l = a.lam[f];
        double p[3], n[3], pp[3], nn[3], wP[3], wN[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) { p[d] = a.u0[d][P]; n[d] = a.u0[d][N]; pp[d] = a.u00[d][P]; nn[d] = a.u00[d][N]; }
        if (a.rho0) {
            const double rP = a.rho0[P], rN = a.rho0[N], rrP = a.rho00[P], rrN = a.rho00[N];
#pragma unroll
            for (int d = 0; d < 3; ++d) { p[d] = rP * p[d]; n[d] = rN * n[d]; pp[d] = rrP * pp[d]; nn[d] = rrN * nn[d]; }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) { wP[d] = (a.c0 * p[d]) - (a.c00 * pp[d]); wN[d] = (a.c0 * n[d]) - (a.c00 * nn[d]); }
        const double sx = a.s[0][f], sy = a.s[1][f], sz = a.s[2][f];
        auto flux = [&](const double* o, const double* q) {
            const double ix = fma(l, o[0] - q[0], q[0]), iy = fma(l, o[1] - q[1], q[1]), iz = fma(l, o[2] - q[2], q[2]);
            return fma(iz, sz, fma(ix, sx, iy * sy));
        };
        const double fU = flux(p, n), fW = flux(wP, wN);
        const double p0 = a.phi0[f];
        a.out[f] = (ddt_phi_coeff(p0, p0 - fU) * a.rdt) * (((a.c0 * p0) - (a.c00 * a.phi00[f])) - fW);
    }
}
// ---- the local-time-step schemes localEuler and CoEuler (localEulerDdtScheme.C, CoEulerDdtScheme.C, static mesh; DESIGN 3.5h) ----
// fvm::ddt (localEulerDdtScheme.C:339-445): Euler's expressions with rDeltaT a cell field -- diag = (r*rho)*V, source = ((r*rho0)*psi0)*V;
// without a density field rho = rho0 = rhoValue (1: the plain form, r*1 is exact)
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvm_ddt_local(const double* __restrict__ rD, double rhoValue, const double* __restrict__ rho, const double* __restrict__ rho0,
                                                      const double* __restrict__ vol, const double* __restrict__ psi0, double* __restrict__ diag,
                                                      double* __restrict__ source, int64_t n)
{
    auto one = [](double r, double v, double p0, double q, double q0, double (&o)[2]) { o[0] = (r * q) * v; o[1] = ((r * q0) * p0) * v; };
    if (RHO) cell_map<2>(n, {rD, vol, psi0, rho, rho0}, {diag, source}, [&](const double (&x)[5], double (&o)[2]) { one(x[0], x[1], x[2], x[3], x[4], o); });
    else cell_map<2>(n, {rD, vol, psi0}, {diag, source}, [&](const double (&x)[3], double (&o)[2]) { one(x[0], x[1], x[2], rhoValue, rhoValue, o); });
}
// fvc::ddt (:149-157, :200-209, :255-264): (r*rhoValue)*(vf - vf0), or r*((rho*vf) - (rho0*vf0)) with a density field
template <bool RHO>
__global__ __launch_bounds__(RB) void k_fvc_ddt_local(const double* __restrict__ rD, double rhoValue, const double* __restrict__ rho, const double* __restrict__ rho0,
                                                      const double* __restrict__ vf, const double* __restrict__ vf0, double* __restrict__ out, int64_t n)
{
    if (RHO) cell_map<2>(n, {rD, vf, vf0, rho, rho0}, {out}, [](const double (&x)[5], double (&o)[1]) {
        const auto& [r, f, f0, q, q0] = x;
        o[0] = r * ((q * f) - (q0 * f0));
    });
    else cell_map<2>(n, {rD, vf, vf0}, {out}, [&](const double (&x)[3], double (&o)[1]) { o[0] = (x[0] * rhoValue) * (x[1] - x[2]); });
}
// fvc::ddtCorr(U, phi) (:531-560): k_ddt_phi_corr with rDeltaT := fvc::interpolate(rDeltaT) on the face, one fma (surfaceInterpolationScheme.C:275-280)
__global__ void k_ddt_phi_corr_local(const RowPassArgs a, const double* __restrict__ rD, const double* __restrict__ phi0, double* __restrict__ out, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        const double p0 = phi0[f];
        const double phiCorr = p0 - flux_face(a, f);
        const double rn = rD[a.up[f]];
        const double rf = fma(a.a0[f], rD[a.lo[f]] - rn, rn);
        out[f] = (ddt_phi_coeff(p0, phiCorr) * rf) * phiCorr;
    }
}
// CoEulerDdtScheme::CofrDeltaT on one face (CoEulerDdtScheme.C:125-167), every field operator rounded on its own:
//   Co = (deltaCoeffs*(|phi|/magSf))*deltaT  [mass flux: |phi|/(rho_f*magSf)];  x = max(Co/maxCo, 1)/deltaT,  max(a, b) = (a > b) ? a : b
__device__ __forceinline__ double co_face_x(double dc, double phi, double magSf, bool mass, double rhoF, double deltaT, double maxCo)
{
    const double den = mass ? rhoF * magSf : magSf;
    const double co = (dc * (fabs(phi) / den)) * deltaT;
    const double q = co / maxCo;
    return (q > 1.0 ? q : 1.0) / deltaT;
}
// ... as a streaming pass over n faces (a patch's): rhoF null: volumetric flux
__global__ __launch_bounds__(RB) void k_co_face_r_delta_t(const double* __restrict__ dc, const double* __restrict__ magSf, const double* __restrict__ phi,
                                                          const double* __restrict__ rhoF, double deltaT, double maxCo, double* __restrict__ out, int64_t n)
{
    if (rhoF) cell_map<2>(n, {dc, magSf, phi, rhoF}, {out}, [&](const double (&x)[4], double (&o)[1]) { o[0] = co_face_x(x[0], x[2], x[1], true, x[3], deltaT, maxCo); });
    else cell_map<2>(n, {dc, magSf, phi}, {out}, [&](const double (&x)[3], double (&o)[1]) { o[0] = co_face_x(x[0], x[2], x[1], false, 0.0, deltaT, maxCo); });
}
// CoEulerDdtScheme::CorDeltaT on the internal faces (:61-94: matrixOperation with maxOp from 0.0, own faces then neighbour-side faces) in ONE
// row pass on k_row_pass's skeleton: a block forms x_f of its own faces once and stages them in LDS, cut neighbour-side faces are recomputed
// from the inputs before the barrier, every cell takes its max; no face array is written (the reference: about six face passes, the
// temporaries and the row gather).  Mass flux (rho given): rho_f = fvc::interpolate(rho.oldTime()) gathered at the face's two cells.
struct CoArgs {
    const uint32_t* row16; const uint16_t* losort16; const int32_t *esc, *escStart;
    const int32_t *os, *ls, *losort, *blockStart;
    int n, cap, xcd;
    const double *delta, *magSf, *phi, *lam, *rho;   // lam, rho null: volumetric flux
    const int32_t *lo, *up;                           // caller-order face addressing (read with rho)
    double deltaT, maxCo;
    double* out;
};
template <int BS, bool R16>
__global__ __launch_bounds__(BS) void k_co_r_delta_t(const CoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    const int lb = a.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.blockStart) { c0 = a.blockStart[lb]; cEnd = a.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.os[c0], nf = a.os[cEnd] - f0;
    const bool staged = nf <= a.cap;
    const bool mass = a.rho != nullptr;
    double* sX = rp_smem;
    auto face = [&](int f) -> double {
        double rhoF = 0.0;
        if (mass) { const double rn = a.rho[a.up[f]]; rhoF = fma(a.lam[f], a.rho[a.lo[f]] - rn, rn); }
        return co_face_x(a.delta[f], a.phi[f], a.magSf[f], mass, rhoF, a.deltaT, a.maxCo);
    };
    if (staged)
        for (int j = tid; j < nf; j += BS) sX[j] = face(f0 + j);
    int nb = 0, ne = 0, ob = 0, oe = 0;
    const int escBase = R16 ? a.escStart[lb] : 0;
    if (live) {
        if (R16) {
            const uint32_t w1 = a.row16[c], w0 = tid ? a.row16[c - 1] : 0u;
            const int lsBase = a.ls[c0];
            ob = f0 + (int)(w0 & 0xFFFFu); oe = f0 + (int)(w1 & 0xFFFFu); nb = lsBase + (int)(w0 >> 16); ne = lsBase + (int)(w1 >> 16);
        } else { nb = a.ls[c]; ne = a.ls[c + 1]; ob = a.os[c]; oe = a.os[c + 1]; }
    }
    auto nei_face = [&](int j) -> int {
        if (!R16) return a.losort[j];
        const unsigned e = a.losort16[j];
        return (e & 0x8000u) ? a.esc[escBase + (int)(e & 0x7FFFu)] : f0 + (int)e;
    };
    // cut neighbour-side faces are recomputed from the inputs (same roundings) before the barrier
    const int cnt = ne - nb;
    int nfk[3]; double nv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nfk[k] = (k < cnt) ? nei_face(nb + k) : 0;
        nv[k] = (k < cnt && (!staged || nfk[k] < f0)) ? face(nfk[k]) : 0.0;
    }
    __syncthreads();
    if (!live) return;
    double acc = 0.0;
    auto take = [&](double x) { acc = x > acc ? x : acc; };
    for (int j = ob; j < oe; ++j) take(staged ? sX[j - f0] : face(j));
#pragma unroll
    for (int k = 0; k < 3; ++k) if (k < cnt) take((staged && nfk[k] >= f0) ? sX[nfk[k] - f0] : nv[k]);
    for (int j = nb + 3; j < ne; ++j) { const int f = nei_face(j); take((staged && f >= f0) ? sX[f - f0] : face(f)); }
    a.out[c] = acc;
}
__global__ __launch_bounds__(RB) void k_upwind_weights(const double* __restrict__ flux, double* __restrict__ w, int64_t n)
{
    cell_map<4>(n, {flux}, {w}, [](const double (&f)[1], double (&o)[1]) { o[0] = f[0] >= 0 ? 1.0 : 0.0; });
}
// limitedLinear(k): NVDTVD.H r(), limitedLinear.H:79-97, limitedSurfaceInterpolationScheme.C:177-187 in ONE face pass
// (the reference: grad field, limiter transform with seven gathers, weights transform)
__global__ void k_limited_linear_weights(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, double twoByk,
                                         const double* __restrict__ cdw, const double* __restrict__ flux, const double* __restrict__ phi,
                                         const double* __restrict__ gx, const double* __restrict__ gy, const double* __restrict__ gz,
                                         const double* __restrict__ Cx, const double* __restrict__ Cy, const double* __restrict__ Cz,
                                         double* __restrict__ w, double* __restrict__ limOut, int nf, int xcd)
{
    int f0, f1; block_chunk(nf, xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = lo[f], N = up[f];
        const double fl = flux[f];
        const double gradf = phi[N] - phi[P];
        const double dx = Cx[N] - Cx[P], dy = Cy[N] - Cy[P], dz = Cz[N] - Cz[P];
        const int c = fl > 0 ? P : N;
        const double gradcf = fma(dz, gz[c], fma(dx, gx[c], dy * gy[c]));
        double r;
        if (fabs(gradcf) >= 1000 * fabs(gradf)) r = 2 * 1000 * (gradcf >= 0 ? 1.0 : -1.0) * (gradf >= 0 ? 1.0 : -1.0) - 1;
        else r = fma(2.0, gradcf / gradf, -1.0);
        double lim = twoByk * r;
        lim = lim < 1 ? lim : 1;
        lim = lim > 0 ? lim : 0;
        if (limOut) limOut[f] = lim;
        w[f] = fma(lim, cdw[f], (1.0 - lim) * (fl >= 0 ? 1.0 : 0.0));
    }
}
// faceFlux*correction(vf) of linearUpwind / LUST on the internal faces for n_rhs <= 4 components in one sweep (the reference: the
// gradient, the correction field, [the 0.25 scale,] the product -- per component): faceFlux and Cf read once, C and the gradients gathered
// at the upwind cell; XCD-aware chunks as k_limited_linear_weights
struct CorrOut { double* out[4]; };
__global__ void k_linear_upwind_corr(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const double* __restrict__ flux,
                                     const CorrIn q, const CorrOut o, int nRhs, int nf, int xcd)
{
    int f0, f1; block_chunk(nf, xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        double t[4]; lu_face(q, nRhs, lo, up, flux, f, t);
#pragma unroll
        for (int r = 0; r < 4; ++r) if (r < nRhs) o.out[r][f] = t[r];
    }
}
// the same on one COUPLED patch (linearUpwind.C:49-62, the functor the reference runs): flux > 0: (pCf - C[o]) & grad[o]; otherwise
// ((pCf - C[o]) - pd) & gradNbr[i], pd = patch().delta(), gradNbr the gradient's patchNeighbourField
struct PatchCorrIn {
    const double *pcf[3], *cc[3], *pd[3], *grad[12], *nbr[12];
    double scale;
};
__global__ void k_patch_linear_upwind_corr(const int32_t* __restrict__ faceCells, const double* __restrict__ pflux, const PatchCorrIn q,
                                           const CorrOut o, int nRhs, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = faceCells[i];
    const double fl = pflux[i];
    const bool own = fl > 0;
    double dx = q.pcf[0][i] - q.cc[0][c], dy = q.pcf[1][i] - q.cc[1][c], dz = q.pcf[2][i] - q.cc[2][c];
    if (!own) { dx = dx - q.pd[0][i]; dy = dy - q.pd[1][i]; dz = dz - q.pd[2][i]; }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < nRhs) {
            const double gx = own ? q.grad[3 * r][c] : q.nbr[3 * r][i], gy = own ? q.grad[3 * r + 1][c] : q.nbr[3 * r + 1][i],
                         gz = own ? q.grad[3 * r + 2][c] : q.nbr[3 * r + 2][i];
            o.out[r][i] = fl * (q.scale * lu_dot(dx, dy, dz, gx, gy, gz));
        }
}
// LUST weights (LUST.H:104-110): 0.75*w_linear + 0.25*pos(faceFlux) -- three field operations, three roundings (no fma)
__global__ __launch_bounds__(RB) void k_lust_weights(const double* __restrict__ cdw, const double* __restrict__ flux, double* __restrict__ w, int64_t n)
{
    cell_map<4>(n, {cdw, flux}, {w}, [](const double (&x)[2], double (&o)[1]) { o[0] = 0.75 * x[0] + 0.25 * (x[1] >= 0 ? 1.0 : 0.0); });
}
// ---- the explicit correction of `cubic` (schemes/cubic/cubic.H:111-184, DESIGN 3.5j) ---------------------------------------------------
// [faceFlux *] correction(vf) for n_rhs <= 4 components in one face pass (the reference: three coefficient fields, then per component the
// two-weight interpolate, the gradient's interpolate, the dot product, two divisions and the sum).  The coefficients come from the one
// lambda stream, each field operator rounded on its own:  kSc = lambda*(1 - lambda*(3 - 2*lambda)),  kVecP = ((1 - lambda)*(1 - lambda))*lambda,
// kVecN = (lambda*lambda)*(lambda - 1).  On the internal faces the interpolate functor (surfaceInterpolationScheme.C:159-166) contracts
// its first product; on a coupled patch the reference evaluates field operators (.C:257-259): two rounded products and a sum.
struct CubicGeo { const double *lam, *sf[3], *magSf, *dc; };
__device__ __forceinline__ void cubic_coeffs(double lam, double& kSc, double& kP, double& kN)
{
    kSc = lam * (1 - lam * (3 - 2 * lam));
    kP = ((1 - lam) * (1 - lam)) * lam;
    kN = (lam * lam) * (lam - 1);
}
// corr = c0 + (((gI & Sf)/magSf)/deltaCoeffs), then the flux; gI the interpolated gradient
__device__ __forceinline__ double cubic_close(const CubicGeo& g, int f, double c0, double gx, double gy, double gz, const double* flux)
{
    const double corr = c0 + ((lu_dot(gx, gy, gz, g.sf[0][f], g.sf[1][f], g.sf[2][f]) / g.magSf[f]) / g.dc[f]);
    return flux ? flux[f] * corr : corr;
}
struct CubicArgs {
    const int32_t *lo, *up;
    CubicGeo g;
    const double *flux, *vf[4], *grad[12];
    double* out[4];
    int nRhs, nf, xcd;
};
// the internal faces: XCD-aware chunks as k_linear_upwind_corr; seven face arrays streamed, vf and its gradient gathered at both cells
__global__ void k_cubic_corr(const CubicArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        double kSc, kP, kN; cubic_coeffs(a.g.lam[f], kSc, kP, kN);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < a.nRhs) {
                const double c0 = fma(kSc, a.vf[r][P], (-kSc) * a.vf[r][N]);
                double gI[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) gI[k] = fma(kP, a.grad[3 * r + k][P], kN * a.grad[3 * r + k][N]);
                a.out[r][f] = cubic_close(a.g, f, c0, gI[0], gI[1], gI[2], a.flux);
            }
    }
}
struct PatchCubicArgs {
    const int32_t* fc;
    CubicGeo g;
    const double *flux, *vf[4], *nvf[4], *grad[12], *ngrad[12];
    double* out[4];
    int nRhs, n;
};
// one COUPLED patch: vf / grad through faceCells, nvf / ngrad the caller's patchNeighbourField; nothing contracted but the dot product
__global__ void k_patch_cubic_corr(const PatchCubicArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int o = a.fc[i];
    double kSc, kP, kN; cubic_coeffs(a.g.lam[i], kSc, kP, kN);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < a.nRhs) {
            const double c0 = kSc * a.vf[r][o] + (-kSc) * a.nvf[r][i];
            double gI[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) gI[k] = kP * a.grad[3 * r + k][o] + kN * a.ngrad[3 * r + k][i];
            a.out[r][i] = cubic_close(a.g, i, c0, gI[0], gI[1], gI[2], a.flux);
        }
}
// ---- the TVD/NVD limited schemes (limitedSchemes/*, DESIGN 3.5b) ------------------------------------------------------------------
// LimitedSchemeCalcLimiterFunctor (LimitedScheme.C:41-55) for every limiter of the family over NVDTVD (a scalar) or NVDVTVDV (the "V"
// schemes: a vector, its gradient grad[3*j + k] = d(phi_j)/dx_k), with the LimitedLimiter bounds (Limited.H:93-133, scalar form only),
// then the weights lim*cdw + (1 - lim)*pos(flux) (limitedSurfaceInterpolationScheme.C:155-161).  One contraction rule throughout: a dot
// product is lu_dot, of two products in a sum the first is fused; max / min are the reference's (s1 > s2) ? s1 : s2 / (s1 < s2) ? s1 : s2.
enum { LIM_LINEAR, LIM_VANLEER, LIM_MUSCL, LIM_MINMOD, LIM_SUPERBEE, LIM_UMIST, LIM_VANALBADA, LIM_OSPRE, LIM_QUICK, LIM_CUBIC, LIM_GAMMA, LIM_SFCD, LIM_N,
       // the filtered centred limiters (mi_filtered_limiter, DESIGN 3.5j): kinds of the same face passes that no mi_limiter reaches
       LIM_FLT_LINEAR = LIM_N, LIM_FLT_LINEAR2, LIM_FLT_LINEAR3, LIM_ALL };
struct LimCoef { double twoByk, gammaK, lower, upper; int bounded; double fltK, fltL; };   // fltL: l_ = l + 1.0 (filteredLinear2.H:101)
__device__ __forceinline__ double rmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double rmin(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double rsign(double s) { return s >= 0 ? 1.0 : -1.0; }
__device__ __forceinline__ double rstab(double s) { return s >= 0 ? s + 1e-15 : s - 1e-15; }   // stabilise(s, SMALL)
// phi(p, j): component j at the owner side (p) or the neighbour side; grad(p, c): gradient component c there.  Only what KIND reads
// is loaded: the scalar form gathers the gradient at the upwind cell only, limitedCubic and the filtered kinds at both.
template <int KIND, bool VEC, class PHI, class GRAD>
__device__ __forceinline__ double lim_face(const LimCoef& L, double cdw, double fl, const PHI& phi, const GRAD& grad, double dx, double dy, double dz)
{
    constexpr int M = VEC ? 3 : 1;
    double pP[M], pN[M];
#pragma unroll
    for (int j = 0; j < M; ++j) { pP[j] = phi(true, j); pN[j] = phi(false, j); }
    auto dg = [&](bool p, int j) { return lu_dot(dx, dy, dz, grad(p, 3 * j), grad(p, 3 * j + 1), grad(p, 3 * j + 2)); };   // d & grad(phi_j)
    if constexpr (KIND >= LIM_FLT_LINEAR) {                        // centred: both cells' gradients, never the flux; no product-plus-sum to contract
        double df, cP, cN;                                        // the face difference and d & gradc at either cell (V: along dfV)
        if (VEC) {                                                // filteredLinear2V.H:117-126, filteredLinear3V.H:97-106
            double dfV[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) dfV[j] = pN[j] - pP[j];
            df = lu_dot(dfV[0], dfV[1], dfV[2], dfV[0], dfV[1], dfV[2]);
            cP = lu_dot(dfV[0], dfV[1], dfV[2], dg(true, 0), dg(true, 1), dg(true, 2));
            cN = lu_dot(dfV[0], dfV[1], dfV[2], dg(false, 0), dg(false, 1), dg(false, 2));
        } else {
            df = pN[0] - pP[0];
            cP = dg(true, 0);
            cN = dg(false, 0);
        }
        if constexpr (KIND == LIM_FLT_LINEAR) {                   // filteredLinear.H:81-92: between linear and 20 % upwind
            const double lim = 2 - (0.5 * rmin(fabs(df - cP), fabs(df - cN))) / (rmax(fabs(cP), fabs(cN)) + 1e-15);
            return rmax(rmin(lim, 1.0), 0.8);
        }
        const double tP = 2 * cP, tN = 2 * cN;                    // exact
        if constexpr (KIND == LIM_FLT_LINEAR2) {                  // filteredLinear2.H:117-140; the V form adds VSMALL (filteredLinear2V.H:135,141)
            const double m = df > 0 ? rmin(rmax(df - tP, 0.0), rmax(df - tN, 0.0)) : rmin(rmax(tP - df, 0.0), rmax(tN - df, 0.0));
            const double lim = L.fltL - (L.fltK * m) / (rmax(fabs(df), rmax(fabs(tP), fabs(tN))) + (VEC ? 1e-300 : 1e-15));
            return rmax(rmin(lim, 1.0), 0.0);
        }
        const double lim = 1 - ((L.fltK * (tN - df)) * (tP - df)) / rmax((tN + tP) * (tN + tP), 1e-15);   // filteredLinear3.H:104, filteredLinear3V.H:109
        return rmax(rmin(lim, 1.0), 0.0);
    }
    if (!VEC && L.bounded && ((fl > 0 && (pP[0] < L.lower || pN[0] > L.upper)) || (fl < 0 && (pN[0] < L.lower || pP[0] > L.upper)))) return 0.0;
    const bool up = fl > 0;                                       // strict (NVDTVD.H:110)
    double gfV[3] = {0.0, 0.0, 0.0}, gradf, gradcf;
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 3; ++j) gfV[j] = pN[j] - pP[j];
        gradf = lu_dot(gfV[0], gfV[1], gfV[2], gfV[0], gfV[1], gfV[2]);
        gradcf = lu_dot(gfV[0], gfV[1], gfV[2], dg(up, 0), dg(up, 1), dg(up, 2));
    } else {
        gradf = pN[0] - pP[0];
        gradcf = dg(up, 0);
    }
    if constexpr (KIND == LIM_GAMMA || KIND == LIM_SFCD) {         // NVDTVD.H:85-92 phict
        const double phict = fabs(gradf) >= 1000 * fabs(gradcf) ? 1 - 0.5 * 1000 * rsign(gradcf) * rsign(gradf) : 1 - 0.5 * gradf / gradcf;
        if constexpr (KIND == LIM_GAMMA) return rmin(rmax(phict / L.gammaK, 0.0), 1.0);   // Gamma.H:96
        const double lp = rmin(rmax(phict, 0.0), 0.5);                                      // SFCD.H:81-82
        return lp / (1 - lp);
    }
    if constexpr (KIND == LIM_QUICK) {                            // QUICK.H:80-99, QUICKV.H:80-101
        const double q = 1 - cdw;
        double phiCD, phiU;
        if (VEC) {
            double w[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) w[j] = fma(cdw, pP[j], q * pN[j]);
            phiCD = lu_dot(gfV[0], gfV[1], gfV[2], w[0], w[1], w[2]);
            phiU = up ? lu_dot(gfV[0], gfV[1], gfV[2], pP[0], pP[1], pP[2]) : lu_dot(gfV[0], gfV[1], gfV[2], pN[0], pN[1], pN[2]);
        } else {
            phiCD = fma(cdw, pP[0], q * pN[0]);
            phiU = up ? pP[0] : pN[0];
        }
        const double phif = 0.5 * fma(up ? q : -cdw, gradcf, phiCD + phiU);   // gradcf: (gradfV &) (d & gradc[upwind])
        return rmax(rmin((phif - phiU) / rstab(phiCD - phiU), 2.0), 0.0);
    }
    const double r = fabs(gradcf) >= 1000 * fabs(gradf) ? 2 * 1000 * rsign(gradcf) * rsign(gradf) - 1 : fma(2.0, gradcf / gradf, -1.0);   // NVDTVD.H:119-126
    if constexpr (KIND == LIM_LINEAR) return rmax(rmin(L.twoByk * r, 1.0), 0.0);                      // limitedLinear.H:96
    if constexpr (KIND == LIM_VANLEER) return (r + fabs(r)) / (1 + fabs(r));                          // vanLeer.H:81
    if constexpr (KIND == LIM_MUSCL) return rmax(rmin(rmin(2 * r, 0.5 * r + 0.5), 2.0), 0.0);         // MUSCL.H:80
    if constexpr (KIND == LIM_MINMOD) return rmax(rmin(r, 1.0), 0.0);                                 // Minmod.H:80
    if constexpr (KIND == LIM_SUPERBEE) return rmax(rmax(rmin(2 * r, 1.0), rmin(r, 2.0)), 0.0);       // SuperBee.H:81
    if constexpr (KIND == LIM_UMIST) return rmax(rmin(rmin(rmin(2 * r, fma(0.75, r, 0.25)), 0.25 * r + 0.75), 2.0), 0.0);   // UMIST.H:80
    if constexpr (KIND == LIM_VANALBADA) return r * (r + 1) / fma(r, r, 1.0);                         // vanAlbada.H:81
    if constexpr (KIND == LIM_OSPRE) { const double rr = r * (r + 1); return 1.5 * rr / (rr + 1); }   // OSPRE.H:81-82
    if constexpr (KIND == LIM_CUBIC) {                            // limitedCubic.H:91-127, limitedCubicV.H:91-124
        const double twor = L.twoByk * r, q = 1 - cdw;
        double phif, phiCD, fU;
        if (VEC) {
            double fV[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) fV[j] = fma(cdw, pP[j], (1.0 - cdw) * pN[j]);
            const double fP = lu_dot(fV[0], fV[1], fV[2], pP[0], pP[1], pP[2]), fN = lu_dot(fV[0], fV[1], fV[2], pN[0], pN[1], pN[2]);
            const double tN = lu_dot(fV[0], fV[1], fV[2], dg(false, 0), dg(false, 1), dg(false, 2));
            const double tP = lu_dot(fV[0], fV[1], fV[2], dg(true, 0), dg(true, 1), dg(true, 2));
            fU = up ? fP : fN;
            phif = fma(cdw, fP - 0.25 * tN, q * (fN + 0.25 * tP));
            phiCD = fma(cdw, fP, q * fN);
        } else {
            fU = up ? pP[0] : pN[0];
            phif = fma(cdw, pP[0] - 0.25 * dg(false, 0), q * (pN[0] + 0.25 * dg(true, 0)));
            phiCD = fma(cdw, pP[0], q * pN[0]);
        }
        const double cubic = (phif - fU) / rstab(phiCD - fU);
        return rmax(rmin(rmin(twor, cubic), 2.0), 0.0);
    }
    return 0.0;
}
struct LimArgs {
    const int32_t *lo, *up;
    const double *cdw, *flux, *phi[3], *grad[9], *cc[3];
    double *w, *limOut;
    LimCoef k;
    int nf, xcd;
};
// the internal faces: XCD-aware chunks as k_limited_linear_weights; cdw and flux streamed, phi / grad / C gathered; d = C[N] - C[P]
template <int KIND, bool VEC>
__global__ void k_limited_weights(const LimArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        const double fl = a.flux[f], cdw = a.cdw[f];
        const double dx = a.cc[0][N] - a.cc[0][P], dy = a.cc[1][N] - a.cc[1][P], dz = a.cc[2][N] - a.cc[2][P];
        const double lim = lim_face<KIND, VEC>(a.k, cdw, fl, [&](bool p, int j) { return a.phi[j][p ? P : N]; },
                                               [&](bool p, int c) { return a.grad[c][p ? P : N]; }, dx, dy, dz);
        if (a.limOut) a.limOut[f] = lim;
        a.w[f] = fma(lim, cdw, (1.0 - lim) * (fl >= 0 ? 1.0 : 0.0));
    }
}
struct PatchLimArgs {
    const int32_t* fc;
    const double *cdw, *flux, *phi[3], *nphi[3], *grad[9], *ngrad[9], *pd[3];
    double *w, *limOut;
    LimCoef k;
    int n;
};
// one COUPLED patch (LimitedScheme.C:145-195): phiP / gradcP through faceCells, phiN / gradcN the caller's patchNeighbourField,
// d = pd - (0,0,0) = pd
template <int KIND, bool VEC>
__global__ void k_patch_limited_weights(const PatchLimArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int o = a.fc[i];
    const double fl = a.flux[i], cdw = a.cdw[i];
    const double lim = lim_face<KIND, VEC>(a.k, cdw, fl, [&](bool p, int j) { return p ? a.phi[j][o] : a.nphi[j][i]; },
                                           [&](bool p, int c) { return p ? a.grad[c][o] : a.ngrad[c][i]; }, a.pd[0][i], a.pd[1][i], a.pd[2][i]);
    if (a.limOut) a.limOut[i] = lim;
    a.w[i] = fma(lim, cdw, (1.0 - lim) * (fl >= 0 ? 1.0 : 0.0));
}
// fvc::grad, Gauss (gaussGrad.C:27-90): the row pass above with four staged face arrays (Sf x3 + ssf) and three
// accumulators; ssf is read once for the three components; every term is one fma, like the oracle.
struct GradArgs {
    const int32_t *os, *ls, *losort, *blockStart;
    const double *Sfx, *Sfy, *Sfz, *ssf, *vol;
    double *gx, *gy, *gz;
    int n, cap, xcd;
};
template <int BS>
__global__ __launch_bounds__(BS) void k_gauss_grad(const GradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    double *sx = rp_smem, *sy = sx + a.cap, *sz = sy + a.cap, *ss = sz + a.cap;
    const int lb = a.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.blockStart) { c0 = a.blockStart[lb]; cEnd = a.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.os[c0], nf = a.os[cEnd] - f0;
    const bool staged = nf <= a.cap;
    if (staged) {
        stage_dma8<BS>(a.Sfx + f0, sx, nf, tid); stage_dma8<BS>(a.Sfy + f0, sy, nf, tid);
        stage_dma8<BS>(a.Sfz + f0, sz, nf, tid); stage_dma8<BS>(a.ssf + f0, ss, nf, tid);
    }
    int nb = 0, ne = 0;
    if (live) { nb = a.ls[c]; ne = a.ls[c + 1]; }
    const int cnt = ne - nb;
    int nfk[4]; double nx[4], ny[4], nz[4], ns[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nfk[k] = (k < cnt) ? a.losort[nb + k] : 0;
        if (k < cnt && (!staged || nfk[k] < f0)) { const int f = nfk[k]; nx[k] = a.Sfx[f]; ny[k] = a.Sfy[f]; nz[k] = a.Sfz[f]; ns[k] = a.ssf[f]; }
        else { nx[k] = ny[k] = nz[k] = ns[k] = 0.0; }
    }
    __syncthreads();
    if (!live) return;
    double ox = 0, oy = 0, oz = 0;
    const int ob = a.os[c], oe = a.os[c + 1];
    if (staged) for (int j = ob - f0; j < oe - f0; ++j) { const double s = ss[j]; ox = fma(sx[j], s, ox); oy = fma(sy[j], s, oy); oz = fma(sz[j], s, oz); }
    else for (int j = ob; j < oe; ++j) { const double s = a.ssf[j]; ox = fma(a.Sfx[j], s, ox); oy = fma(a.Sfy[j], s, oy); oz = fma(a.Sfz[j], s, oz); }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) {
        if (staged && nfk[k] >= f0) { const int j = nfk[k] - f0; nx[k] = sx[j]; ny[k] = sy[j]; nz[k] = sz[j]; ns[k] = ss[j]; }
        ox = fma(-nx[k], ns[k], ox); oy = fma(-ny[k], ns[k], oy); oz = fma(-nz[k], ns[k], oz);
    }
    for (int j = nb + 4; j < ne; ++j) {
        const int f = a.losort[j];
        double vx, vy, vz, s;
        if (staged && f >= f0) { vx = sx[f - f0]; vy = sy[f - f0]; vz = sz[f - f0]; s = ss[f - f0]; }
        else { vx = a.Sfx[f]; vy = a.Sfy[f]; vz = a.Sfz[f]; s = a.ssf[f]; }
        ox = fma(-vx, s, ox); oy = fma(-vy, s, oy); oz = fma(-vz, s, oz);
    }
    if (a.vol) { const double v = a.vol[c]; ox /= v; oy /= v; oz /= v; }
    a.gx[c] = ox; a.gy[c] = oy; a.gz[c] = oz;
}
// fvc::surfaceIntegrate of three face fields at once (the flux components of k_face_dev_tgrad_flux): k_gauss_grad's skeleton with
// three staged face arrays and plain sums -- own faces ascending +, then the losort faces -, then the optional /V, the order of
// mi_surface_integrate (lduAddressingFunctors.H:10-64) -- so the row tables are read once for the three components
struct RowSum3Args {
    const int32_t *os, *ls, *losort, *blockStart;
    const double *f[3], *vol;
    double* out[3];
    int n, cap, xcd;
};
template <int BS>
__global__ __launch_bounds__(BS) void k_row_sum3(const RowSum3Args a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    double *s0 = rp_smem, *s1 = s0 + a.cap, *s2 = s1 + a.cap;
    const int lb = a.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.blockStart) { c0 = a.blockStart[lb]; cEnd = a.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.os[c0], nf = a.os[cEnd] - f0;
    const bool staged = nf <= a.cap;
    if (staged) { stage_dma8<BS>(a.f[0] + f0, s0, nf, tid); stage_dma8<BS>(a.f[1] + f0, s1, nf, tid); stage_dma8<BS>(a.f[2] + f0, s2, nf, tid); }
    int nb = 0, ne = 0;
    if (live) { nb = a.ls[c]; ne = a.ls[c + 1]; }
    const int cnt = ne - nb;
    int nfk[4]; double n0[4], n1[4], n2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nfk[k] = (k < cnt) ? a.losort[nb + k] : 0;
        if (k < cnt && (!staged || nfk[k] < f0)) { const int f = nfk[k]; n0[k] = a.f[0][f]; n1[k] = a.f[1][f]; n2[k] = a.f[2][f]; }
        else { n0[k] = n1[k] = n2[k] = 0.0; }
    }
    __syncthreads();
    if (!live) return;
    double o0 = 0, o1 = 0, o2 = 0;
    const int ob = a.os[c], oe = a.os[c + 1];
    if (staged) for (int j = ob - f0; j < oe - f0; ++j) { o0 += s0[j]; o1 += s1[j]; o2 += s2[j]; }
    else for (int j = ob; j < oe; ++j) { o0 += a.f[0][j]; o1 += a.f[1][j]; o2 += a.f[2][j]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) {
        if (staged && nfk[k] >= f0) { const int j = nfk[k] - f0; n0[k] = s0[j]; n1[k] = s1[j]; n2[k] = s2[j]; }
        o0 -= n0[k]; o1 -= n1[k]; o2 -= n2[k];
    }
    for (int j = nb + 4; j < ne; ++j) {
        const int f = a.losort[j];
        if (staged && f >= f0) { o0 -= s0[f - f0]; o1 -= s1[f - f0]; o2 -= s2[f - f0]; }
        else { o0 -= a.f[0][f]; o1 -= a.f[1][f]; o2 -= a.f[2][f]; }
    }
    if (a.vol) { const double v = a.vol[c]; o0 /= v; o1 /= v; o2 /= v; }
    a.out[0][c] = o0; a.out[1][c] = o1; a.out[2][c] = o2;
}
__global__ __launch_bounds__(RB) void k_vdiv(const double* x, const double* y, double* out, int64_t n) // out may alias x
{
    cell_map<4>(n, {x, y}, {out}, [](const double (&v)[2], double (&o)[1]) { o[0] = v[0] / v[1]; });
}
__global__ __launch_bounds__(RB) void k_axpby(double a, const double* x, double b, const double* y, double* out, int64_t n) // out may alias x or y
{
    cell_map<4>(n, {x, y}, {out}, [&](const double (&v)[2], double (&o)[1]) { o[0] = fma(a, v[0], b * v[1]); });
}

} // namespace mi

struct mi_patch_s {
    mi_ctx_s* ctx = nullptr;
    int32_t nFaces = 0, nUnique = 0;
    DevBuf<int32_t> cells, start, sort, faceCells;
};
typedef struct mi_patch_s* mi_patch_t;

namespace {
int ensure_caller_tables(mi_addr_s* a)
{
    if (a->ownerStartC.n == (size_t)a->L.nCells + 1) return MI_OK;
    const int32_t n = a->L.nCells, nf = a->L.nFaces;
    Table<int32_t> os((size_t)n + 1, 0), ls((size_t)n + 1, 0), losort((size_t)nf);
    for (int32_t f = 0; f < nf; ++f) { ++os[(size_t)a->lowerHost[f] + 1]; ++ls[(size_t)a->upperHost[f] + 1]; }
    for (int32_t c = 0; c < n; ++c) { os[(size_t)c + 1] += os[c]; ls[(size_t)c + 1] += ls[c]; }
    for (int32_t f = 0; f + 1 < nf; ++f)
        if (a->lowerHost[f] > a->lowerHost[(size_t)f + 1])
            return fail(MI_ERR_ARG, "assembly sweeps need owner-sorted (upper-triangular) face order");
    Table<int32_t> cur(ls.begin(), ls.end() - 1);
    for (int32_t f = 0; f < nf; ++f) losort[(size_t)cur[a->upperHost[f]]++] = f;
    hipStream_t s = a->ctx->stream;
    MICHK(a->ownerStartC.upload(os, s)); MICHK(a->losortStartC.upload(ls, s)); MICHK(a->losortC.upload(losort, s));
    if (a->lowerAddr.n != (size_t)nf) { MICHK(a->lowerAddr.upload(a->lowerHost, s)); MICHK(a->upperAddr.upload(a->upperHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
    // blocks of the row passes: the layout's tiles when the caller's numbering is tile-contiguous, fixed ranges otherwise --
    // 1024 cells for the one- and two-array passes (more neighbour-side faces inside the block: fvm::div 286 -> 253 us on the
    // 216^3 box), 256 for the four-array gradient (1024-cell blocks leave one workgroup per CU: 397 -> 437 us)
    const bool tiles = a->identity && a->L.nTiles > 0 && a->L.maxCells <= 1024;
    for (int k = 0; k < 2; ++k) {
        mi_addr_s::RowPlan& rp = a->rowPlan[k];
        rp = mi_addr_s::RowPlan();
        rp.tiles = tiles;
        rp.capForced = sw::get(SW_ROW_CAP);
        if (tiles) {
            rp.bs = a->L.maxCells <= 256 ? 256 : a->L.maxCells <= 512 ? 512 : 1024;
            rp.blocks = a->L.nTiles;
            for (int32_t t = 0; t < a->L.nTiles; ++t)
                rp.maxFaces = std::max(rp.maxFaces, os[(size_t)a->L.tileCellStart[(size_t)t + 1]] - os[(size_t)a->L.tileCellStart[t]]);
        } else {
            const int bs = sw::get(k == 0 ? SW_ROW_BS : SW_GRAD_BS);
            rp.bs = bs <= 256 ? 256 : bs <= 512 ? 512 : 1024;
            rp.blocks = (n + rp.bs - 1) / rp.bs;
            for (int32_t c0 = 0; c0 < n; c0 += rp.bs) rp.maxFaces = std::max(rp.maxFaces, os[(size_t)std::min(c0 + rp.bs, n)] - os[c0]);
        }
    }
    // block-local 16-bit row tables for the blocks of plan [0] (k_row_pass<..., R16>): usable when every block has < 32768 own
    // faces and cut faces and < 65536 neighbour-list entries (a 1024-cell block has ~3 000 / ~300 / ~3 000)
    if (sw::get(SW_ROW16) != 0 && nf > 0) {
        const mi_addr_s::RowPlan& rp = a->rowPlan[0];
        const int nB = rp.blocks;
        auto block_cells = [&](int b, int32_t& c0, int32_t& c1) {
            if (rp.tiles) { c0 = a->L.tileCellStart[(size_t)b]; c1 = a->L.tileCellStart[(size_t)b + 1]; }
            else { c0 = b * rp.bs; c1 = std::min(c0 + rp.bs, n); }
        };
        Table<int32_t> escStart((size_t)nB + 1, 0);
        std::atomic<bool> fits{true};
        mi::parallel_for(nB, 64, [&](int64_t b) {
            int32_t c0, c1; block_cells((int)b, c0, c1);
            const int32_t f0 = os[(size_t)c0];
            int32_t cut = 0;
            for (int32_t j = ls[(size_t)c0]; j < ls[(size_t)c1]; ++j) if (losort[(size_t)j] < f0) ++cut;
            if (os[(size_t)c1] - f0 >= 32768 || cut >= 32768 || ls[(size_t)c1] - ls[(size_t)c0] >= 65536) fits = false;
            escStart[(size_t)b + 1] = cut;
        });
        if (fits) {
            for (int b = 0; b < nB; ++b) escStart[(size_t)b + 1] += escStart[(size_t)b];
            Table<uint32_t> row16((size_t)n);
            Table<uint16_t> l16((size_t)nf);
            Table<int32_t> esc((size_t)std::max(escStart[(size_t)nB], 1));
            mi::parallel_for(nB, 64, [&](int64_t b) {
                int32_t c0, c1; block_cells((int)b, c0, c1);
                const int32_t f0 = os[(size_t)c0], l0 = ls[(size_t)c0];
                int32_t k = 0;
                for (int32_t c = c0; c < c1; ++c) row16[(size_t)c] = (uint32_t)(os[(size_t)c + 1] - f0) | ((uint32_t)(ls[(size_t)c + 1] - l0) << 16);
                for (int32_t j = l0; j < ls[(size_t)c1]; ++j) {
                    const int32_t f = losort[(size_t)j];
                    if (f >= f0) l16[(size_t)j] = (uint16_t)(f - f0);
                    else { esc[(size_t)escStart[(size_t)b] + (size_t)k] = f; l16[(size_t)j] = (uint16_t)(0x8000u | (uint32_t)k); ++k; }
                }
            });
            MICHK(a->row16.upload(row16, s)); MICHK(a->losort16.upload(l16, s)); MICHK(a->rowEsc.upload(esc, s)); MICHK(a->rowEscStart.upload(escStart, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    return MI_OK;
}
// workgroups of a face pass or a unique-cell patch pass: one thread per item up to the context's cap (MI_FACE_GRID, 8192 unless a
// test lowers it); past it the kernel's own loop -- grid-stride or block_chunk -- walks the rest, so EVERY kernel launched with it loops
int grid_for(const mi_ctx_s* c, int n) { const int b = (n + 255) / 256, cap = c->faceGrid; return b < 1 ? 1 : (b > cap ? cap : b); }
// a mesh without internal faces is legal lduAddressing (one cell; cells joined by patches only): its face arrays are empty, an empty
// array's pointer may be NULL and is never read -- the entries ask for a face array only of a mesh that has faces (shown by the
// meshes one_cell and no_faces of tests/test_degenerate_meshes.py)
bool faceless(const mi_addr_s* a) { return a->L.nFaces == 0; }
} // namespace

extern "C" int mi_patch_create(mi_ctx_t ctx, int32_t n_cells, int32_t n_patch_faces, const int32_t* face_cells_host, mi_patch_t* out)
{
    if (!ctx || !out || n_patch_faces < 0 || (n_patch_faces > 0 && !face_cells_host)) return fail(MI_ERR_ARG, "mi_patch_create: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    Table<int32_t> order((size_t)n_patch_faces);
    for (int32_t i = 0; i < n_patch_faces; ++i) {
        if (face_cells_host[i] < 0 || face_cells_host[i] >= n_cells) return fail(MI_ERR_ARG, "mi_patch_create: faceCells out of range");
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return face_cells_host[a] < face_cells_host[b]; });
    Table<int32_t> cells, start;
    for (int32_t k = 0; k < n_patch_faces; ++k) {
        const int32_t c = face_cells_host[order[k]];
        if (cells.empty() || cells.back() != c) { cells.push_back(c); start.push_back(k); }
    }
    start.push_back(n_patch_faces);
    mi_patch_s* p = new mi_patch_s();
    p->ctx = ctx; p->nFaces = n_patch_faces; p->nUnique = (int32_t)cells.size();
    int r = p->cells.upload(cells, ctx->stream);
    if (r == MI_OK) r = p->start.upload(start, ctx->stream);
    if (r == MI_OK) r = p->sort.upload(order, ctx->stream);
    if (r == MI_OK) r = p->faceCells.upload(Table<int32_t>(face_cells_host, face_cells_host + n_patch_faces), ctx->stream);
    if (r != MI_OK) { delete p; return r; }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { delete p; return fail(MI_ERR_DEVICE, "upload failed"); }
    *out = p;
    return MI_OK;
}
extern "C" int mi_patch_destroy(mi_patch_t p) { delete p; return MI_OK; }

// fn: 0 add pf, 1 subtract pf, 2 add |pf|   (addToInternalField / subtractFromInternalField / relax functors)
extern "C" int mi_patch_add(mi_patch_t p, const double* pf_dev, double* intf_dev, int fn)
{
    if (!p || !intf_dev || (p->nFaces > 0 && !pf_dev) || fn < 0 || fn > 2) return fail(MI_ERR_ARG, "mi_patch_add: bad argument");
    if (p->nUnique == 0) return MI_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t s = p->ctx->stream;
    const int g = grid_for(p->ctx, p->nUnique);
    if (fn == 0) k_patch_add<0><<<g, 256, 0, s>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, intf_dev, p->nUnique);
    else if (fn == 1) k_patch_add<1><<<g, 256, 0, s>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, intf_dev, p->nUnique);
    else k_patch_add<2><<<g, 256, 0, s>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, intf_dev, p->nUnique);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// cell_inout[faceCells] = max(cell_inout[faceCells], pf): the patch part of CoEulerDdtScheme::CorDeltaT
extern "C" int mi_patch_max(mi_patch_t p, const double* pf_dev, double* cell_inout_dev)
{
    if (!p || !cell_inout_dev || (p->nFaces > 0 && !pf_dev)) return fail(MI_ERR_ARG, "mi_patch_max: bad argument");
    if (pf_dev == cell_inout_dev) return fail(MI_ERR_ARG, "mi_patch_max: the patch field must not be the cell field");
    if (p->nUnique == 0) return MI_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_max<<<grid_for(p->ctx, p->nUnique), 256, 0, p->ctx->stream>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, cell_inout_dev, p->nUnique);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// coupled part of fvMatrix::addBoundarySource (fvMatrix.C:318-346): source[faceCells] += boundaryCoeffs * patchNeighbourField
extern "C" int mi_patch_add_product(mi_patch_t p, const double* pf_dev, const double* q_dev, double* intf_dev, int fn)
{
    if (!p || !intf_dev || (p->nFaces > 0 && (!pf_dev || !q_dev)) || fn < 0 || fn > 1) return fail(MI_ERR_ARG, "mi_patch_add_product: bad argument");
    if (p->nUnique == 0) return MI_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t s = p->ctx->stream;
    const int g = grid_for(p->ctx, p->nUnique);
    if (fn == 0) k_patch_add<0, true><<<g, 256, 0, s>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, intf_dev, p->nUnique, q_dev);
    else k_patch_add<1, true><<<g, 256, 0, s>>>(p->cells.p, p->start.p, p->sort.p, pf_dev, intf_dev, p->nUnique, q_dev);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// boundary part of fvMatrix::flux (fvMatrix.C:1621-1653): internalCoeffs*patchInternalField - boundaryCoeffs[*patchNeighbourField]
__global__ void k_patch_flux(const int32_t* __restrict__ faceCells, const double* __restrict__ ic, const double* __restrict__ bc,
                             const double* __restrict__ psi, const double* __restrict__ psiNbr, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double inContrib = ic[i] * psi[faceCells[i]];
    const double nbContrib = psiNbr ? bc[i] * psiNbr[i] : bc[i];
    out[i] = inContrib - nbContrib;
}
extern "C" int mi_patch_flux(mi_patch_t p, const double* internal_coeffs_dev, const double* boundary_coeffs_dev, const double* psi_dev,
                             const double* patch_neighbour_field_dev_or_null, double* flux_dev)
{
    if (!p || (p->nFaces > 0 && (!internal_coeffs_dev || !boundary_coeffs_dev || !psi_dev || !flux_dev))) return fail(MI_ERR_ARG, "mi_patch_flux: bad argument");
    if (p->nFaces == 0) return MI_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_flux<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(p->faceCells.p, internal_coeffs_dev, boundary_coeffs_dev, psi_dev,
                                                                      patch_neighbour_field_dev_or_null, flux_dev, p->nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

namespace {
bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }    // the checks of a call's arrays are in row_entry.inc
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// a streaming pass on the fixed RG x RB grid, on the context's stream
template <class K, class... A>
int cell_launch(mi_ctx_s* c, K kernel, A... args)
{
    HIPCHK(hipSetDevice(c->device));
    kernel<<<RG, RB, 0, c->stream>>>(args...);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// the whitespace-separated words of a scheme string, as the reference's Istream reads them
std::vector<std::string> scheme_words(const char* text)
{
    std::vector<std::string> tok;
    auto sp = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == '\f' || ch == '\v'; };
    for (const char* c = text; *c;) {
        while (*c && sp(*c)) ++c;
        const char* b = c;
        while (*c && !sp(*c)) ++c;
        if (c > b) tok.emplace_back(b, c);
    }
    return tok;
}
// is the whole word a number (strtod: "nan" and "inf" are numbers; who refuses them says so itself)
bool scheme_number(const std::string& word, double& v)
{
    char* end = nullptr;
    v = std::strtod(word.c_str(), &end);
    return end != word.c_str() && *end == '\0';
}
// LDS per workgroup of a row pass: `arrays` staged face arrays of cap doubles.  Two workgroups per CU stay resident when the
// largest block fits in 76 KiB; a block with more own faces than cap falls back to global reads inside the kernel.
int row_cap(const mi_addr_s::RowPlan& rp, int arrays)
{
    if (rp.capForced > 0) return (rp.capForced + 1) & ~1; // MI_ROW_CAP (read when the plan is made): a small value sends blocks down the unstaged path (tests)
    const int want = (rp.maxFaces + 1) & ~1, fit2 = (76 * 1024 / 8 / arrays) & ~1, fit1 = (156 * 1024 / 8 / arrays) & ~1;
    return std::max(2, want <= fit2 ? want : want <= fit1 ? want : fit2); // one resident workgroup per CU when only that stages every block
}
template <class K, class A>
int row_launch(mi_addr_s* a, const mi_addr_s::RowPlan& rp, K kernel, const A& args, size_t lds)
{
    mi_ctx_s* cx = a->ctx;
    const void* fn = (const void*)kernel;
    if (lds > 48 * 1024 && !cx->ldsAttrSet.count(fn)) {
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));
        cx->ldsAttrSet.insert(fn);
    }
    kernel<<<rp.blocks, rp.bs, lds, cx->stream>>>(args);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// the block size of the row plan and the form of the row tables (16-bit row16 / losort16 or the 32-bit ones) pick a kernel instantiation:
// f(RowShape<BS, R16>{}) launches it
template <int BS, bool R16> struct RowShape { static constexpr int bs = BS; static constexpr bool r16 = R16; };
template <class F>
int for_row_shape(const mi_addr_s* a, const mi_addr_s::RowPlan& rp, F f)
{
    if (a->row16.n > 0) return rp.bs == 256 ? f(RowShape<256, true>{}) : rp.bs == 512 ? f(RowShape<512, true>{}) : f(RowShape<1024, true>{});
    return rp.bs == 256 ? f(RowShape<256, false>{}) : rp.bs == 512 ? f(RowShape<512, false>{}) : f(RowShape<1024, false>{});
}
template <int KIND, int OM, int NM>
int row_pass(mi_addr_s* a, RowPassArgs ra)
{
    if (a->L.nCells == 0) return MI_OK;
    const int arrays = (KIND == RP_DIV || (KIND == RP_SUM && ra.a0 != ra.a1)) ? 2 : 1;
    ra.os = a->ownerStartC.p; ra.ls = a->losortStartC.p; ra.losort = a->losortC.p;
    ra.row16 = a->row16.p; ra.losort16 = a->losort16.p; ra.esc = a->rowEsc.p; ra.escStart = a->rowEscStart.p;
    const mi_addr_s::RowPlan& rp = a->rowPlan[0];
    ra.blockStart = rp.tiles ? a->tileCellStart.p : nullptr;
    ra.n = a->L.nCells; ra.cap = row_cap(rp, arrays); ra.xcd = a->ctx->xcdRows;
    const size_t lds = (size_t)arrays * ra.cap * sizeof(double);
    return for_row_shape(a, rp, [&](auto s) { return row_launch(a, rp, k_row_pass<KIND, OM, NM, decltype(s)::bs, decltype(s)::r16>, ra, lds); });
}
template <int OM, int NM>
int row_sum(mi_addr_s* a, const double* ownArr, const double* neiArr, const double* init, const double* vol, double* out)
{
    RowPassArgs ra{};
    ra.a0 = ownArr; ra.a1 = neiArr; ra.init = init; ra.vol = vol; ra.out = out;
    return row_pass<RP_SUM, OM, NM>(a, ra);
}
} // namespace

extern "C" int mi_row_face_op(mi_addr_t a, int kind, const double* lower_dev, const double* upper_dev, double* inout_dev)
{
    if (!a || (!upper_dev && !faceless(a)) || !inout_dev || kind < 0 || kind > 2) return fail(MI_ERR_ARG, "mi_row_face_op: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    const double* lo = lower_dev ? lower_dev : upper_dev; // symmetric: lower aliases upper (lduMatrix.C:328-345)
    if (kind == ROW_SUMDIAG) return row_sum<M_PLUS, M_PLUS>(a, lo, upper_dev, inout_dev, nullptr, inout_dev);
    if (kind == ROW_NEGSUMDIAG) return row_sum<M_MINUS, M_MINUS>(a, lo, upper_dev, inout_dev, nullptr, inout_dev);
    return row_sum<M_MAG, M_MAG>(a, upper_dev, lo, inout_dev, nullptr, inout_dev);
}

extern "C" int mi_fvm_laplacian(mi_addr_t a, const double* delta_coeffs_dev, const double* gamma_magsf_dev, double* upper_out_dev, double* diag_out_dev)
{
    if (!a || !diag_out_dev) return fail(MI_ERR_ARG, "mi_fvm_laplacian: bad argument");
    if (!faceless(a) && (!delta_coeffs_dev || !gamma_magsf_dev || !upper_out_dev)) return fail(MI_ERR_ARG, "mi_fvm_laplacian: bad argument");
    if (!al16(delta_coeffs_dev) || !al16(gamma_magsf_dev) || !al16(upper_out_dev)) return fail(MI_ERR_ARG, "mi_fvm_laplacian: face fields must be 16-byte aligned");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (!faceless(a) && (upper_out_dev == delta_coeffs_dev || upper_out_dev == gamma_magsf_dev)) return fail(MI_ERR_ARG, "mi_fvm_laplacian: upper_out must not alias an input");
    // one pass (the reference: 3 + temporaries): each block forms the coefficients of its own faces, keeps them in LDS for
    // the row sums of its cells and recomputes only the faces cut by its boundary (with the same single rounding)
    RowPassArgs ra{};
    ra.a0 = delta_coeffs_dev; ra.a1 = gamma_magsf_dev; ra.f0out = upper_out_dev; ra.out = diag_out_dev;
    return row_pass<RP_LAPLACIAN, M_MINUS, M_MINUS>(a, ra);
}

extern "C" int mi_fvm_div(mi_addr_t a, const double* weights_dev, const double* face_flux_dev, double* lower_out_dev, double* upper_out_dev, double* diag_out_dev)
{
    if (!a || !diag_out_dev) return fail(MI_ERR_ARG, "mi_fvm_div: bad argument");
    if (!faceless(a) && (!weights_dev || !face_flux_dev || !lower_out_dev || !upper_out_dev)) return fail(MI_ERR_ARG, "mi_fvm_div: bad argument");
    if (!al16(weights_dev) || !al16(face_flux_dev) || !al16(lower_out_dev) || !al16(upper_out_dev)) return fail(MI_ERR_ARG, "mi_fvm_div: face fields must be 16-byte aligned");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (!faceless(a) && (lower_out_dev == weights_dev || lower_out_dev == face_flux_dev || upper_out_dev == weights_dev || upper_out_dev == face_flux_dev ||
                         lower_out_dev == upper_out_dev))
        return fail(MI_ERR_ARG, "mi_fvm_div: the coefficient outputs must not alias an input or each other");
    RowPassArgs ra{};
    ra.a0 = weights_dev; ra.a1 = face_flux_dev; ra.f0out = lower_out_dev; ra.f1out = upper_out_dev; ra.out = diag_out_dev;
    return row_pass<RP_DIV, M_MINUS, M_MINUS>(a, ra);
}


namespace {
// the correction's inputs for n_rhs components; every output must differ from every one of them (faces and cells of other blocks read
// them while this call writes)
int corr_in(const char* who, const mi_div_correction* k, int nRhs, CorrIn& q, const double* const* outs, int nOuts)
{
    if (!k || nRhs < 1 || nRhs > 4) return fail(MI_ERR_ARG, std::string(who) + ": a correction needs 1 to 4 components");
    q = CorrIn{};
    q.scale = k->scale;
    for (int d = 0; d < 3; ++d) { q.cf[d] = k->cf_dev[d]; q.cc[d] = k->c_dev[d]; }
    for (int j = 0; j < 3 * nRhs; ++j) q.grad[j] = k->grad_dev[j];
    const double* in[18];
    int m = 0;
    for (int d = 0; d < 3; ++d) { in[m++] = q.cf[d]; in[m++] = q.cc[d]; }
    for (int j = 0; j < 3 * nRhs; ++j) in[m++] = q.grad[j];
    for (int j = 0; j < m; ++j) if (!in[j]) return fail(MI_ERR_ARG, std::string(who) + ": correction arrays missing (Cf, C and 3 gradient components per right-hand side)");
    for (int d = 0; d < 3; ++d) if (!al16(q.cf[d])) return fail(MI_ERR_ARG, std::string(who) + ": face fields must be 16-byte aligned");
    for (int o = 0; o < nOuts; ++o)
        for (int j = 0; j < m; ++j)
            if (outs[o] && outs[o] == in[j]) return fail(MI_ERR_ARG, std::string(who) + ": an output must not alias a correction input");
    return MI_OK;
}
} // namespace

extern "C" int mi_linear_upwind_correction(mi_addr_t a, const mi_div_correction* corr, int32_t n_rhs, const double* face_flux_dev, double* const* out_dev)
{
    const char* who = "mi_linear_upwind_correction";
    if (!a) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (faceless(a)) return MI_OK;                        // no face to correct: the outputs are empty
    if (!face_flux_dev) return fail(MI_ERR_ARG, std::string(who) + ": the correction of a convection scheme needs its faceFlux");
    if (!al16(face_flux_dev)) return fail(MI_ERR_ARG, std::string(who) + ": face fields must be 16-byte aligned");
    if (!out_dev || n_rhs < 1 || n_rhs > 4) return fail(MI_ERR_ARG, std::string(who) + ": 1 to 4 outputs needed");
    CorrOut o{};
    for (int r = 0; r < n_rhs; ++r) {
        o.out[r] = out_dev[r];
        if (!o.out[r]) return fail(MI_ERR_ARG, std::string(who) + ": null output");
        if (o.out[r] == face_flux_dev) return fail(MI_ERR_ARG, std::string(who) + ": an output must not alias faceFlux");
        for (int s = 0; s < r; ++s) if (o.out[s] == o.out[r]) return fail(MI_ERR_ARG, std::string(who) + ": the outputs must differ");
    }
    CorrIn q;
    MICHK(corr_in(who, corr, n_rhs, q, o.out, n_rhs));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    k_linear_upwind_corr<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, face_flux_dev, q, o, n_rhs, a->L.nFaces,
                                                                                    a->ctx->xcdRows);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_patch_linear_upwind_correction(mi_patch_t p, double scale, int32_t n_rhs, const double* patch_flux_dev, const double* const* patch_cf_dev,
                                                 const double* const* c_dev, const double* const* patch_delta_dev, const double* const* grad_dev,
                                                 const double* const* nbr_grad_dev, double* const* out_dev)
{
    const char* who = "mi_patch_linear_upwind_correction";
    if (!p || n_rhs < 1 || n_rhs > 4) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (p->nFaces == 0) return MI_OK;
    if (!patch_flux_dev || !patch_cf_dev || !c_dev || !patch_delta_dev || !grad_dev || !nbr_grad_dev || !out_dev)
        return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    PatchCorrIn q{};
    q.scale = scale;
    const double* in[31];
    int m = 0;
    in[m++] = patch_flux_dev;
    for (int d = 0; d < 3; ++d) { in[m++] = q.pcf[d] = patch_cf_dev[d]; in[m++] = q.cc[d] = c_dev[d]; in[m++] = q.pd[d] = patch_delta_dev[d]; }
    for (int j = 0; j < 3 * n_rhs; ++j) { in[m++] = q.grad[j] = grad_dev[j]; in[m++] = q.nbr[j] = nbr_grad_dev[j]; }
    for (int j = 0; j < m; ++j) if (!in[j]) return fail(MI_ERR_ARG, std::string(who) + ": input arrays missing");
    CorrOut o{};
    for (int r = 0; r < n_rhs; ++r) {
        o.out[r] = out_dev[r];
        if (!o.out[r]) return fail(MI_ERR_ARG, std::string(who) + ": null output");
        for (int j = 0; j < m; ++j) if (o.out[r] == in[j]) return fail(MI_ERR_ARG, std::string(who) + ": an output must not alias an input");
        for (int s = 0; s < r; ++s) if (o.out[s] == o.out[r]) return fail(MI_ERR_ARG, std::string(who) + ": the outputs must differ");
    }
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_linear_upwind_corr<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(p->faceCells.p, patch_flux_dev, q, o, n_rhs, p->nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_lust_weights(mi_ctx_t c, int64_t n_faces, const double* cd_weights_dev, const double* face_flux_dev, double* weights_out_dev)
{
    if (!c || n_faces < 0 || !cd_weights_dev || !face_flux_dev || !weights_out_dev) return fail(MI_ERR_ARG, "mi_lust_weights: bad argument");
    if (!al16(cd_weights_dev) || !al16(face_flux_dev) || !al16(weights_out_dev)) return fail(MI_ERR_ARG, "mi_lust_weights: arrays must be 16-byte aligned");
    if (n_faces == 0) return MI_OK;
    return cell_launch(c, k_lust_weights, cd_weights_dev, face_flux_dev, weights_out_dev, n_faces);
}

// [fvm::ddt] + [fvm::div] - [fvm::laplacian] [+- fvm::Sp] [+- explicit terms] in one row pass (k_row_assemble)
namespace {
// the time form of one assembly: Euler (or no time derivative), or the inputs of backward / CrankNicolson / the local forms as their entry read them
struct TimeForm { int form; BackIn bw; CnIn cn; LocalIn loc; };
struct AsmOut { double *lower, *upper, *diag; double* const* source; double* sumMag; };
int assemble_impl(mi_addr_t a, const mi_fvm_terms* t, const TimeForm& tf, const mi_div_correction* corr, const AsmOut& o);
int n_rhs_held(const mi_fvm_terms* t) { return std::min(std::max(t->n_rhs, 0), 4); } // assemble_impl refuses a count outside 0..4
}
extern "C" int mi_fvm_assemble(mi_addr_t a, const mi_fvm_terms* t, double* lower_out_dev, double* upper_out_dev, double* diag_out_dev,
                               double* const* source_out_dev, double* sum_mag_off_diag_out_dev)
{
    return mi_fvm_assemble_corrected(a, t, nullptr, lower_out_dev, upper_out_dev, diag_out_dev, source_out_dev, sum_mag_off_diag_out_dev);
}
// ... with the explicit correction of linearUpwind / LUST in the div term (CORR)
extern "C" int mi_fvm_assemble_corrected(mi_addr_t a, const mi_fvm_terms* t, const mi_div_correction* corr, double* lower_out_dev, double* upper_out_dev,
                                         double* diag_out_dev, double* const* source_out_dev, double* sum_mag_off_diag_out_dev)
{
    return assemble_impl(a, t, TimeForm{TF_EULER, {}, {}, {}}, corr, {lower_out_dev, upper_out_dev, diag_out_dev, source_out_dev, sum_mag_off_diag_out_dev});
}
// ... with the backward time derivative in place of Euler's (BACK), with or without the correction
extern "C" int mi_fvm_assemble_backward(mi_addr_t a, const mi_fvm_terms* t, const mi_ddt_backward* bw, const mi_div_correction* corr, double* lower_out_dev,
                                        double* upper_out_dev, double* diag_out_dev, double* const* source_out_dev, double* sum_mag_off_diag_out_dev)
{
    if (!a || !t || !bw) return fail(MI_ERR_ARG, "mi_fvm_assemble_backward: bad argument");
    if (!t->ddt) return fail(MI_ERR_ARG, "mi_fvm_assemble_backward: terms->ddt is 0 (no time derivative: mi_fvm_assemble)");
    if ((bw->rho_old_old_dev != nullptr) != (t->rho_dev != nullptr)) return fail(MI_ERR_ARG, "mi_fvm_assemble_backward: rho, rho_old and rho_old_old go together");
    if (t->n_rhs > 0 && !bw->psi_old_old_dev) return fail(MI_ERR_ARG, "mi_fvm_assemble_backward: old-old fields missing");
    TimeForm tf{TF_BACK, {bw->coefft * t->r_delta_t, bw->coefft0, bw->coefft00, bw->rho_old_old_dev, {}}, {}, {}};
    for (int r = 0; r < n_rhs_held(t); ++r) tf.bw.psiOldOld[r] = bw->psi_old_old_dev[r];
    return assemble_impl(a, t, tf, corr, {lower_out_dev, upper_out_dev, diag_out_dev, source_out_dev, sum_mag_off_diag_out_dev});
}
// ... with the CrankNicolson time derivative (CN), with or without the correction: terms->r_delta_t carries rDtCoef
extern "C" int mi_fvm_assemble_cn(mi_addr_t a, const mi_fvm_terms* t, const mi_ddt_cn_terms* cn, const mi_div_correction* corr, double* lower_out_dev,
                                  double* upper_out_dev, double* diag_out_dev, double* const* source_out_dev, double* sum_mag_off_diag_out_dev)
{
    if (!a || !t || !cn) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: bad argument");
    if (!t->ddt) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: terms->ddt is 0 (no time derivative: mi_fvm_assemble)");
    if (!(cn->oc >= 0.0 && cn->oc <= 1.0)) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: the off-centring coefficient should be >= 0 and <= 1");
    if (t->n_rhs > 0 && !cn->ddt0_dev) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: ddt0 fields missing");
    TimeForm tf{TF_CN, {}, {cn->oc, cn->oc < 1.0 ? 1 : 0, {}}, {}};
    for (int r = 0; r < n_rhs_held(t); ++r) tf.cn.ddt0[r] = cn->ddt0_dev[r];
    return assemble_impl(a, t, tf, corr, {lower_out_dev, upper_out_dev, diag_out_dev, source_out_dev, sum_mag_off_diag_out_dev});
}
// ... with the local-time-step derivative (localEuler / CoEuler: rDeltaT a cell field) and / or the bounded Gauss convection (LOCAL), with or
// without the correction
extern "C" int mi_fvm_assemble_local(mi_addr_t a, const mi_fvm_terms* t, const mi_fvm_local_terms* loc, const mi_div_correction* corr, double* lower_out_dev,
                                     double* upper_out_dev, double* diag_out_dev, double* const* source_out_dev, double* sum_mag_off_diag_out_dev)
{
    const char* who = "mi_fvm_assemble_local";
    if (!a || !t || !loc) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!loc->r_delta_t_dev && !loc->div_flux_dev) return fail(MI_ERR_ARG, std::string(who) + ": neither r_delta_t_dev nor div_flux_dev (use mi_fvm_assemble)");
    if (loc->r_delta_t_dev && !t->ddt) return fail(MI_ERR_ARG, std::string(who) + ": r_delta_t_dev with terms->ddt == 0 (steadyState takes no rDeltaT field)");
    if (loc->div_flux_dev && !t->div_flux_dev && !faceless(a)) return fail(MI_ERR_ARG, std::string(who) + ": bounded (div_flux_dev) without a convection term (terms->div_flux_dev is NULL)");
    if (loc->div_flux_dev && !t->vol_dev) return fail(MI_ERR_ARG, std::string(who) + ": cell volumes needed");
    for (const double* q : {loc->r_delta_t_dev, loc->div_flux_dev}) {
        if (!q) continue;
        bool hit = q == lower_out_dev || q == upper_out_dev || q == diag_out_dev || q == sum_mag_off_diag_out_dev;
        for (int r = 0; source_out_dev && r < n_rhs_held(t); ++r) hit = hit || q == source_out_dev[r];
        if (hit) return fail(MI_ERR_ARG, std::string(who) + ": r_delta_t_dev / div_flux_dev must not be an output");
    }
    TimeForm tf{TF_LOCAL, {}, {}, {loc->r_delta_t_dev, loc->div_flux_dev}};
    return assemble_impl(a, t, tf, corr, {lower_out_dev, upper_out_dev, diag_out_dev, source_out_dev, sum_mag_off_diag_out_dev});
}
namespace {
// the argument block of one kernel variant, built once as that variant's own type, and its launch; everything was checked by assemble_impl
template <bool DIV, bool LAP, bool CORR, int TF>
int asm_launch(mi_addr_s* a, const mi_fvm_terms* t, const TimeForm& tf, const CorrIn& corr, const AsmOut& o)
{
    typename AsmSel<CORR, TF>::type ra{};
    ra.flux = t->div_flux_dev; ra.w = t->div_weights_dev; ra.delta = t->lap_delta_coeffs_dev; ra.gam = t->lap_gamma_magsf_dev;
    ra.lowerOut = o.lower; ra.upperOut = o.upper; ra.diagOut = o.diag; ra.sumMagOut = o.sumMag;
    ra.ddt = t->ddt ? 1 : 0; ra.rdt = t->r_delta_t; ra.rhoValue = t->rho_value; ra.rho = t->rho_dev; ra.rhoOld = t->rho_old_dev; ra.vol = t->vol_dev;
    ra.sp = t->sp_dev; ra.spMinus = t->sp_sign < 0 ? 1 : 0;
    ra.nRhs = t->n_rhs; ra.nSu = t->n_su;
    for (int r = 0; r < t->n_rhs; ++r) { ra.psiOld[r] = t->ddt ? t->psi_old_dev[r] : nullptr; ra.sourceOut[r] = o.source[r]; }
    for (int k = 0; k < t->n_su; ++k) ra.suMinus[k] = t->su_sign[k] < 0 ? 1 : 0;
    for (int j = 0; j < t->n_su * t->n_rhs; ++j) ra.su[j] = t->su_dev[j];
    if constexpr (CORR) { ra.lo = a->lowerAddr.p; ra.up = a->upperAddr.p; ra.corr = corr; }
    if constexpr (TF == TF_BACK) ra.bw = tf.bw;
    if constexpr (TF == TF_CN) ra.cn = tf.cn;
    if constexpr (TF == TF_LOCAL) ra.loc = tf.loc;
    ra.os = a->ownerStartC.p; ra.ls = a->losortStartC.p; ra.losort = a->losortC.p;
    ra.row16 = a->row16.p; ra.losort16 = a->losort16.p; ra.esc = a->rowEsc.p; ra.escStart = a->rowEscStart.p;
    const mi_addr_s::RowPlan& rp = a->rowPlan[0];
    ra.blockStart = rp.tiles ? a->tileCellStart.p : nullptr;
    const int arrays = (DIV ? 2 : 0) + (LAP ? 1 : 0) + (CORR ? t->n_rhs : 0);
    ra.n = a->L.nCells; ra.cap = row_cap(rp, arrays); ra.xcd = a->ctx->xcdRows;
    const size_t lds = (size_t)arrays * ra.cap * sizeof(double);
    return for_row_shape(a, rp, [&](auto s) { return row_launch(a, rp, k_row_assemble<DIV, LAP, decltype(s)::bs, decltype(s)::r16, CORR, TF>, ra, lds); });
}
// the five (DIV, LAP, CORR) cases of one time form
template <int TF>
int asm_launch_tf(bool DIV, bool LAP, bool CORR, mi_addr_s* a, const mi_fvm_terms* t, const TimeForm& tf, const CorrIn& corr, const AsmOut& o)
{
    if (CORR && LAP) return asm_launch<true, true, true, TF>(a, t, tf, corr, o);
    if (CORR) return asm_launch<true, false, true, TF>(a, t, tf, corr, o);
    if (DIV && LAP) return asm_launch<true, true, false, TF>(a, t, tf, corr, o);
    if (DIV) return asm_launch<true, false, false, TF>(a, t, tf, corr, o);
    return asm_launch<false, true, false, TF>(a, t, tf, corr, o);
}
int assemble_impl(mi_addr_t a, const mi_fvm_terms* t, const TimeForm& tf, const mi_div_correction* corr, const AsmOut& o)
{
    if (!a || !t || !o.diag) return fail(MI_ERR_ARG, "mi_fvm_assemble: bad argument");
    // a face term is present when its array is given.  A mesh without faces (one_cell, no_faces: tests/test_degenerate_meshes.py) gives every
    // face array empty and maybe NULL: its face terms are all taken as present and empty -- no face is read or written, every row sum is
    // +0.0 as in the unfused sequence -- and the checks of the face arrays do not apply
    const bool noFaces = faceless(a);
    const bool DIV = t->div_flux_dev != nullptr || noFaces, LAP = t->lap_delta_coeffs_dev != nullptr || noFaces;
    if (LAP && !t->lap_gamma_magsf_dev && !noFaces) return fail(MI_ERR_ARG, "mi_fvm_assemble: laplacian needs deltaCoeffs and gammaMagSf");
    if (!DIV && !LAP) return fail(MI_ERR_ARG, "mi_fvm_assemble: no face term (use mi_fvm_ddt_euler* for a diagonal matrix)");
    if (!noFaces && (!o.upper || (DIV && !o.lower))) return fail(MI_ERR_ARG, "mi_fvm_assemble: coefficient outputs missing (a convection term makes the matrix asymmetric)");
    if (t->n_rhs < 0 || t->n_rhs > 4 || t->n_su < 0 || t->n_su > 4) return fail(MI_ERR_ARG, "mi_fvm_assemble: at most 4 right-hand sides and 4 explicit terms");
    if ((t->ddt || t->sp_dev || t->n_su > 0) && !t->vol_dev) return fail(MI_ERR_ARG, "mi_fvm_assemble: cell volumes needed");
    if (t->ddt && ((t->rho_dev != nullptr) != (t->rho_old_dev != nullptr))) return fail(MI_ERR_ARG, "mi_fvm_assemble: rho and rho_old go together");
    if (t->n_rhs > 0 && (!o.source || (t->ddt && !t->psi_old_dev))) return fail(MI_ERR_ARG, "mi_fvm_assemble: source outputs / old fields missing");
    if (t->n_su > 0 && (!t->su_dev || !t->su_sign || t->n_rhs == 0)) return fail(MI_ERR_ARG, "mi_fvm_assemble: explicit terms need su_dev, su_sign and a right-hand side");
    const double* faceIn[4] = {t->div_flux_dev, t->div_weights_dev, t->lap_delta_coeffs_dev, t->lap_gamma_magsf_dev};
    for (const double* q : faceIn) {
        if (q && !al16(q)) return fail(MI_ERR_ARG, "mi_fvm_assemble: face fields must be 16-byte aligned");
        if (q && !noFaces && (q == o.upper || q == o.lower)) return fail(MI_ERR_ARG, "mi_fvm_assemble: a coefficient output must not alias an input (cut faces are recomputed from the inputs)");
    }
    if (o.lower && o.lower == o.upper) return fail(MI_ERR_ARG, "mi_fvm_assemble: lower_out and upper_out must differ");
    const bool CORR = corr != nullptr && !noFaces;        // no face: nothing to correct, the correction's face arrays are empty
    if (CORR) {
        const char* who = "mi_fvm_assemble_corrected";
        if (!DIV) return fail(MI_ERR_ARG, std::string(who) + ": a convection correction without a convection term (div_flux_dev is NULL)");
        if (a->L.nExt > 0)
            return fail(MI_ERR_ARG, std::string(who) + ": the addressing has coupled patches, whose correction faces the reference adds before the "
                        "division by V -- use the unfused path (mi_linear_upwind_correction + mi_patch_linear_upwind_correction + mi_surface_integrate + "
                        "mi_patch_add + mi_vec_div + mi_vec_submul)");
        if (t->n_rhs < 1 || !t->vol_dev) return fail(MI_ERR_ARG, std::string(who) + ": the correction needs n_rhs >= 1 right-hand sides and the cell volumes");
    }
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    CorrIn ci{};
    if (CORR) {
        const double* outs[8] = {o.lower, o.upper, o.diag, o.sumMag};
        for (int r = 0; r < t->n_rhs; ++r) outs[4 + r] = o.source[r];
        MICHK(corr_in("mi_fvm_assemble_corrected", corr, t->n_rhs, ci, outs, 4 + t->n_rhs));
    }
    if (a->L.nCells == 0) return MI_OK;
    for (int r = 0; r < t->n_rhs; ++r)
        if (!o.source[r] || (t->ddt && !t->psi_old_dev[r])) return fail(MI_ERR_ARG, "mi_fvm_assemble: null right-hand side array");
    if (tf.form == TF_BACK)
        for (int r = 0; r < t->n_rhs; ++r)
            if (!tf.bw.psiOldOld[r]) return fail(MI_ERR_ARG, "mi_fvm_assemble_backward: null old-old field");
    if (tf.form == TF_CN)
        for (int r = 0; r < t->n_rhs; ++r) {
            const double* d = tf.cn.ddt0[r];
            if (!d) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: null ddt0 field");
            if (d == o.lower || d == o.upper || d == o.diag || d == o.sumMag) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: a ddt0 field must not be an output");
            for (int q = 0; q < t->n_rhs; ++q) if (d == o.source[q]) return fail(MI_ERR_ARG, "mi_fvm_assemble_cn: a ddt0 field must not be an output");
        }
    for (int j = 0; j < t->n_su * t->n_rhs; ++j)
        if (!t->su_dev[j]) return fail(MI_ERR_ARG, "mi_fvm_assemble: null explicit term");
    if (tf.form == TF_BACK) return asm_launch_tf<TF_BACK>(DIV, LAP, CORR, a, t, tf, ci, o);
    if (tf.form == TF_CN) return asm_launch_tf<TF_CN>(DIV, LAP, CORR, a, t, tf, ci, o);
    if (tf.form == TF_LOCAL) return asm_launch_tf<TF_LOCAL>(DIV, LAP, CORR, a, t, tf, ci, o);
    return asm_launch_tf<TF_EULER>(DIV, LAP, CORR, a, t, tf, ci, o);
}
} // namespace

extern "C" int mi_surface_integrate(mi_addr_t a, const double* ssf_dev, const double* vol_dev_or_null, double* ivf_dev)
{
    if (!a || (!ssf_dev && !faceless(a)) || !ivf_dev) return fail(MI_ERR_ARG, "mi_surface_integrate: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    return row_sum<M_PLUS, M_MINUS>(a, ssf_dev, ssf_dev, nullptr, vol_dev_or_null, ivf_dev);
}

extern "C" int mi_face_interpolate(mi_addr_t a, const double* lambda_dev, const double* phi_dev, double* sf_dev)
{
    if (!a || !phi_dev || (!faceless(a) && (!lambda_dev || !sf_dev))) return fail(MI_ERR_ARG, "mi_face_interpolate: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    k_face_interpolate<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, lambda_dev, phi_dev, sf_dev, a->L.nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// gaussConvectionScheme::fvcDiv (gaussConvectionScheme.C:117-140): fvc::surfaceIntegrate(faceFlux*interpolate(faceFlux, vf)) -- one face pass
// (the reference: weights, interpolate, product = three field passes) + the row sum of surfaceIntegrate
extern "C" int mi_fvc_div(mi_addr_t a, const double* face_flux_dev, const double* weights_dev_or_null, const double* vf_dev, const double* vol_dev_or_null,
                          double* face_out_dev, double* div_out_dev)
{
    if (!a || !vf_dev || !div_out_dev || (!faceless(a) && (!face_flux_dev || !face_out_dev))) return fail(MI_ERR_ARG, "mi_fvc_div: bad argument");
    if (!faceless(a) && (face_out_dev == face_flux_dev || face_out_dev == weights_dev_or_null)) return fail(MI_ERR_ARG, "mi_fvc_div: face_out must not alias a face input");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces > 0) {
        k_face_conv_flux<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, weights_dev_or_null, face_flux_dev, vf_dev, face_out_dev, a->L.nFaces);
        HIPCHK(hipGetLastError());
    }
    return row_sum<M_PLUS, M_MINUS>(a, face_out_dev, face_out_dev, nullptr, vol_dev_or_null, div_out_dev);
}

// gaussLaplacianScheme<Type, scalar>::fvmLaplacian, explicit non-orthogonal correction (gaussLaplacianSchemes.C:64-90)
extern "C" int mi_sngrad_correction_flux(mi_addr_t a, const double* cvx_dev, const double* cvy_dev, const double* cvz_dev, const double* weights_dev,
                                         const double* gx_dev, const double* gy_dev, const double* gz_dev, const double* gamma_magsf_dev_or_null,
                                         double* flux_out_dev)
{
    if (!a || !cvx_dev || !cvy_dev || !cvz_dev || !weights_dev || !gx_dev || !gy_dev || !gz_dev || !flux_out_dev)
        return fail(MI_ERR_ARG, "mi_sngrad_correction_flux: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    k_sngrad_corr_flux<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, cvx_dev, cvy_dev, cvz_dev, weights_dev, gx_dev, gy_dev,
                                                                                  gz_dev, gamma_magsf_dev_or_null, flux_out_dev, a->L.nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_patch_sngrad_correction_flux(mi_patch_t p, const double* cvx_dev, const double* cvy_dev, const double* cvz_dev, const double* weights_dev,
                                               const double* gx_dev, const double* gy_dev, const double* gz_dev, const double* nbr_gx_dev,
                                               const double* nbr_gy_dev, const double* nbr_gz_dev, const double* gamma_magsf_dev_or_null, double* flux_out_dev)
{
    if (!p) return fail(MI_ERR_ARG, "mi_patch_sngrad_correction_flux: bad argument");
    if (p->nFaces == 0) return MI_OK;
    if (!cvx_dev || !cvy_dev || !cvz_dev || !weights_dev || !gx_dev || !gy_dev || !gz_dev || !nbr_gx_dev || !nbr_gy_dev || !nbr_gz_dev || !flux_out_dev)
        return fail(MI_ERR_ARG, "mi_patch_sngrad_correction_flux: bad argument");
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_sngrad_corr_flux<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(p->faceCells.p, cvx_dev, cvy_dev, cvz_dev, weights_dev, gx_dev, gy_dev, gz_dev,
                                                                                 nbr_gx_dev, nbr_gy_dev, nbr_gz_dev, gamma_magsf_dev_or_null, flux_out_dev, p->nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// ---- the `limited` snGrad scheme: parser (host only) and the two face passes --------------------------------------------------
extern "C" int mi_sngrad_parse(const char* text, mi_sngrad_scheme* out)
{
    const std::string who = "mi_sngrad_parse";
    if (!text || !out) return fail(MI_ERR_ARG, who + ": bad argument");
    const std::vector<std::string> tok = scheme_words(text);
    if (tok.empty()) return fail(MI_ERR_ARG, who + ": empty scheme");
    const char* const plain[] = {"uncorrected", "orthogonal", "corrected"};     // MI_SNGRAD_UNCORRECTED, _ORTHOGONAL, _CORRECTED
    auto plain_kind = [&](const std::string& s) { for (int k = 0; k < 3; ++k) if (s == plain[k]) return k; return -1; };
    mi_sngrad_scheme s{};
    s.limit_coeff = 1.0;                                         // limitedSnGrad.H:122-127; read by the limited kind only
    if (plain_kind(tok[0]) >= 0) {
        if (tok.size() > 1) return fail(MI_ERR_ARG, who + ": extra '" + tok[1] + "' after '" + tok[0] + "'");
        s.kind = plain_kind(tok[0]);
        *out = s;
        return MI_OK;
    }
    if (tok[0] != "limited") return fail(MI_ERR_ARG, who + ": snGrad scheme '" + tok[0] + "' is not supported (uncorrected | orthogonal | corrected | limited [corrected] <k>)");
    if (tok.size() < 2) return fail(MI_ERR_ARG, who + ": 'limited' needs a coefficient ('limited <k>' | 'limited corrected <k>')");
    // limitedSnGrad.H:86-110: a number directly after `limited` is the coefficient over `corrected`; otherwise a scheme, then the coefficient
    std::size_t at = 1;
    double k = 0;
    if (!scheme_number(tok[1], k)) {
        if (tok[1] == "limited") return fail(MI_ERR_ARG, who + ": a limited scheme over a limited scheme ('limited limited') is not supported");
        if (tok[1] == "uncorrected" || tok[1] == "orthogonal")
            return fail(MI_ERR_ARG, who + ": 'limited " + tok[1] + "' is not supported: the correction() of '" + tok[1] + "' is not implemented in the reference");
        if (tok[1] != "corrected") return fail(MI_ERR_ARG, who + ": corrected scheme '" + tok[1] + "' under 'limited' is not supported (only corrected)");
        if (tok.size() < 3) return fail(MI_ERR_ARG, who + ": 'limited corrected' needs the coefficient k");
        if (!scheme_number(tok[2], k)) return fail(MI_ERR_ARG, who + ": '" + tok[2] + "' is not a number");
        at = 2;
    }
    if (tok.size() > at + 1) return fail(MI_ERR_ARG, who + ": extra '" + tok[at + 1] + "'");
    if (!(k >= 0 && k <= 1)) return fail(MI_ERR_ARG, who + ": limitCoeff is specified as " + tok[at] + " but should be >= 0 && <= 1");
    s.kind = MI_SNGRAD_LIMITED; s.limit_coeff = k;
    *out = s;
    return MI_OK;
}
namespace {
// the checks both limited passes share; fills the argument block.  in[]: every input array, for the aliasing test
template <int NCOMP>
int sngrad_limited_args(const std::string& who, double k, const double* cvx, const double* cvy, const double* cvz, const double* w, const double* dc,
                        const double* const* vf, const double* const* g, const double* const* nbrVf, const double* const* nbrG, const double* gamma,
                        double* const* flux, double* limiter, int n, SnGradLimArgs<NCOMP>& a, SnGradNbrArgs<NCOMP>& nb)
{
    const double* in[6 + 8 * NCOMP];
    int m = 0;
    for (const double* q : {cvx, cvy, cvz, w, dc}) { if (!q) return fail(MI_ERR_ARG, who + ": a face array is missing"); in[m++] = q; }
    for (int j = 0; j < NCOMP; ++j) in[m++] = vf[j];
    for (int i = 0; i < 3 * NCOMP; ++i) in[m++] = g[i];
    if (nbrVf) { for (int j = 0; j < NCOMP; ++j) in[m++] = nbrVf[j]; for (int i = 0; i < 3 * NCOMP; ++i) in[m++] = nbrG[i]; }
    for (int i = 0; i < m; ++i) if (!in[i]) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (gamma) in[m++] = gamma;
    for (int i = 0; i < m; ++i) if (!al8(in[i])) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
    double* outs[NCOMP + 1];
    int no = 0;
    for (int j = 0; j < NCOMP; ++j) outs[no++] = flux[j];
    if (limiter) outs[no++] = limiter;
    for (int i = 0; i < no; ++i) {
        if (!outs[i]) return fail(MI_ERR_ARG, who + ": an output array is missing");
        if (!al8(outs[i])) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
        for (int q = 0; q < m; ++q) if (outs[i] == in[q]) return fail(MI_ERR_ARG, who + ": an output must not alias an input");
        for (int q = 0; q < i; ++q) if (outs[i] == outs[q]) return fail(MI_ERR_ARG, who + ": the outputs must differ");
    }
    a.cvx = cvx; a.cvy = cvy; a.cvz = cvz; a.lambda = w; a.deltaCoeffs = dc; a.gammaMagSf = gamma; a.limiter = limiter;
    a.k = k; a.oneMinusK = 1 - k; a.n = n;
    for (int j = 0; j < NCOMP; ++j) { a.vf[j] = vf[j]; a.flux[j] = flux[j]; if (nbrVf) nb.vf[j] = nbrVf[j]; }
    for (int i = 0; i < 3 * NCOMP; ++i) { a.g[i] = g[i]; if (nbrVf) nb.g[i] = nbrG[i]; }
    return MI_OK;
}
template <int NCOMP>
int sngrad_limited_internal(const std::string& who, mi_addr_s* a, double k, const double* cvx, const double* cvy, const double* cvz, const double* w,
                            const double* dc, const double* const* vf, const double* const* g, const double* gamma, double* const* flux, double* limiter)
{
    SnGradLimArgs<NCOMP> q{}; SnGradNbrArgs<NCOMP> none{};
    MICHK(sngrad_limited_args<NCOMP>(who, k, cvx, cvy, cvz, w, dc, vf, g, nullptr, nullptr, gamma, flux, limiter, a->L.nFaces, q, none));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    k_sngrad_limited_flux<NCOMP><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
template <int NCOMP>
int sngrad_limited_patch(const std::string& who, mi_patch_s* p, double k, const double* cvx, const double* cvy, const double* cvz, const double* w,
                         const double* dc, const double* const* vf, const double* const* nbrVf, const double* const* g, const double* const* nbrG,
                         const double* gamma, double* const* flux, double* limiter)
{
    SnGradLimArgs<NCOMP> q{}; SnGradNbrArgs<NCOMP> nb{};
    MICHK(sngrad_limited_args<NCOMP>(who, k, cvx, cvy, cvz, w, dc, vf, g, nbrVf, nbrG, gamma, flux, limiter, p->nFaces, q, nb));
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_sngrad_limited_flux<NCOMP><<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(p->faceCells.p, q, nb);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
int sngrad_limited_common(const std::string& who, bool handle, int32_t n_comp, double k, bool tables)
{
    if (!handle) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n_comp != 1 && n_comp != 3) return fail(MI_ERR_ARG, who + ": n_comp must be 1 or 3");
    if (!(k >= 0 && k <= 1)) return fail(MI_ERR_ARG, who + ": limit_coeff should be >= 0 && <= 1");
    if (!tables) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    return MI_OK;
}
} // namespace
extern "C" int mi_sngrad_limited_correction_flux(mi_addr_t a, int32_t n_comp, double limit_coeff, const double* cvx_dev, const double* cvy_dev,
                                                 const double* cvz_dev, const double* weights_dev, const double* delta_coeffs_dev,
                                                 const double* const* vf_dev, const double* const* grad_dev, const double* gamma_magsf_dev_or_null,
                                                 double* const* flux_out_dev, double* limiter_out_dev_or_null)
{
    const std::string who = "mi_sngrad_limited_correction_flux";
    MICHK(sngrad_limited_common(who, a != nullptr, n_comp, limit_coeff, vf_dev && grad_dev && flux_out_dev));
    if (n_comp == 1) return sngrad_limited_internal<1>(who, a, limit_coeff, cvx_dev, cvy_dev, cvz_dev, weights_dev, delta_coeffs_dev, vf_dev, grad_dev,
                                                      gamma_magsf_dev_or_null, flux_out_dev, limiter_out_dev_or_null);
    return sngrad_limited_internal<3>(who, a, limit_coeff, cvx_dev, cvy_dev, cvz_dev, weights_dev, delta_coeffs_dev, vf_dev, grad_dev,
                                      gamma_magsf_dev_or_null, flux_out_dev, limiter_out_dev_or_null);
}
extern "C" int mi_patch_sngrad_limited_correction_flux(mi_patch_t p, int32_t n_comp, double limit_coeff, const double* cvx_dev, const double* cvy_dev,
                                                       const double* cvz_dev, const double* weights_dev, const double* delta_coeffs_dev,
                                                       const double* const* vf_dev, const double* const* nbr_vf_dev, const double* const* grad_dev,
                                                       const double* const* nbr_grad_dev, const double* gamma_magsf_dev_or_null,
                                                       double* const* flux_out_dev, double* limiter_out_dev_or_null)
{
    const std::string who = "mi_patch_sngrad_limited_correction_flux";
    MICHK(sngrad_limited_common(who, p != nullptr, n_comp, limit_coeff, vf_dev && nbr_vf_dev && grad_dev && nbr_grad_dev && flux_out_dev));
    if (p->nFaces == 0) return MI_OK;
    if (n_comp == 1) return sngrad_limited_patch<1>(who, p, limit_coeff, cvx_dev, cvy_dev, cvz_dev, weights_dev, delta_coeffs_dev, vf_dev, nbr_vf_dev, grad_dev,
                                                   nbr_grad_dev, gamma_magsf_dev_or_null, flux_out_dev, limiter_out_dev_or_null);
    return sngrad_limited_patch<3>(who, p, limit_coeff, cvx_dev, cvy_dev, cvz_dev, weights_dev, delta_coeffs_dev, vf_dev, nbr_vf_dev, grad_dev,
                                   nbr_grad_dev, gamma_magsf_dev_or_null, flux_out_dev, limiter_out_dev_or_null);
}
extern "C" int mi_patch_internal_field(mi_patch_t p, const double* psi_dev, double* out_dev)
{
    if (!p || (p->nFaces > 0 && (!psi_dev || !out_dev))) return fail(MI_ERR_ARG, "mi_patch_internal_field: bad argument");
    if (p->nFaces == 0) return MI_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_internal_field<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(p->faceCells.p, psi_dev, out_dev, p->nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_vec_submul(mi_ctx_t c, int64_t n, const double* x_dev, const double* y_dev, double* inout_dev)
{
    if (!c || n < 0 || (n > 0 && (!x_dev || !y_dev || !inout_dev))) return fail(MI_ERR_ARG, "mi_vec_submul: bad argument");
    if (!al16(x_dev) || !al16(y_dev) || !al16(inout_dev)) return fail(MI_ERR_ARG, "mi_vec_submul: arrays must be 16-byte aligned");
    if (n == 0) return MI_OK;
    return cell_launch(c, k_submul, x_dev, y_dev, inout_dev, n);
}

// fvMatrix<Type>::relax(alpha) (fvMatrix.C:1087-1345): one diagonal, n_rhs sources / solution components (the vector equation's
// S += (D - D0)*psi per component).  sum_mag_off_diag given (mi_fvm_assemble's by-product): the sumMagOffDiag row pass is skipped and
// the array is completed in place with the coupled patches' |boundaryCoeffs|.
extern "C" int mi_relax_multi(mi_addr_t a, double alpha, double* diag_dev, const double* lower_dev, const double* upper_dev,
                              double* sum_mag_off_diag_dev, int32_t n_rhs, double* const* source_dev, const double* const* psi_dev,
                              int32_t n_patches, const mi_patch_t* patches, const double* const* internal_coeffs_dev,
                              const double* const* boundary_coeffs_dev, const int32_t* coupled)
{
    if (!a || !diag_dev || (!upper_dev && !sum_mag_off_diag_dev) || n_rhs < 0 || (n_rhs > 0 && (!source_dev || !psi_dev)) || n_patches < 0)
        return fail(MI_ERR_ARG, "mi_relax: bad argument");
    for (int32_t r = 0; r < n_rhs; ++r) if (!source_dev[r] || !psi_dev[r]) return fail(MI_ERR_ARG, "mi_relax: null source / psi");
    if (alpha <= 0) return MI_OK;
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = a->L.nCells;
    if (a->relaxD0.n != (size_t)n) { MICHK(a->relaxD0.alloc((size_t)n)); MICHK(a->relaxSumOff.alloc((size_t)n)); }
    HIPCHK(hipMemcpyAsync(a->relaxD0.p, diag_dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    double* sumOff = sum_mag_off_diag_dev;
    if (!sumOff) {
        sumOff = a->relaxSumOff.p;
        HIPCHK(hipMemsetAsync(sumOff, 0, sizeof(double) * (size_t)n, s));
        MICHK(mi_row_face_op(a, ROW_SUMMAGOFFDIAG, lower_dev, upper_dev, sumOff));
    }
    for (int32_t p = 0; p < n_patches; ++p) {
        if (!patches[p] || patches[p]->nFaces == 0) continue;
        if (coupled && coupled[p]) {
            MICHK(mi_patch_add(patches[p], internal_coeffs_dev[p], diag_dev, 0));
            MICHK(mi_patch_add(patches[p], boundary_coeffs_dev[p], sumOff, 2));
        } else MICHK(mi_patch_add(patches[p], internal_coeffs_dev[p], diag_dev, 2));
    }
    MICHK(cell_launch(c, k_relax_dominance, diag_dev, sumOff, alpha, n));
    for (int32_t p = 0; p < n_patches; ++p) {
        if (!patches[p] || patches[p]->nFaces == 0) continue;
        MICHK(mi_patch_add(patches[p], internal_coeffs_dev[p], diag_dev, 1));
    }
    for (int32_t r = 0; r < n_rhs; ++r) MICHK(cell_launch(c, k_relax_source, source_dev[r], diag_dev, a->relaxD0.p, psi_dev[r], n));
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_relax(mi_addr_t a, double alpha, double* diag_dev, const double* lower_dev, const double* upper_dev,
                        double* source_dev, const double* psi_dev, int32_t n_patches, const mi_patch_t* patches,
                        const double* const* internal_coeffs_dev, const double* const* boundary_coeffs_dev, const int32_t* coupled)
{
    if (!a || !diag_dev || !upper_dev || !source_dev || !psi_dev || n_patches < 0) return fail(MI_ERR_ARG, "mi_relax: bad argument");
    double* src[1] = {source_dev}; const double* psi[1] = {psi_dev};
    return mi_relax_multi(a, alpha, diag_dev, lower_dev, upper_dev, nullptr, 1, src, psi, n_patches, patches, internal_coeffs_dev, boundary_coeffs_dev, coupled);
}

// fvMatrix::setReference (fvMatrix.C:964-981): source[celli] += diag[celli]*value (host arithmetic in the reference: the product is
// rounded, then added); diag[celli] = 2*diag[celli]
__global__ void k_set_reference(int32_t celli, double value, double* __restrict__ diag, double* __restrict__ source)
{
    const double t = diag[celli] * value;
    source[celli] = source[celli] + t;
    diag[celli] = 2 * diag[celli];
}
extern "C" int mi_fvm_set_reference(mi_addr_t a, int32_t celli, double value, double* diag_dev, double* source_dev)
{
    if (!a || !diag_dev || !source_dev || celli >= a->L.nCells) return fail(MI_ERR_ARG, "mi_fvm_set_reference: bad argument");
    if (celli < 0) return MI_OK;      // "celli >= 0" of the reference: a rank that does not hold the reference cell
    HIPCHK(hipSetDevice(a->ctx->device));
    k_set_reference<<<1, 1, 0, a->ctx->stream>>>(celli, value, diag_dev, source_dev);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// fvMatrix::setValues (fvMatrix.C:454-656; functors :352-452)
__global__ void k_set_values_cells(const int32_t* __restrict__ labels, const double* __restrict__ values, int nSet, double* __restrict__ psi,
                                   const double* __restrict__ diag, double* __restrict__ source, uint8_t* __restrict__ mask, double* __restrict__ val)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nSet; i += gridDim.x * blockDim.x) {
        const int c = labels[i];
        const double v = values[i];
        psi[c] = v; source[c] = v * diag[c]; mask[c] = 1; val[c] = v;
    }
}
template <bool UPSTREAM>
__global__ void k_set_values_rows(const int32_t* __restrict__ os, const int32_t* __restrict__ ls, const int32_t* __restrict__ losort,
                                  const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const uint8_t* __restrict__ mask,
                                  const double* __restrict__ val, const double* __restrict__ U, const double* __restrict__ L,
                                  double* __restrict__ source, int n)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || mask[c]) return;
    double out = source[c];
    for (int j = os[c]; j < os[c + 1]; ++j) { const int nb = up[j]; if (mask[nb]) out = fma(-(UPSTREAM ? U[j] : L[j]), val[nb], out); }
    for (int j = ls[c]; j < ls[c + 1]; ++j) { const int g = losort[j], ow = lo[g]; if (mask[ow]) out = fma(-(UPSTREAM ? L[g] : U[g]), val[ow], out); }
    source[c] = out;
}
template <bool UPSTREAM>
__global__ void k_set_values_faces(const int32_t* __restrict__ lo, const int32_t* __restrict__ up, const uint8_t* __restrict__ mask,
                                   const double* __restrict__ U, const double* __restrict__ L, double* __restrict__ Uo, double* __restrict__ Lo, int nf)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += gridDim.x * blockDim.x) {
        const bool oS = mask[lo[f]] != 0, nS = mask[up[f]] != 0;
        const double u = U[f], l = L[f];
        Uo[f] = (UPSTREAM ? (oS || nS) : oS) ? 0.0 : u;
        Lo[f] = (UPSTREAM ? (oS || nS) : nS) ? 0.0 : l;
    }
}
__global__ void k_set_values_patch(const int32_t* __restrict__ faceCells, const uint8_t* __restrict__ mask, double* __restrict__ ic, double* __restrict__ bc, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && mask[faceCells[i]]) { ic[i] = 0.0; bc[i] = 0.0; }
}
extern "C" int mi_fvm_set_values(mi_addr_t a, int32_t n_set, const int32_t* cell_labels_dev, const double* values_dev, int32_t upstream_semantics,
                                 double* psi_dev, const double* diag_dev, double* source_dev, const double* upper_in_dev, const double* lower_in_dev,
                                 double* upper_out_dev, double* lower_out_dev, int32_t n_patches, const mi_patch_t* patches,
                                 double* const* internal_coeffs_dev, double* const* boundary_coeffs_dev)
{
    if (!a || n_set < 0 || !psi_dev || !diag_dev || !source_dev || !upper_in_dev || !upper_out_dev || !lower_out_dev || n_patches < 0 ||
        (n_set > 0 && (!cell_labels_dev || !values_dev)))
        return fail(MI_ERR_ARG, "mi_fvm_set_values: bad argument");
    if (upper_out_dev == lower_out_dev) return fail(MI_ERR_ARG, "mi_fvm_set_values: upper_out and lower_out must differ (the result is asymmetric)");
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    MICHK(ensure_caller_tables(a));
    hipStream_t s = c->stream;
    const int n = a->L.nCells, nf = a->L.nFaces;
    if (a->setMask.n != (size_t)n) { MICHK(a->setMask.alloc((size_t)n)); MICHK(a->setVal.alloc((size_t)n)); }
    HIPCHK(hipMemsetAsync(a->setMask.p, 0, (size_t)n, s));
    const double* L = lower_in_dev ? lower_in_dev : upper_in_dev;
    if (n_set > 0) k_set_values_cells<<<grid_for(c, n_set), 256, 0, s>>>(cell_labels_dev, values_dev, n_set, psi_dev, diag_dev, source_dev, a->setMask.p, a->setVal.p);
    if (n > 0) {
        if (upstream_semantics) k_set_values_rows<true><<<(n + 255) / 256, 256, 0, s>>>(a->ownerStartC.p, a->losortStartC.p, a->losortC.p, a->lowerAddr.p, a->upperAddr.p, a->setMask.p, a->setVal.p, upper_in_dev, L, source_dev, n);
        else k_set_values_rows<false><<<(n + 255) / 256, 256, 0, s>>>(a->ownerStartC.p, a->losortStartC.p, a->losortC.p, a->lowerAddr.p, a->upperAddr.p, a->setMask.p, a->setVal.p, upper_in_dev, L, source_dev, n);
    }
    if (nf > 0) {
        if (upstream_semantics) k_set_values_faces<true><<<grid_for(c, nf), 256, 0, s>>>(a->lowerAddr.p, a->upperAddr.p, a->setMask.p, upper_in_dev, L, upper_out_dev, lower_out_dev, nf);
        else k_set_values_faces<false><<<grid_for(c, nf), 256, 0, s>>>(a->lowerAddr.p, a->upperAddr.p, a->setMask.p, upper_in_dev, L, upper_out_dev, lower_out_dev, nf);
    }
    for (int32_t p = 0; p < n_patches; ++p) {
        if (!patches[p] || patches[p]->nFaces == 0) continue;
        if (!internal_coeffs_dev || !boundary_coeffs_dev || !internal_coeffs_dev[p] || !boundary_coeffs_dev[p]) return fail(MI_ERR_ARG, "mi_fvm_set_values: patch coefficients missing");
        k_set_values_patch<<<(patches[p]->nFaces + 255) / 256, 256, 0, s>>>(patches[p]->faceCells.p, a->setMask.p, internal_coeffs_dev[p], boundary_coeffs_dev[p], patches[p]->nFaces);
    }
    HIPCHK(hipGetLastError());
    return MI_OK;
}


// ---- scheme front-end (SURVEY.md 8f rank 1) -----------------------------------------------------------------------
extern "C" int mi_fvm_ddt_euler(mi_ctx_t c, int64_t n, double r_delta_t, double rho, const double* vol_dev, const double* psi_old_dev,
                                double* diag_out_dev, double* source_out_dev)
{
    if (!c || n < 0 || !vol_dev || !psi_old_dev || !diag_out_dev || !source_out_dev) return fail(MI_ERR_ARG, "mi_fvm_ddt_euler: bad argument");
    if (!al16(vol_dev) || !al16(psi_old_dev) || !al16(diag_out_dev) || !al16(source_out_dev)) return fail(MI_ERR_ARG, "mi_fvm_ddt_euler: arrays must be 16-byte aligned");
    return cell_launch(c, k_ddt_euler, r_delta_t * rho, vol_dev, psi_old_dev, diag_out_dev, source_out_dev, n);
}
extern "C" int mi_fvm_ddt_euler_rho(mi_ctx_t c, int64_t n, double r_delta_t, const double* rho_dev, const double* rho_old_dev, const double* vol_dev,
                                    const double* psi_old_dev, double* diag_out_dev, double* source_out_dev)
{
    if (!c || n < 0 || !rho_dev || !rho_old_dev || !vol_dev || !psi_old_dev || !diag_out_dev || !source_out_dev) return fail(MI_ERR_ARG, "mi_fvm_ddt_euler_rho: bad argument");
    if (!al16(rho_dev) || !al16(rho_old_dev) || !al16(vol_dev) || !al16(psi_old_dev) || !al16(diag_out_dev) || !al16(source_out_dev))
        return fail(MI_ERR_ARG, "mi_fvm_ddt_euler_rho: arrays must be 16-byte aligned");
    return cell_launch(c, k_ddt_euler_rho, r_delta_t, rho_dev, rho_old_dev, vol_dev, psi_old_dev, diag_out_dev, source_out_dev, n);
}
extern "C" int mi_fvm_su(mi_ctx_t c, int64_t n, const double* vol_dev, const double* su_dev, double* source_inout_dev)
{
    if (!c || n < 0 || !vol_dev || !su_dev || !source_inout_dev) return fail(MI_ERR_ARG, "mi_fvm_su: bad argument");
    if (!al16(vol_dev) || !al16(su_dev) || !al16(source_inout_dev)) return fail(MI_ERR_ARG, "mi_fvm_su: arrays must be 16-byte aligned");
    return cell_launch(c, k_fvm_su, vol_dev, su_dev, source_inout_dev, n);
}
extern "C" int mi_fvm_sp(mi_ctx_t c, int64_t n, const double* vol_dev, const double* sp_dev_or_null, double sp_value, double* diag_inout_dev)
{
    if (!c || n < 0 || !vol_dev || !diag_inout_dev) return fail(MI_ERR_ARG, "mi_fvm_sp: bad argument");
    if (!al16(vol_dev) || (sp_dev_or_null && !al16(sp_dev_or_null)) || !al16(diag_inout_dev)) return fail(MI_ERR_ARG, "mi_fvm_sp: arrays must be 16-byte aligned");
    return cell_launch(c, k_fvm_sp, vol_dev, sp_dev_or_null, sp_value, diag_inout_dev, n);
}
extern "C" int mi_fvm_susp(mi_ctx_t c, int64_t n, const double* vol_dev, const double* susp_dev, const double* vf_dev, double* diag_inout_dev,
                           double* source_inout_dev)
{
    if (!c || n < 0 || !vol_dev || !susp_dev || !vf_dev || !diag_inout_dev || !source_inout_dev) return fail(MI_ERR_ARG, "mi_fvm_susp: bad argument");
    if (!al16(vol_dev) || !al16(susp_dev) || !al16(vf_dev) || !al16(diag_inout_dev) || !al16(source_inout_dev)) return fail(MI_ERR_ARG, "mi_fvm_susp: arrays must be 16-byte aligned");
    return cell_launch(c, k_fvm_susp, vol_dev, susp_dev, vf_dev, diag_inout_dev, source_inout_dev, n);
}
namespace {
int flux_args(mi_addr_t a, const char* who, const double* lambda_dev, const double* sfx_dev, const double* sfy_dev, const double* sfz_dev, const double* vx_dev,
              const double* vy_dev, const double* vz_dev, RowPassArgs& ra)
{
    if (!a || !vx_dev || !vy_dev || !vz_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!faceless(a) && (!lambda_dev || !sfx_dev || !sfy_dev || !sfz_dev)) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    ra.a0 = lambda_dev; ra.a1 = lambda_dev; ra.sx = sfx_dev; ra.sy = sfy_dev; ra.sz = sfz_dev; ra.vx = vx_dev; ra.vy = vy_dev; ra.vz = vz_dev;
    ra.lo = a->lowerAddr.p; ra.up = a->upperAddr.p;
    return MI_OK;
}
} // namespace
extern "C" int mi_flux_div(mi_addr_t a, const double* lambda_dev, const double* sfx_dev, const double* sfy_dev, const double* sfz_dev, const double* vx_dev,
                           const double* vy_dev, const double* vz_dev, const double* cell_scale_dev_or_null, const double* add_a_dev_or_null,
                           const double* add_b_dev_or_null, double* phi_out_dev, const double* vol_dev_or_null, double* div_out_dev)
{
    RowPassArgs ra{};
    MICHK(flux_args(a, "mi_flux_div", lambda_dev, sfx_dev, sfy_dev, sfz_dev, vx_dev, vy_dev, vz_dev, ra));
    if ((!phi_out_dev && !faceless(a)) || !div_out_dev || (add_b_dev_or_null && !add_a_dev_or_null)) return fail(MI_ERR_ARG, "mi_flux_div: bad argument");
    if (faceless(a)) return row_sum<M_PLUS, M_MINUS>(a, phi_out_dev, phi_out_dev, nullptr, vol_dev_or_null, div_out_dev);   // every row sum is empty
    if (phi_out_dev == lambda_dev || phi_out_dev == sfx_dev || phi_out_dev == sfy_dev || phi_out_dev == sfz_dev || phi_out_dev == add_a_dev_or_null || phi_out_dev == add_b_dev_or_null)
        return fail(MI_ERR_ARG, "mi_flux_div: phi_out must not alias a face input (faces cut by a block boundary are recomputed from the inputs)");
    ra.sc = cell_scale_dev_or_null; ra.addA = add_a_dev_or_null; ra.addB = add_b_dev_or_null;
    // (the one-row-pass form -- every block recomputing the faces cut by its boundary, eight scattered gathers per cut face -- was built
    //  in round 5, measured slower (832 against ~560 us at 216^3, 2.26 x the algorithmic traffic: profiles/r05_assembly_pmc.md) and removed
    //  in round 6; the face pass + row sum below is the only form)
    if (a->L.nFaces > 0) {
        k_face_flux<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(ra, phi_out_dev, a->L.nFaces);
        HIPCHK(hipGetLastError());
    }
    return row_sum<M_PLUS, M_MINUS>(a, phi_out_dev, phi_out_dev, nullptr, vol_dev_or_null, div_out_dev);
}
extern "C" int mi_ddt_phi_corr(mi_addr_t a, double r_delta_t, const double* lambda_dev, const double* sfx_dev, const double* sfy_dev, const double* sfz_dev,
                               const double* ux_old_dev, const double* uy_old_dev, const double* uz_old_dev, const double* rho_old_dev_or_null,
                               const double* phi_old_dev, double* out_dev)
{
    RowPassArgs ra{};
    MICHK(flux_args(a, "mi_ddt_phi_corr", lambda_dev, sfx_dev, sfy_dev, sfz_dev, ux_old_dev, uy_old_dev, uz_old_dev, ra));
    if (a->L.nFaces == 0) return MI_OK;
    if (!phi_old_dev || !out_dev) return fail(MI_ERR_ARG, "mi_ddt_phi_corr: bad argument");
    ra.sc = rho_old_dev_or_null;
    k_ddt_phi_corr<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(ra, r_delta_t, phi_old_dev, out_dev, a->L.nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// ---- the backward time scheme (backwardDdtScheme.C, static mesh; DESIGN 3.5d) ------------------------------------------------------
extern "C" int mi_ddt_backward_coeffs(double delta_t, double delta_t0, int32_t n_old_times, double coeffs_out[3])
{
    if (!coeffs_out || !(delta_t > 0)) return fail(MI_ERR_ARG, "mi_ddt_backward_coeffs: deltaT must be positive");
    if (n_old_times >= 2 && !(delta_t0 > 0)) return fail(MI_ERR_ARG, "mi_ddt_backward_coeffs: deltaT0 must be positive");
    const double deltaT0 = n_old_times < 2 ? 1e15 : delta_t0;   // GREAT: fewer than two old times (backwardDdtScheme.C:57-69)
    const double coefft = 1 + delta_t / (delta_t + deltaT0);
    const double coefft00 = delta_t * delta_t / (deltaT0 * (delta_t + deltaT0));
    coeffs_out[0] = coefft; coeffs_out[1] = coefft + coefft00; coeffs_out[2] = coefft00;
    return MI_OK;
}
namespace {
// the arrays of a streaming call: all present and 16-byte aligned, no output among the inputs or twice
int stream_arrays(const char* who, const double* const* in, int nIn, double* const* out, int nOut)
{
    for (int i = 0; i < nIn; ++i) if (!in[i]) return fail(MI_ERR_ARG, std::string(who) + ": input arrays missing");
    for (int o = 0; o < nOut; ++o) {
        if (!out[o]) return fail(MI_ERR_ARG, std::string(who) + ": output arrays missing");
        if (!al16(out[o])) return fail(MI_ERR_ARG, std::string(who) + ": arrays must be 16-byte aligned");
        for (int i = 0; i < nIn; ++i) if (out[o] == in[i]) return fail(MI_ERR_ARG, std::string(who) + ": an output must not alias an input");
        for (int q = 0; q < o; ++q) if (out[o] == out[q]) return fail(MI_ERR_ARG, std::string(who) + ": the outputs must differ");
    }
    for (int i = 0; i < nIn; ++i) if (!al16(in[i])) return fail(MI_ERR_ARG, std::string(who) + ": arrays must be 16-byte aligned");
    return MI_OK;
}
} // namespace
extern "C" int mi_fvm_ddt_backward(mi_ctx_t c, int64_t n, double r_delta_t, const double coeffs[3], double rho_value, const double* rho_dev,
                                   const double* rho_old_dev, const double* rho_old_old_dev, const double* vol_dev, const double* psi_old_dev,
                                   const double* psi_old_old_dev, double* diag_out_dev, double* source_out_dev)
{
    const char* who = "mi_fvm_ddt_backward";
    if (!c || n < 0 || !coeffs) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const bool RHO = rho_dev || rho_old_dev || rho_old_old_dev;
    if (RHO && !(rho_dev && rho_old_dev && rho_old_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho, rho_old and rho_old_old go together");
    const double* in[6] = {vol_dev, psi_old_dev, psi_old_old_dev, rho_dev, rho_old_dev, rho_old_old_dev};
    double* out[2] = {diag_out_dev, source_out_dev};
    MICHK(stream_arrays(who, in, RHO ? 6 : 3, out, 2));
    if (n == 0) return MI_OK;
    const double cA = coeffs[0] * r_delta_t;
    if (RHO) return cell_launch(c, k_fvm_ddt_backward<true>, r_delta_t, cA, coeffs[1], coeffs[2], rho_value, rho_dev, rho_old_dev, rho_old_old_dev, vol_dev,
                                                                 psi_old_dev, psi_old_old_dev, diag_out_dev, source_out_dev, n);
    return cell_launch(c, k_fvm_ddt_backward<false>, r_delta_t, cA, coeffs[1], coeffs[2], rho_value, nullptr, nullptr, nullptr, vol_dev, psi_old_dev,
                                                             psi_old_old_dev, diag_out_dev, source_out_dev, n);
}
extern "C" int mi_fvc_ddt_backward(mi_ctx_t c, int64_t n, double r_delta_t, const double coeffs[3], double rho_value, const double* rho_dev,
                                   const double* rho_old_dev, const double* rho_old_old_dev, const double* vf_dev, const double* vf_old_dev,
                                   const double* vf_old_old_dev, double* out_dev)
{
    const char* who = "mi_fvc_ddt_backward";
    if (!c || n < 0 || !coeffs) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const bool RHO = rho_dev || rho_old_dev || rho_old_old_dev;
    if (RHO && !(rho_dev && rho_old_dev && rho_old_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho, rho_old and rho_old_old go together");
    const double* in[6] = {vf_dev, vf_old_dev, vf_old_old_dev, rho_dev, rho_old_dev, rho_old_old_dev};
    double* out[1] = {out_dev};
    MICHK(stream_arrays(who, in, RHO ? 6 : 3, out, 1));
    if (n == 0) return MI_OK;
    if (RHO) return cell_launch(c, k_fvc_ddt_backward<true>, r_delta_t, coeffs[0], coeffs[1], coeffs[2], rho_dev, rho_old_dev, rho_old_old_dev, vf_dev,
                                                                 vf_old_dev, vf_old_old_dev, out_dev, n);
    return cell_launch(c, k_fvc_ddt_backward<false>, r_delta_t * rho_value, coeffs[0], coeffs[1], coeffs[2], nullptr, nullptr, nullptr, vf_dev, vf_old_dev,
                                                             vf_old_old_dev, out_dev, n);
}
extern "C" int mi_ddt_phi_corr_backward(mi_addr_t a, double r_delta_t, const double coeffs[3], const double* lambda_dev, const double* sfx_dev,
                                        const double* sfy_dev, const double* sfz_dev, const double* ux_old_dev, const double* uy_old_dev,
                                        const double* uz_old_dev, const double* ux_old_old_dev, const double* uy_old_old_dev, const double* uz_old_old_dev,
                                        const double* rho_old_dev_or_null, const double* rho_old_old_dev_or_null, const double* phi_old_dev,
                                        const double* phi_old_old_dev, double* out_dev)
{
    const char* who = "mi_ddt_phi_corr_backward";
    RowPassArgs ra{};
    MICHK(flux_args(a, who, lambda_dev, sfx_dev, sfy_dev, sfz_dev, ux_old_dev, uy_old_dev, uz_old_dev, ra));
    if (!coeffs || !ux_old_old_dev || !uy_old_old_dev || !uz_old_old_dev || !phi_old_dev || !phi_old_old_dev || !out_dev)
        return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if ((rho_old_dev_or_null != nullptr) != (rho_old_old_dev_or_null != nullptr)) return fail(MI_ERR_ARG, std::string(who) + ": rho_old and rho_old_old go together");
    for (const double* q : {lambda_dev, sfx_dev, sfy_dev, sfz_dev, phi_old_dev, phi_old_old_dev})
        if (q == out_dev) return fail(MI_ERR_ARG, std::string(who) + ": the output must not alias a face input");
    if (a->L.nFaces == 0) return MI_OK;
    DdtCorrBackArgs k{};
    k.lo = ra.lo; k.up = ra.up; k.lam = lambda_dev; k.s[0] = sfx_dev; k.s[1] = sfy_dev; k.s[2] = sfz_dev;
    k.u0[0] = ux_old_dev; k.u0[1] = uy_old_dev; k.u0[2] = uz_old_dev; k.u00[0] = ux_old_old_dev; k.u00[1] = uy_old_old_dev; k.u00[2] = uz_old_old_dev;
    k.rho0 = rho_old_dev_or_null; k.rho00 = rho_old_old_dev_or_null; k.phi0 = phi_old_dev; k.phi00 = phi_old_old_dev; k.out = out_dev;
    k.rdt = r_delta_t; k.c0 = coeffs[1]; k.c00 = coeffs[2]; k.nf = a->L.nFaces; k.xcd = a->ctx->xcdRows;
    k_ddt_phi_corr_backward<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(k);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// ---- the CrankNicolson time scheme (CrankNicolsonDdtScheme.C, static mesh; DESIGN 3.5g) ----------------------------------------------
extern "C" int mi_ddt_cn_parse(const char* scheme, double* oc_out)
{
    const char* who = "mi_ddt_cn_parse";
    if (!scheme || !oc_out) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, std::string(who) + ": empty scheme");
    if (tok[0] != "CrankNicolson") return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[0] + "' is not CrankNicolson");
    if (tok.size() < 2) return fail(MI_ERR_ARG, std::string(who) + ": 'CrankNicolson' takes the off-centring coefficient, none given");
    if (tok.size() > 2) return fail(MI_ERR_ARG, std::string(who) + ": 'CrankNicolson' takes one coefficient: extra '" + tok[2] + "'");
    double oc = 0;
    if (!scheme_number(tok[1], oc) || oc != oc) return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[1] + "' is not a number");
    if (!(oc >= 0.0 && oc <= 1.0))                                // CrankNicolsonDdtScheme.H:165-180
        return fail(MI_ERR_ARG, std::string(who) + ": coefficient = " + tok[1] + " should be >= 0 and <= 1");
    *oc_out = oc;
    return MI_OK;
}
extern "C" int mi_ddt_cn_begin(double oc, int32_t time_index, mi_ddt_cn_state* state_out)
{
    if (!state_out) return fail(MI_ERR_ARG, "mi_ddt_cn_begin: bad argument");
    if (!(oc >= 0.0 && oc <= 1.0)) return fail(MI_ERR_ARG, "mi_ddt_cn_begin: the off-centring coefficient should be >= 0 and <= 1");
    state_out->oc = oc; state_out->start_time_index = time_index; state_out->ddt0_time_index = time_index;   // DDt0Field's constructor: both the current index
    return MI_OK;
}
extern "C" int mi_ddt_cn_step(mi_ddt_cn_state* state, int32_t time_index, double delta_t, double delta_t0, mi_ddt_cn_scalars* out)
{
    if (!state || !out) return fail(MI_ERR_ARG, "mi_ddt_cn_step: bad argument");
    if (!(delta_t > 0)) return fail(MI_ERR_ARG, "mi_ddt_cn_step: deltaT must be positive");
    const int evaluate = state->ddt0_time_index != time_index;                         // :186-194
    if (evaluate && !(delta_t0 > 0)) return fail(MI_ERR_ARG, "mi_ddt_cn_step: deltaT0 must be positive");
    const double coef = time_index - state->start_time_index > 0 ? 1.0 + state->oc : 1.0;    // coef_ :196-211
    const double coef0 = time_index - state->start_time_index > 1 ? 1.0 + state->oc : 1.0;   // coef0_ :214-229
    out->r_dt_coef = coef / delta_t;                                                   // rDtCoef_ :232-238: one division
    out->r_dt_coef0 = delta_t0 > 0 ? coef0 / delta_t0 : 0.0;                           // rDtCoef0_ :241-247 (the reference reads it only when evaluate)
    out->evaluate = evaluate;
    if (evaluate) state->ddt0_time_index = time_index;
    return MI_OK;
}
extern "C" int mi_ddt_cn_update(mi_ctx_t c, int64_t n, int32_t n_fields, double r_dt_coef0, double oc, double rho_value, const double* rho_old_dev,
                                const double* rho_old_old_dev, const double* const* psi_old_dev, const double* const* psi_old_old_dev,
                                double* const* ddt0_inout_dev)
{
    const char* who = "mi_ddt_cn_update";
    if (!c || n < 0 || n_fields < 1 || n_fields > 4 || !psi_old_dev || !psi_old_old_dev || !ddt0_inout_dev)
        return fail(MI_ERR_ARG, std::string(who) + ": bad argument (1 to 4 fields)");
    if (!(oc >= 0.0 && oc <= 1.0)) return fail(MI_ERR_ARG, std::string(who) + ": the off-centring coefficient should be >= 0 and <= 1");
    const bool RHO = rho_old_dev || rho_old_old_dev;
    if (RHO && !(rho_old_dev && rho_old_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho_old and rho_old_old go together");
    const double* in[10]; double* out[4]; int nIn = 0;
    for (int k = 0; k < n_fields; ++k) { in[nIn++] = psi_old_dev[k]; in[nIn++] = psi_old_old_dev[k]; out[k] = ddt0_inout_dev[k]; }
    if (RHO) { in[nIn++] = rho_old_dev; in[nIn++] = rho_old_old_dev; }
    MICHK(stream_arrays(who, in, nIn, out, n_fields));
    if (n == 0) return MI_OK;
    CnUpdateArgs a{};
    for (int k = 0; k < n_fields; ++k) { a.ddt0[k] = ddt0_inout_dev[k]; a.psi0[k] = psi_old_dev[k]; a.psi00[k] = psi_old_old_dev[k]; }
    a.rho0 = rho_old_dev; a.rho00 = rho_old_old_dev;
    a.c0 = RHO ? r_dt_coef0 : r_dt_coef0 * rho_value; a.oc = oc; a.offc = oc < 1.0 ? 1 : 0; a.nFields = n_fields; a.n = n;
    if (RHO) return cell_launch(c, k_ddt_cn_update<true>, a);
    return cell_launch(c, k_ddt_cn_update<false>, a);
}
extern "C" int mi_fvm_ddt_cn(mi_ctx_t c, int64_t n, double r_dt_coef, double oc, double rho_value, const double* rho_dev, const double* rho_old_dev,
                             const double* vol_dev, const double* psi_old_dev, const double* ddt0_dev, double* diag_out_dev, double* source_out_dev)
{
    const char* who = "mi_fvm_ddt_cn";
    if (!c || n < 0) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!(oc >= 0.0 && oc <= 1.0)) return fail(MI_ERR_ARG, std::string(who) + ": the off-centring coefficient should be >= 0 and <= 1");
    const bool RHO = rho_dev || rho_old_dev;
    if (RHO && !(rho_dev && rho_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho and rho_old go together");
    const double* in[5] = {vol_dev, psi_old_dev, ddt0_dev, rho_dev, rho_old_dev};
    double* out[2] = {diag_out_dev, source_out_dev};
    MICHK(stream_arrays(who, in, RHO ? 5 : 3, out, 2));
    if (n == 0) return MI_OK;
    const int offc = oc < 1.0 ? 1 : 0;
    if (RHO) return cell_launch(c, k_fvm_ddt_cn<true>, r_dt_coef, 0.0, oc, offc, rho_dev, rho_old_dev, vol_dev, psi_old_dev, ddt0_dev, diag_out_dev, source_out_dev, n);
    return cell_launch(c, k_fvm_ddt_cn<false>, r_dt_coef, r_dt_coef * rho_value, oc, offc, nullptr, nullptr, vol_dev, psi_old_dev, ddt0_dev, diag_out_dev, source_out_dev, n);
}
extern "C" int mi_fvc_ddt_cn(mi_ctx_t c, int64_t n, double r_dt_coef, double oc, double rho_value, const double* rho_dev, const double* rho_old_dev,
                             const double* vf_dev, const double* vf_old_dev, const double* ddt0_dev, double* out_dev)
{
    const char* who = "mi_fvc_ddt_cn";
    if (!c || n < 0) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!(oc >= 0.0 && oc <= 1.0)) return fail(MI_ERR_ARG, std::string(who) + ": the off-centring coefficient should be >= 0 and <= 1");
    const bool RHO = rho_dev || rho_old_dev;
    if (RHO && !(rho_dev && rho_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho and rho_old go together");
    const double* in[5] = {vf_dev, vf_old_dev, ddt0_dev, rho_dev, rho_old_dev};
    double* out[1] = {out_dev};
    MICHK(stream_arrays(who, in, RHO ? 5 : 3, out, 1));
    if (n == 0) return MI_OK;
    const int offc = oc < 1.0 ? 1 : 0;
    if (RHO) return cell_launch(c, k_fvc_ddt_cn<true>, r_dt_coef, oc, offc, rho_dev, rho_old_dev, vf_dev, vf_old_dev, ddt0_dev, out_dev, n);
    return cell_launch(c, k_fvc_ddt_cn<false>, r_dt_coef * rho_value, oc, offc, nullptr, nullptr, vf_dev, vf_old_dev, ddt0_dev, out_dev, n);
}
// ---- steadyState, localEuler and CoEuler (steadyStateDdtScheme.C, localEulerDdtScheme.C, CoEulerDdtScheme.C, static mesh; DESIGN 3.5h) ----
extern "C" int mi_ddt_local_parse(const char* scheme, mi_ddt_local_scheme* out)
{
    const char* who = "mi_ddt_local_parse";
    if (!scheme || !out) return fail(MI_ERR_ARG, std::string(who) + ": bad argument (NULL)");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, std::string(who) + ": empty scheme");
    const std::string& name = tok[0];
    if (name == "Euler" || name == "backward" || name == "CrankNicolson") return fail(MI_ERR_ARG, std::string(who) + ": '" + name + "' is not a local scheme");
    size_t words = 0;                                            // what follows the scheme's name
    const char* takes = "";
    if (name == "steadyState") { words = 0; takes = "no argument"; }
    else if (name == "localEuler") { words = 1; takes = "the name of the rDeltaT field"; }
    else if (name == "CoEuler") { words = 3; takes = "the flux's name, the density's name and maxCo"; }
    else return fail(MI_ERR_ARG, std::string(who) + ": '" + name + "' is not steadyState, localEuler or CoEuler");
    if (tok.size() - 1 < words) return fail(MI_ERR_ARG, std::string(who) + ": '" + name + "' takes " + takes + ": " + std::to_string(tok.size() - 1) + " of " + std::to_string(words) + " given after '" + tok.back() + "'");
    if (tok.size() - 1 > words) return fail(MI_ERR_ARG, std::string(who) + ": '" + name + "' takes " + takes + ": extra '" + tok[words + 1] + "'");
    mi_ddt_local_scheme s{};
    for (size_t k = 1; k < tok.size() && k <= 2; ++k)
        if (tok[k].size() >= sizeof(s.name)) return fail(MI_ERR_ARG, std::string(who) + ": the name '" + tok[k] + "' is longer than " + std::to_string(sizeof(s.name) - 1) + " characters");
    if (name == "steadyState") s.kind = MI_DDT_STEADY_STATE;
    else if (name == "localEuler") { s.kind = MI_DDT_LOCAL_EULER; std::memcpy(s.name, tok[1].c_str(), tok[1].size()); }
    else {
        s.kind = MI_DDT_CO_EULER;
        std::memcpy(s.name, tok[1].c_str(), tok[1].size()); std::memcpy(s.rho_name, tok[2].c_str(), tok[2].size());
        double m = 0;
        if (!scheme_number(tok[3], m) || m != m) return fail(MI_ERR_ARG, std::string(who) + ": maxCo '" + tok[3] + "' is not a number");
        if (!(m > 0.0) || m - m != 0.0) return fail(MI_ERR_ARG, std::string(who) + ": maxCo = " + tok[3] + " should be finite and > 0");
        s.max_co = m;
    }
    *out = s;
    return MI_OK;
}
extern "C" int mi_fvm_ddt_local(mi_ctx_t c, int64_t n, const double* r_delta_t_dev, double rho_value, const double* rho_dev, const double* rho_old_dev,
                                const double* vol_dev, const double* psi_old_dev, double* diag_out_dev, double* source_out_dev)
{
    const char* who = "mi_fvm_ddt_local";
    if (!c || n < 0) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const bool RHO = rho_dev || rho_old_dev;
    if (RHO && !(rho_dev && rho_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho and rho_old go together");
    const double* in[5] = {r_delta_t_dev, vol_dev, psi_old_dev, rho_dev, rho_old_dev};
    double* out[2] = {diag_out_dev, source_out_dev};
    MICHK(stream_arrays(who, in, RHO ? 5 : 3, out, 2));
    if (n == 0) return MI_OK;
    if (RHO) return cell_launch(c, k_fvm_ddt_local<true>, r_delta_t_dev, rho_value, rho_dev, rho_old_dev, vol_dev, psi_old_dev, diag_out_dev, source_out_dev, n);
    return cell_launch(c, k_fvm_ddt_local<false>, r_delta_t_dev, rho_value, nullptr, nullptr, vol_dev, psi_old_dev, diag_out_dev, source_out_dev, n);
}
extern "C" int mi_fvc_ddt_local(mi_ctx_t c, int64_t n, const double* r_delta_t_dev, double rho_value, const double* rho_dev, const double* rho_old_dev,
                                const double* vf_dev, const double* vf_old_dev, double* out_dev)
{
    const char* who = "mi_fvc_ddt_local";
    if (!c || n < 0) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const bool RHO = rho_dev || rho_old_dev;
    if (RHO && !(rho_dev && rho_old_dev)) return fail(MI_ERR_ARG, std::string(who) + ": rho and rho_old go together");
    const double* in[5] = {r_delta_t_dev, vf_dev, vf_old_dev, rho_dev, rho_old_dev};
    double* out[1] = {out_dev};
    MICHK(stream_arrays(who, in, RHO ? 5 : 3, out, 1));
    if (n == 0) return MI_OK;
    if (RHO) return cell_launch(c, k_fvc_ddt_local<true>, r_delta_t_dev, rho_value, rho_dev, rho_old_dev, vf_dev, vf_old_dev, out_dev, n);
    return cell_launch(c, k_fvc_ddt_local<false>, r_delta_t_dev, rho_value, nullptr, nullptr, vf_dev, vf_old_dev, out_dev, n);
}
extern "C" int mi_ddt_phi_corr_local(mi_addr_t a, const double* r_delta_t_dev, const double* lambda_dev, const double* sfx_dev, const double* sfy_dev,
                                     const double* sfz_dev, const double* ux_old_dev, const double* uy_old_dev, const double* uz_old_dev,
                                     const double* phi_old_dev, double* out_dev)
{
    const char* who = "mi_ddt_phi_corr_local";
    RowPassArgs ra{};
    MICHK(flux_args(a, who, lambda_dev, sfx_dev, sfy_dev, sfz_dev, ux_old_dev, uy_old_dev, uz_old_dev, ra));
    if (!r_delta_t_dev || !phi_old_dev || !out_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    for (const double* q : {r_delta_t_dev, lambda_dev, sfx_dev, sfy_dev, sfz_dev, ux_old_dev, uy_old_dev, uz_old_dev})
        if (q == out_dev) return fail(MI_ERR_ARG, std::string(who) + ": the output must not alias an input that other faces read");
    if (a->L.nFaces == 0) return MI_OK;
    k_ddt_phi_corr_local<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(ra, r_delta_t_dev, phi_old_dev, out_dev, a->L.nFaces);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
namespace {
int co_scalars(const char* who, double delta_t, double max_co)
{
    if (!(delta_t > 0.0) || delta_t - delta_t != 0.0) return fail(MI_ERR_ARG, std::string(who) + ": deltaT must be positive and finite");
    if (!(max_co > 0.0) || max_co - max_co != 0.0) return fail(MI_ERR_ARG, std::string(who) + ": maxCo must be positive and finite");
    return MI_OK;
}
} // namespace
extern "C" int mi_co_face_r_delta_t(mi_ctx_t c, int64_t n, const double* delta_coeffs_dev, const double* mag_sf_dev, const double* phi_dev,
                                    const double* rho_face_dev_or_null, double delta_t, double max_co, double* out_dev)
{
    const char* who = "mi_co_face_r_delta_t";
    if (!c || n < 0) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    MICHK(co_scalars(who, delta_t, max_co));
    const double* in[4] = {delta_coeffs_dev, mag_sf_dev, phi_dev, rho_face_dev_or_null};
    double* out[1] = {out_dev};
    MICHK(stream_arrays(who, in, rho_face_dev_or_null ? 4 : 3, out, 1));
    if (n == 0) return MI_OK;
    return cell_launch(c, k_co_face_r_delta_t, delta_coeffs_dev, mag_sf_dev, phi_dev, rho_face_dev_or_null, delta_t, max_co, out_dev, n);
}
extern "C" int mi_co_r_delta_t(mi_addr_t a, const double* delta_coeffs_dev, const double* mag_sf_dev, const double* phi_dev, const double* lambda_dev_or_null,
                               const double* rho_old_dev_or_null, double delta_t, double max_co, double* r_delta_t_out_dev)
{
    const char* who = "mi_co_r_delta_t";
    if (!a || !r_delta_t_out_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!faceless(a) && (!delta_coeffs_dev || !mag_sf_dev || !phi_dev)) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!faceless(a) && (lambda_dev_or_null != nullptr) != (rho_old_dev_or_null != nullptr))
        return fail(MI_ERR_ARG, std::string(who) + ": the mass-flux form takes lambda and rho_old together");
    MICHK(co_scalars(who, delta_t, max_co));
    for (const double* q : {delta_coeffs_dev, mag_sf_dev, phi_dev, lambda_dev_or_null, rho_old_dev_or_null})
        if (q && q == r_delta_t_out_dev) return fail(MI_ERR_ARG, std::string(who) + ": the output must not alias an input (cut faces are recomputed from the inputs)");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nCells == 0) return MI_OK;
    CoArgs ra{};
    ra.delta = delta_coeffs_dev; ra.magSf = mag_sf_dev; ra.phi = phi_dev; ra.lam = lambda_dev_or_null; ra.rho = rho_old_dev_or_null;
    ra.lo = a->lowerAddr.p; ra.up = a->upperAddr.p; ra.deltaT = delta_t; ra.maxCo = max_co; ra.out = r_delta_t_out_dev;
    ra.os = a->ownerStartC.p; ra.ls = a->losortStartC.p; ra.losort = a->losortC.p;
    ra.row16 = a->row16.p; ra.losort16 = a->losort16.p; ra.esc = a->rowEsc.p; ra.escStart = a->rowEscStart.p;
    const mi_addr_s::RowPlan& rp = a->rowPlan[0];
    ra.blockStart = rp.tiles ? a->tileCellStart.p : nullptr;
    ra.n = a->L.nCells; ra.cap = row_cap(rp, 1); ra.xcd = a->ctx->xcdRows;
    const size_t lds = (size_t)ra.cap * sizeof(double);
    return for_row_shape(a, rp, [&](auto s) { return row_launch(a, rp, k_co_r_delta_t<decltype(s)::bs, decltype(s)::r16>, ra, lds); });
}
extern "C" int mi_upwind_weights(mi_ctx_t c, int64_t n_faces, const double* face_flux_dev, double* weights_out_dev)
{
    if (!c || n_faces < 0 || (n_faces > 0 && (!face_flux_dev || !weights_out_dev))) return fail(MI_ERR_ARG, "mi_upwind_weights: bad argument");
    if (!al16(face_flux_dev) || !al16(weights_out_dev)) return fail(MI_ERR_ARG, "mi_upwind_weights: arrays must be 16-byte aligned");
    if (n_faces == 0) return MI_OK;
    return cell_launch(c, k_upwind_weights, face_flux_dev, weights_out_dev, n_faces);
}
extern "C" int mi_limited_linear_weights(mi_addr_t a, double k, const double* cd_weights_dev, const double* face_flux_dev,
                                         const double* phi_dev, const double* gradx_dev, const double* grady_dev, const double* gradz_dev,
                                         const double* cx_dev, const double* cy_dev, const double* cz_dev,
                                         double* weights_out_dev, double* limiter_out_dev_or_null)
{
    if (!a || !cd_weights_dev || !face_flux_dev || !phi_dev || !gradx_dev || !grady_dev || !gradz_dev || !cx_dev || !cy_dev || !cz_dev || !weights_out_dev)
        return fail(MI_ERR_ARG, "mi_limited_linear_weights: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    const double twoByk = 2.0 / (k > 1e-15 ? k : 1e-15);
    k_limited_linear_weights<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(a->lowerAddr.p, a->upperAddr.p, twoByk, cd_weights_dev, face_flux_dev,
        phi_dev, gradx_dev, grady_dev, gradz_dev, cx_dev, cy_dev, cz_dev, weights_out_dev, limiter_out_dev_or_null, a->L.nFaces, a->ctx->xcdRows);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// ---- the limited schemes: parse (host only) and the two face passes -------------------------------------------------------------
namespace {
struct LimName { const char* name; int kind, vec, bounded, hasK; double lower, upper; };   // bounded 1: "lo hi" read; 2: Limited01 (0, 1)
// the names the reference registers (finiteVolume/Make/files:253-273 and the make* macros of limitedSchemes/*/*.C)
const LimName kLimNames[] = {
    {"limitedLinear", MI_LIM_LIMITED_LINEAR, 0, 0, 1, 0, 0}, {"limitedLinearV", MI_LIM_LIMITED_LINEAR, 1, 0, 1, 0, 0},
    {"limitedLimitedLinear", MI_LIM_LIMITED_LINEAR, 0, 1, 1, 0, 0}, {"limitedLinear01", MI_LIM_LIMITED_LINEAR, 0, 2, 1, 0, 1},
    {"vanLeer", MI_LIM_VAN_LEER, 0, 0, 0, 0, 0}, {"vanLeerV", MI_LIM_VAN_LEER, 1, 0, 0, 0, 0},
    {"limitedVanLeer", MI_LIM_VAN_LEER, 0, 1, 0, 0, 0}, {"vanLeer01", MI_LIM_VAN_LEER, 0, 2, 0, 0, 1},
    {"MUSCL", MI_LIM_MUSCL, 0, 0, 0, 0, 0}, {"MUSCLV", MI_LIM_MUSCL, 1, 0, 0, 0, 0},
    {"limitedMUSCL", MI_LIM_MUSCL, 0, 1, 0, 0, 0}, {"MUSCL01", MI_LIM_MUSCL, 0, 2, 0, 0, 1},
    {"Minmod", MI_LIM_MINMOD, 0, 0, 0, 0, 0}, {"MinmodV", MI_LIM_MINMOD, 1, 0, 0, 0, 0},
    {"SuperBee", MI_LIM_SUPERBEE, 0, 0, 0, 0, 0}, {"SuperBeeV", MI_LIM_SUPERBEE, 1, 0, 0, 0, 0},
    {"UMIST", MI_LIM_UMIST, 0, 0, 0, 0, 0}, {"UMISTV", MI_LIM_UMIST, 1, 0, 0, 0, 0},
    {"vanAlbada", MI_LIM_VAN_ALBADA, 0, 0, 0, 0, 0}, {"vanAlbadaV", MI_LIM_VAN_ALBADA, 1, 0, 0, 0, 0},
    {"OSPRE", MI_LIM_OSPRE, 0, 0, 0, 0, 0}, {"OSPREV", MI_LIM_OSPRE, 1, 0, 0, 0, 0},
    {"QUICK", MI_LIM_QUICK, 0, 0, 0, 0, 0}, {"QUICKV", MI_LIM_QUICK, 1, 0, 0, 0, 0},
    {"limitedCubic", MI_LIM_LIMITED_CUBIC, 0, 0, 1, 0, 0}, {"limitedCubicV", MI_LIM_LIMITED_CUBIC, 1, 0, 1, 0, 0},
    {"limitedLimitedCubic", MI_LIM_LIMITED_CUBIC, 0, 1, 1, 0, 0}, {"limitedCubic01", MI_LIM_LIMITED_CUBIC, 0, 2, 1, 0, 1},
    {"Gamma", MI_LIM_GAMMA, 0, 0, 1, 0, 0}, {"GammaV", MI_LIM_GAMMA, 1, 0, 1, 0, 0},
    {"limitedGamma", MI_LIM_GAMMA, 0, 1, 1, 0, 0}, {"Gamma01", MI_LIM_GAMMA, 0, 2, 1, 0, 1},
    {"SFCD", MI_LIM_SFCD, 0, 0, 0, 0, 0}, {"SFCDV", MI_LIM_SFCD, 1, 0, 0, 0, 0},
};
bool lim_has_k(int kind) { return kind == MI_LIM_LIMITED_LINEAR || kind == MI_LIM_LIMITED_CUBIC || kind == MI_LIM_GAMMA; }
// the constructors' checks (limitedLinear.H:67-73, limitedCubic.H:67-73, Gamma.H:66-72, Limited.H:54-64) on a caller-filled mi_limiter
int lim_check(const char* who, const mi_limiter* l, LimCoef& c)
{
    if (!l || l->kind < 0 || l->kind >= LIM_N || (l->vector_form != 0 && l->vector_form != 1) || (l->bounded != 0 && l->bounded != 1))
        return fail(MI_ERR_ARG, std::string(who) + ": invalid mi_limiter");
    if (lim_has_k(l->kind) && !(l->k >= 0 && l->k <= 1)) return fail(MI_ERR_ARG, std::string(who) + ": coefficient k should be >= 0 and <= 1");
    if (l->bounded && l->vector_form) return fail(MI_ERR_ARG, std::string(who) + ": the bounded (Limited) form exists for scalar fields only");
    if (l->bounded && !(l->lower <= l->upper)) return fail(MI_ERR_ARG, std::string(who) + ": lower bound is higher than the upper bound");
    c = LimCoef{};
    c.twoByk = 2.0 / (l->k > 1e-15 ? l->k : 1e-15);                          // 2.0/max(k, SMALL)
    c.gammaK = l->k / 2.0 > 1e-15 ? l->k / 2.0 : 1e-15;                      // Gamma.H:76 max(k/2, SMALL)
    c.lower = l->lower; c.upper = l->upper; c.bounded = l->bounded;
    return MI_OK;
}
#define MI_LIM_CASES(KERNEL, ARGS)                                                                                                       \
    template <int KIND, bool VEC> void launch_##KERNEL(dim3 g, dim3 b, hipStream_t s, const ARGS& a) { KERNEL<KIND, VEC><<<g, b, 0, s>>>(a); } \
    void dispatch_##KERNEL(int kind, bool vec, dim3 g, dim3 b, hipStream_t s, const ARGS& a)                                             \
    {                                                                                                                                    \
        typedef void (*F)(dim3, dim3, hipStream_t, const ARGS&);                                                                         \
        static const F tab[2][LIM_ALL] = {                                                                                               \
            {launch_##KERNEL<0, false>, launch_##KERNEL<1, false>, launch_##KERNEL<2, false>, launch_##KERNEL<3, false>,                 \
             launch_##KERNEL<4, false>, launch_##KERNEL<5, false>, launch_##KERNEL<6, false>, launch_##KERNEL<7, false>,                 \
             launch_##KERNEL<8, false>, launch_##KERNEL<9, false>, launch_##KERNEL<10, false>, launch_##KERNEL<11, false>,               \
             launch_##KERNEL<LIM_FLT_LINEAR, false>, launch_##KERNEL<LIM_FLT_LINEAR2, false>, launch_##KERNEL<LIM_FLT_LINEAR3, false>},  \
            {launch_##KERNEL<0, true>, launch_##KERNEL<1, true>, launch_##KERNEL<2, true>, launch_##KERNEL<3, true>,                     \
             launch_##KERNEL<4, true>, launch_##KERNEL<5, true>, launch_##KERNEL<6, true>, launch_##KERNEL<7, true>,                     \
             launch_##KERNEL<8, true>, launch_##KERNEL<9, true>, launch_##KERNEL<10, true>, launch_##KERNEL<11, true>,                   \
             nullptr /* filteredLinear has no V form: flt_check refuses it */, launch_##KERNEL<LIM_FLT_LINEAR2, true>,                   \
             launch_##KERNEL<LIM_FLT_LINEAR3, true>}};                                                                                   \
        tab[vec ? 1 : 0][kind](g, b, s, a);                                                                                              \
    }
MI_LIM_CASES(k_limited_weights, LimArgs)
MI_LIM_CASES(k_patch_limited_weights, PatchLimArgs)
#undef MI_LIM_CASES
// every output must differ from every input (other faces read the inputs while the pass writes) and from the other output
int lim_outputs(const char* who, const double* const* in, int m, double* w, double* limOut)
{
    for (int j = 0; j < m; ++j) if (!in[j]) return fail(MI_ERR_ARG, std::string(who) + ": input arrays missing");
    if (!w) return fail(MI_ERR_ARG, std::string(who) + ": the weights output is missing");
    if (w == limOut) return fail(MI_ERR_ARG, std::string(who) + ": weights_out and limiter_out must differ");
    for (int j = 0; j < m; ++j)
        if (in[j] == w || (limOut && in[j] == limOut)) return fail(MI_ERR_ARG, std::string(who) + ": an output must not alias an input");
    return MI_OK;
}
} // namespace

extern "C" int mi_limiter_parse(const char* scheme, mi_limiter* out)
{
    if (!scheme || !out) return fail(MI_ERR_ARG, "mi_limiter_parse: bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, "mi_limiter_parse: empty scheme");
    const std::string& name = tok[0];
    const LimName* e = nullptr;
    for (const LimName& x : kLimNames) if (name == x.name) e = &x;
    if (!e) return fail(MI_ERR_ARG, "mi_limiter_parse: unknown limited scheme '" + name + "'");
    const int want = (e->hasK ? 1 : 0) + (e->bounded == 1 ? 2 : 0);   // LimitedLimiter: the limiter's own coefficient first, then lower, upper
    const int got = (int)tok.size() - 1;
    if (got > want) return fail(MI_ERR_ARG, "mi_limiter_parse: '" + name + "' takes " + std::to_string(want) + " coefficient(s): extra '" + tok[want + 1] + "'");
    double v[3] = {0, 0, 0};
    for (int j = 0; j < got; ++j)
        if (!scheme_number(tok[j + 1], v[j])) return fail(MI_ERR_ARG, "mi_limiter_parse: '" + tok[j + 1] + "' is not a number");
    if (got < want) return fail(MI_ERR_ARG, "mi_limiter_parse: '" + name + "' takes " + std::to_string(want) + " coefficient(s), " + std::to_string(got) + " given");
    mi_limiter l{};
    l.kind = e->kind; l.vector_form = e->vec; l.bounded = e->bounded ? 1 : 0;
    l.k = e->hasK ? v[0] : 0.0;
    l.lower = e->bounded == 2 ? 0.0 : e->bounded == 1 ? v[e->hasK ? 1 : 0] : 0.0;
    l.upper = e->bounded == 2 ? 1.0 : e->bounded == 1 ? v[e->hasK ? 2 : 1] : 0.0;
    LimCoef c;
    MICHK(lim_check("mi_limiter_parse", &l, c));
    *out = l;
    return MI_OK;
}

namespace {
// the internal-face pass of a checked limiter (coefficients k, kernel kind, V form): mi_limited_weights and mi_filtered_weights
int lim_internal(const char* who, mi_addr_s* a, const LimCoef& k, int kind, bool vec, const double* cd_weights_dev, const double* face_flux_dev,
                 const double* const* phi_dev, const double* const* grad_dev, const double* const* c_dev, double* weights_out_dev,
                 double* limiter_out_dev_or_null)
{
    LimArgs q{};
    q.k = k;
    const int m = vec ? 3 : 1;
    const double* in[17];
    int n = 0;
    in[n++] = q.cdw = cd_weights_dev; in[n++] = q.flux = face_flux_dev;
    for (int j = 0; j < m; ++j) in[n++] = q.phi[j] = phi_dev[j];
    for (int j = 0; j < 3 * m; ++j) in[n++] = q.grad[j] = grad_dev[j];
    for (int d = 0; d < 3; ++d) in[n++] = q.cc[d] = c_dev[d];
    MICHK(lim_outputs(who, in, n, weights_out_dev, limiter_out_dev_or_null));
    if (!al16(cd_weights_dev) || !al16(face_flux_dev) || !al16(weights_out_dev) || (limiter_out_dev_or_null && !al16(limiter_out_dev_or_null)))
        return fail(MI_ERR_ARG, std::string(who) + ": face fields must be 16-byte aligned");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.w = weights_out_dev; q.limOut = limiter_out_dev_or_null;
    q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    dispatch_k_limited_weights(kind, vec, dim3(grid_for(a->ctx, a->L.nFaces)), dim3(256), a->ctx->stream, q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// the same on one coupled patch: mi_patch_limited_weights and mi_patch_filtered_weights
int lim_patch(const char* who, mi_patch_s* p, const LimCoef& k, int kind, bool vec, const double* patch_cd_weights_dev, const double* patch_flux_dev,
              const double* const* phi_dev, const double* const* nbr_phi_dev, const double* const* grad_dev, const double* const* nbr_grad_dev,
              const double* const* patch_delta_dev, double* weights_out_dev, double* limiter_out_dev_or_null)
{
    if (p->nFaces == 0) return MI_OK;
    if (!phi_dev || !nbr_phi_dev || !grad_dev || !nbr_grad_dev || !patch_delta_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    PatchLimArgs q{};
    q.k = k;
    const int m = vec ? 3 : 1;
    const double* in[29];
    int n = 0;
    in[n++] = q.cdw = patch_cd_weights_dev; in[n++] = q.flux = patch_flux_dev;
    for (int j = 0; j < m; ++j) { in[n++] = q.phi[j] = phi_dev[j]; in[n++] = q.nphi[j] = nbr_phi_dev[j]; }
    for (int j = 0; j < 3 * m; ++j) { in[n++] = q.grad[j] = grad_dev[j]; in[n++] = q.ngrad[j] = nbr_grad_dev[j]; }
    for (int d = 0; d < 3; ++d) in[n++] = q.pd[d] = patch_delta_dev[d];
    MICHK(lim_outputs(who, in, n, weights_out_dev, limiter_out_dev_or_null));
    HIPCHK(hipSetDevice(p->ctx->device));
    q.fc = p->faceCells.p; q.w = weights_out_dev; q.limOut = limiter_out_dev_or_null; q.n = p->nFaces;
    dispatch_k_patch_limited_weights(kind, vec, dim3((p->nFaces + 255) / 256), dim3(256), p->ctx->stream, q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace

extern "C" int mi_limited_weights(mi_addr_t a, const mi_limiter* lim, const double* cd_weights_dev, const double* face_flux_dev,
                                  const double* const* phi_dev, const double* const* grad_dev, const double* const* c_dev,
                                  double* weights_out_dev, double* limiter_out_dev_or_null)
{
    const char* who = "mi_limited_weights";
    if (!a || !phi_dev || !grad_dev || !c_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    LimCoef k;
    MICHK(lim_check(who, lim, k));
    return lim_internal(who, a, k, lim->kind, lim->vector_form != 0, cd_weights_dev, face_flux_dev, phi_dev, grad_dev, c_dev, weights_out_dev,
                        limiter_out_dev_or_null);
}

extern "C" int mi_patch_limited_weights(mi_patch_t p, const mi_limiter* lim, const double* patch_cd_weights_dev, const double* patch_flux_dev,
                                        const double* const* phi_dev, const double* const* nbr_phi_dev, const double* const* grad_dev,
                                        const double* const* nbr_grad_dev, const double* const* patch_delta_dev,
                                        double* weights_out_dev, double* limiter_out_dev_or_null)
{
    const char* who = "mi_patch_limited_weights";
    if (!p) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    LimCoef k;
    MICHK(lim_check(who, lim, k));
    return lim_patch(who, p, k, lim->kind, lim->vector_form != 0, patch_cd_weights_dev, patch_flux_dev, phi_dev, nbr_phi_dev, grad_dev, nbr_grad_dev,
                     patch_delta_dev, weights_out_dev, limiter_out_dev_or_null);
}

// ---- the filtered centred limiters: parse (host only) and the two face passes on the limited schemes' kernels (DESIGN 3.5j) -----------
namespace {
struct FltName { const char* name; int kind, vec, nCoef; };
// the names the reference registers (limitedSchemes/filteredLinear/filteredLinear.C:33-37, filteredLinear2/filteredLinear2.C:34-44,
// filteredLinear3/filteredLinear3.C:34-44)
const FltName kFltNames[] = {
    {"filteredLinear", MI_FLT_LINEAR, 0, 0}, {"filteredLinear2", MI_FLT_LINEAR2, 0, 2}, {"filteredLinear2V", MI_FLT_LINEAR2, 1, 2},
    {"filteredLinear3", MI_FLT_LINEAR3, 0, 1}, {"filteredLinear3V", MI_FLT_LINEAR3, 1, 1},
};
// the constructors' checks (filteredLinear2.H:85-99, filteredLinear2V.H:85-99, filteredLinear3.H:75-81, filteredLinear3V.H:75-81) on a
// caller-filled mi_filtered_limiter; a coefficient its kind does not read is not looked at
int flt_check(const char* who, const mi_filtered_limiter* l, LimCoef& c)
{
    if (!l || l->kind < MI_FLT_LINEAR || l->kind > MI_FLT_LINEAR3 || (l->vector_form != 0 && l->vector_form != 1) ||
        (l->kind == MI_FLT_LINEAR && l->vector_form))
        return fail(MI_ERR_ARG, std::string(who) + ": invalid mi_filtered_limiter");
    if (l->kind != MI_FLT_LINEAR && !(l->k >= 0 && l->k <= 1)) return fail(MI_ERR_ARG, std::string(who) + ": coefficient k should be >= 0 and <= 1");
    if (l->kind == MI_FLT_LINEAR2 && !(l->l >= 0 && l->l <= 1)) return fail(MI_ERR_ARG, std::string(who) + ": coefficient l should be >= 0 and <= 1");
    c = LimCoef{};
    c.fltK = l->k;
    c.fltL = l->l + 1.0;                                         // filteredLinear2.H:101: l_ += 1.0
    return MI_OK;
}
} // namespace

extern "C" int mi_filtered_parse(const char* scheme, mi_filtered_limiter* out)
{
    const std::string who = "mi_filtered_parse";
    if (!scheme || !out) return fail(MI_ERR_ARG, who + ": bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, who + ": empty scheme");
    const std::string& name = tok[0];
    const FltName* e = nullptr;
    for (const FltName& x : kFltNames) if (name == x.name) e = &x;
    if (!e) return fail(MI_ERR_ARG, who + ": unknown filtered scheme '" + name + "' (filteredLinear | filteredLinear2 k l | filteredLinear2V k l | "
                                          "filteredLinear3 k | filteredLinear3V k)");
    const int want = e->nCoef, got = (int)tok.size() - 1;
    if (got > want) return fail(MI_ERR_ARG, who + ": '" + name + "' takes " + std::to_string(want) + " coefficient(s): extra '" + tok[want + 1] + "'");
    double v[2] = {0, 0};
    for (int j = 0; j < got; ++j)
        if (!scheme_number(tok[j + 1], v[j])) return fail(MI_ERR_ARG, who + ": '" + tok[j + 1] + "' is not a number");
    if (got < want) return fail(MI_ERR_ARG, who + ": '" + name + "' takes " + std::to_string(want) + " coefficient(s), " + std::to_string(got) + " given");
    mi_filtered_limiter l{};
    l.kind = e->kind; l.vector_form = e->vec; l.k = v[0]; l.l = v[1];
    LimCoef c;
    MICHK(flt_check(who.c_str(), &l, c));
    *out = l;
    return MI_OK;
}

extern "C" int mi_filtered_weights(mi_addr_t a, const mi_filtered_limiter* lim, const double* cd_weights_dev, const double* face_flux_dev,
                                   const double* const* phi_dev, const double* const* grad_dev, const double* const* c_dev,
                                   double* weights_out_dev, double* limiter_out_dev_or_null)
{
    const char* who = "mi_filtered_weights";
    if (!a || !phi_dev || !grad_dev || !c_dev) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    LimCoef k;
    MICHK(flt_check(who, lim, k));
    return lim_internal(who, a, k, LIM_FLT_LINEAR + lim->kind, lim->vector_form != 0, cd_weights_dev, face_flux_dev, phi_dev, grad_dev, c_dev,
                        weights_out_dev, limiter_out_dev_or_null);
}

extern "C" int mi_patch_filtered_weights(mi_patch_t p, const mi_filtered_limiter* lim, const double* patch_cd_weights_dev, const double* patch_flux_dev,
                                         const double* const* phi_dev, const double* const* nbr_phi_dev, const double* const* grad_dev,
                                         const double* const* nbr_grad_dev, const double* const* patch_delta_dev,
                                         double* weights_out_dev, double* limiter_out_dev_or_null)
{
    const char* who = "mi_patch_filtered_weights";
    if (!p) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    LimCoef k;
    MICHK(flt_check(who, lim, k));
    return lim_patch(who, p, k, LIM_FLT_LINEAR + lim->kind, lim->vector_form != 0, patch_cd_weights_dev, patch_flux_dev, phi_dev, nbr_phi_dev, grad_dev,
                     nbr_grad_dev, patch_delta_dev, weights_out_dev, limiter_out_dev_or_null);
}

// ---- the cubic correction: the internal faces and one coupled patch (DESIGN 3.5j) ----------------------------------------------------
namespace {
// geometry, fields and outputs of either cubic pass: every array present, the streamed face fields aligned, no output among the inputs or twice
int cubic_arrays(const std::string& who, const mi_cubic_geometry* geo, int nRhs, const double* flux, const double* const* const* cellIn, int nCellIn,
                 double* const* out, bool aligned, CubicGeo& g)
{
    if (!geo) return fail(MI_ERR_ARG, who + ": the geometry is missing");
    g.lam = geo->lambda_dev; g.magSf = geo->mag_sf_dev; g.dc = geo->delta_coeffs_dev;
    for (int d = 0; d < 3; ++d) g.sf[d] = geo->sf_dev[d];
    const double* in[7 + 32] = {g.lam, g.sf[0], g.sf[1], g.sf[2], g.magSf, g.dc};
    int m = 6;
    for (int j = 0; j < m; ++j) if (!in[j]) return fail(MI_ERR_ARG, who + ": geometry arrays missing (lambda, Sf x3, magSf, deltaCoeffs)");
    if (aligned) for (int j = 0; j < m; ++j) if (!al16(in[j])) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned");
    if (flux) { if (aligned && !al16(flux)) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned"); in[m++] = flux; }
    for (int t = 0; t < nCellIn; ++t) {
        const int cnt = (t % 2 == 0 ? 1 : 3) * nRhs;              // tables alternate: a field (n_rhs arrays), its gradient (3*n_rhs)
        for (int j = 0; j < cnt; ++j) {
            if (!cellIn[t][j]) return fail(MI_ERR_ARG, who + ": input arrays missing (one field and 3 gradient components per right-hand side)");
            in[m++] = cellIn[t][j];
        }
    }
    for (int r = 0; r < nRhs; ++r) {
        if (!out[r]) return fail(MI_ERR_ARG, who + ": null output");
        if (aligned && !al16(out[r])) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned");
        for (int j = 0; j < m; ++j) if (out[r] == in[j]) return fail(MI_ERR_ARG, who + ": an output must not alias an input");
        for (int s = 0; s < r; ++s) if (out[s] == out[r]) return fail(MI_ERR_ARG, who + ": the outputs must differ");
    }
    return MI_OK;
}
} // namespace

extern "C" int mi_cubic_correction(mi_addr_t a, const mi_cubic_geometry* geo, int32_t n_rhs, const double* const* vf_dev, const double* const* grad_dev,
                                   const double* face_flux_dev_or_null, double* const* out_dev)
{
    const std::string who = "mi_cubic_correction";
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n_rhs < 1 || n_rhs > 4) return fail(MI_ERR_ARG, who + ": a correction needs 1 to 4 components");
    if (faceless(a)) return MI_OK;                        // no face to correct: the outputs are empty
    if (!vf_dev || !grad_dev || !out_dev) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    CubicArgs q{};
    const double* const* tables[2] = {vf_dev, grad_dev};
    MICHK(cubic_arrays(who, geo, n_rhs, face_flux_dev_or_null, tables, 2, out_dev, true, q.g));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.flux = face_flux_dev_or_null;
    for (int r = 0; r < n_rhs; ++r) { q.vf[r] = vf_dev[r]; q.out[r] = out_dev[r]; }
    for (int j = 0; j < 3 * n_rhs; ++j) q.grad[j] = grad_dev[j];
    q.nRhs = n_rhs; q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    k_cubic_corr<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_patch_cubic_correction(mi_patch_t p, const mi_cubic_geometry* patch_geo, int32_t n_rhs, const double* const* vf_dev,
                                         const double* const* nbr_vf_dev, const double* const* grad_dev, const double* const* nbr_grad_dev,
                                         const double* patch_flux_dev_or_null, double* const* out_dev)
{
    const std::string who = "mi_patch_cubic_correction";
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n_rhs < 1 || n_rhs > 4) return fail(MI_ERR_ARG, who + ": a correction needs 1 to 4 components");
    if (p->nFaces == 0) return MI_OK;
    if (!vf_dev || !nbr_vf_dev || !grad_dev || !nbr_grad_dev || !out_dev) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    PatchCubicArgs q{};
    const double* const* tables[4] = {vf_dev, grad_dev, nbr_vf_dev, nbr_grad_dev};
    MICHK(cubic_arrays(who, patch_geo, n_rhs, patch_flux_dev_or_null, tables, 4, out_dev, false, q.g));
    HIPCHK(hipSetDevice(p->ctx->device));
    q.fc = p->faceCells.p; q.flux = patch_flux_dev_or_null;
    for (int r = 0; r < n_rhs; ++r) { q.vf[r] = vf_dev[r]; q.nvf[r] = nbr_vf_dev[r]; q.out[r] = out_dev[r]; }
    for (int j = 0; j < 3 * n_rhs; ++j) { q.grad[j] = grad_dev[j]; q.ngrad[j] = nbr_grad_dev[j]; }
    q.nRhs = n_rhs; q.n = p->nFaces;
    k_patch_cubic_corr<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_gauss_grad(mi_addr_t a, const double* sfx_dev, const double* sfy_dev, const double* sfz_dev, const double* ssf_dev,
                             const double* vol_dev_or_null, double* gx_dev, double* gy_dev, double* gz_dev)
{
    if (!a || !gx_dev || !gy_dev || !gz_dev) return fail(MI_ERR_ARG, "mi_gauss_grad: bad argument");
    if (!faceless(a) && (!sfx_dev || !sfy_dev || !sfz_dev || !ssf_dev)) return fail(MI_ERR_ARG, "mi_gauss_grad: bad argument");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nCells == 0) return MI_OK;
    GradArgs ga{};
    const mi_addr_s::RowPlan& rp = a->rowPlan[1];
    ga.os = a->ownerStartC.p; ga.ls = a->losortStartC.p; ga.losort = a->losortC.p; ga.blockStart = rp.tiles ? a->tileCellStart.p : nullptr;
    ga.Sfx = sfx_dev; ga.Sfy = sfy_dev; ga.Sfz = sfz_dev; ga.ssf = ssf_dev; ga.vol = vol_dev_or_null;
    ga.gx = gx_dev; ga.gy = gy_dev; ga.gz = gz_dev;
    ga.n = a->L.nCells; ga.cap = row_cap(rp, 4); ga.xcd = a->ctx->xcdRows;
    const size_t lds = (size_t)4 * ga.cap * sizeof(double);
    if (rp.bs == 256) return row_launch(a, rp, k_gauss_grad<256>, ga, lds);
    if (rp.bs == 512) return row_launch(a, rp, k_gauss_grad<512>, ga, lds);
    return row_launch(a, rp, k_gauss_grad<1024>, ga, lds);
}
// ---- fvc::div(visc*dev[2](T(grad(U)))): internal faces, the boundary gradient, the patch flux (DESIGN 3.5f) ---------------------------
namespace {
// the arrays of one of the three entries: every one present and aligned for a double, no output among the inputs or twice
int dev_tgrad_arrays(const std::string& who, const double* const* in, int nIn, double* const* out, int nOut)
{
    for (int i = 0; i < nIn; ++i) {
        if (!in[i]) return fail(MI_ERR_ARG, who + ": an input array is missing");
        if (!al8(in[i])) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
    }
    for (int o = 0; o < nOut; ++o) {
        if (!out[o]) return fail(MI_ERR_ARG, who + ": an output array is missing");
        if (!al8(out[o])) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
        for (int i = 0; i < nIn; ++i) if (out[o] == in[i]) return fail(MI_ERR_ARG, who + ": an output must not alias an input");
        for (int q = 0; q < o; ++q) if (out[o] == out[q]) return fail(MI_ERR_ARG, who + ": the outputs must differ");
    }
    return MI_OK;
}
int dev_kind(const std::string& who, int32_t kind)
{
    if (kind != MI_DEV && kind != MI_DEV2) return fail(MI_ERR_ARG, who + ": kind must be MI_DEV or MI_DEV2");
    return MI_OK;
}
} // namespace
extern "C" int mi_fvc_div_dev_tgrad(mi_addr_t a, int32_t kind, const double* lambda_dev, const double* sfx_dev, const double* sfy_dev,
                                    const double* sfz_dev, const double* visc_dev, const double* const* grad_dev, const double* vol_dev_or_null,
                                    double* const* face_out_dev, double* const* div_out_dev)
{
    const std::string who = "mi_fvc_div_dev_tgrad";
    MICHK(dev_kind(who, kind));
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    if (!grad_dev || !face_out_dev || !div_out_dev) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    if (a->L.nCells == 0) return MI_OK;
    const double* in[16] = {visc_dev};
    int nIn = 1;
    for (int i = 0; i < 9; ++i) in[nIn++] = grad_dev[i];
    if (vol_dev_or_null) in[nIn++] = vol_dev_or_null;
    if (a->L.nFaces == 0) {                                      // no face (their arrays are empty), no launch: the sums are empty
        MICHK(dev_tgrad_arrays(who, in, nIn, div_out_dev, 3));
        HIPCHK(hipSetDevice(a->ctx->device));
        for (int j = 0; j < 3; ++j) HIPCHK(hipMemsetAsync(div_out_dev[j], 0, (size_t)a->L.nCells * sizeof(double), a->ctx->stream));
        return MI_OK;
    }
    for (const double* q : {lambda_dev, sfx_dev, sfy_dev, sfz_dev}) in[nIn++] = q;
    double* out[6];
    for (int j = 0; j < 3; ++j) { out[j] = face_out_dev[j]; out[3 + j] = div_out_dev[j]; }
    MICHK(dev_tgrad_arrays(who, in, nIn, out, 6));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    DevTGradArgs fa{};
    fa.lo = a->lowerAddr.p; fa.up = a->upperAddr.p; fa.lam = lambda_dev; fa.s[0] = sfx_dev; fa.s[1] = sfy_dev; fa.s[2] = sfz_dev; fa.visc = visc_dev;
    for (int i = 0; i < 9; ++i) fa.g[i] = grad_dev[i];
    for (int j = 0; j < 3; ++j) fa.out[j] = face_out_dev[j];
    fa.nf = a->L.nFaces; fa.xcd = a->ctx->xcdRows;
    if (kind == MI_DEV) k_face_dev_tgrad_flux<MI_DEV><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(fa);
    else k_face_dev_tgrad_flux<MI_DEV2><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(fa);
    HIPCHK(hipGetLastError());
    RowSum3Args ra{};
    const mi_addr_s::RowPlan& rp = a->rowPlan[1];                // the gradient's plan: three staged arrays against its four
    ra.os = a->ownerStartC.p; ra.ls = a->losortStartC.p; ra.losort = a->losortC.p; ra.blockStart = rp.tiles ? a->tileCellStart.p : nullptr;
    for (int j = 0; j < 3; ++j) { ra.f[j] = face_out_dev[j]; ra.out[j] = div_out_dev[j]; }
    ra.vol = vol_dev_or_null;
    ra.n = a->L.nCells; ra.cap = row_cap(rp, 3); ra.xcd = a->ctx->xcdRows;
    const size_t lds = (size_t)3 * ra.cap * sizeof(double);
    if (rp.bs == 256) return row_launch(a, rp, k_row_sum3<256>, ra, lds);
    if (rp.bs == 512) return row_launch(a, rp, k_row_sum3<512>, ra, lds);
    return row_launch(a, rp, k_row_sum3<1024>, ra, lds);
}
namespace {
template <int NCOMP>
int patch_gauss_grad_correct(const std::string& who, mi_patch_s* p, const double* sfx, const double* sfy, const double* sfz, const double* magSf,
                             const double* const* sn, const double* const* g, double* const* out)
{
    PatchGradCorrArgs<NCOMP> q{};
    const double* in[4 + 4 * NCOMP] = {sfx, sfy, sfz, magSf};
    int nIn = 4;
    for (int j = 0; j < NCOMP; ++j) in[nIn++] = q.sn[j] = sn[j];
    for (int i = 0; i < 3 * NCOMP; ++i) { in[nIn++] = q.g[i] = g[i]; q.out[i] = out[i]; }
    MICHK(dev_tgrad_arrays(who, in, nIn, out, 3 * NCOMP));
    q.fc = p->faceCells.p; q.s[0] = sfx; q.s[1] = sfy; q.s[2] = sfz; q.magSf = magSf; q.n = p->nFaces;
    HIPCHK(hipSetDevice(p->ctx->device));
    k_patch_gauss_grad_correct<NCOMP><<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace
extern "C" int mi_patch_gauss_grad_correct(mi_patch_t p, int32_t n_comp, const double* patch_sfx_dev, const double* patch_sfy_dev,
                                           const double* patch_sfz_dev, const double* patch_magsf_dev, const double* const* patch_sngrad_dev,
                                           const double* const* grad_dev, double* const* patch_grad_out_dev)
{
    const std::string who = "mi_patch_gauss_grad_correct";
    if (n_comp != 1 && n_comp != 3) return fail(MI_ERR_ARG, who + ": n_comp must be 1 or 3");
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    if (!patch_sngrad_dev || !grad_dev || !patch_grad_out_dev) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    if (p->nFaces == 0) return MI_OK;
    if (n_comp == 1) return patch_gauss_grad_correct<1>(who, p, patch_sfx_dev, patch_sfy_dev, patch_sfz_dev, patch_magsf_dev, patch_sngrad_dev, grad_dev, patch_grad_out_dev);
    return patch_gauss_grad_correct<3>(who, p, patch_sfx_dev, patch_sfy_dev, patch_sfz_dev, patch_magsf_dev, patch_sngrad_dev, grad_dev, patch_grad_out_dev);
}
extern "C" int mi_patch_dev_tgrad_flux(mi_patch_t p, int32_t kind, const double* patch_sfx_dev, const double* patch_sfy_dev, const double* patch_sfz_dev,
                                       const double* patch_weights_dev_or_null, const double* visc_dev, const double* const* grad_dev,
                                       const double* nbr_visc_dev, const double* const* nbr_grad_dev, double* const* flux_out_dev)
{
    const std::string who = "mi_patch_dev_tgrad_flux";
    MICHK(dev_kind(who, kind));
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    const bool coupled = patch_weights_dev_or_null != nullptr;
    if (!grad_dev || !flux_out_dev || (coupled && !nbr_grad_dev)) return fail(MI_ERR_ARG, who + ": a pointer table is missing");
    if (p->nFaces == 0) return MI_OK;
    PatchDevTGradArgs q{};
    const double* in[24] = {patch_sfx_dev, patch_sfy_dev, patch_sfz_dev, visc_dev};
    int nIn = 4;
    for (int i = 0; i < 9; ++i) in[nIn++] = q.g[i] = grad_dev[i];
    if (coupled) {
        in[nIn++] = q.w = patch_weights_dev_or_null; in[nIn++] = q.nvisc = nbr_visc_dev;
        for (int i = 0; i < 9; ++i) in[nIn++] = q.ng[i] = nbr_grad_dev[i];
    }
    MICHK(dev_tgrad_arrays(who, in, nIn, flux_out_dev, 3));
    q.fc = p->faceCells.p; q.s[0] = patch_sfx_dev; q.s[1] = patch_sfy_dev; q.s[2] = patch_sfz_dev; q.visc = visc_dev; q.n = p->nFaces;
    for (int j = 0; j < 3; ++j) q.out[j] = flux_out_dev[j];
    HIPCHK(hipSetDevice(p->ctx->device));
    const dim3 grid((p->nFaces + 255) / 256), block(256);
    hipStream_t s = p->ctx->stream;
    if (kind == MI_DEV) { if (coupled) k_patch_dev_tgrad_flux<MI_DEV, true><<<grid, block, 0, s>>>(q); else k_patch_dev_tgrad_flux<MI_DEV, false><<<grid, block, 0, s>>>(q); }
    else { if (coupled) k_patch_dev_tgrad_flux<MI_DEV2, true><<<grid, block, 0, s>>>(q); else k_patch_dev_tgrad_flux<MI_DEV2, false><<<grid, block, 0, s>>>(q); }
    HIPCHK(hipGetLastError());
    return MI_OK;
}
extern "C" int mi_vec_axpby(mi_ctx_t c, int64_t n, double a, const double* x_dev, double b, const double* y_dev, double* out_dev)
{
    if (!c || n < 0 || (n > 0 && (!x_dev || !y_dev || !out_dev))) return fail(MI_ERR_ARG, "mi_vec_axpby: bad argument");
    if (!al16(x_dev) || !al16(y_dev) || !al16(out_dev)) return fail(MI_ERR_ARG, "mi_vec_axpby: arrays must be 16-byte aligned");
    if (n == 0) return MI_OK;
    return cell_launch(c, k_axpby, a, x_dev, b, y_dev, out_dev, n);
}
extern "C" int mi_vec_div(mi_ctx_t c, int64_t n, const double* x_dev, const double* y_dev, double* out_dev)
{
    if (!c || n < 0 || !x_dev || !y_dev || !out_dev) return fail(MI_ERR_ARG, "mi_vec_div: bad argument");
    if (!al16(x_dev) || !al16(y_dev) || !al16(out_dev)) return fail(MI_ERR_ARG, "mi_vec_div: arrays must be 16-byte aligned");
    return cell_launch(c, k_vdiv, x_dev, y_dev, out_dev, n);
}
