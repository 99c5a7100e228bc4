// mules.inc -- explicit MULES: limiter, limit and explicitSolve (included by engine.hip after reconstruct.inc; DESIGN 3.5l), and below them
// semi-implicit MULES (limiterCorr, limitCorr, correct) and the interfaceCompression scheme with the compression flux (DESIGN 3.5m).
//
//   limiter        MULESTemplates.C:381-745 with MULESFunctors.H: per cell the bounds over the NEIGHBOUR values (the cell's own value is not
//                  among them) and the boundary psiPf, sumPhiBD, sumPhip / mSumPhim from VSMALL with `phiCorr > 0.0` choosing the branch, the
//                  clamp by the global bounds, the static-mesh expressions of :538-554 one rounding per written operation; then nLimiterIter
//                  times the sums of lambda*phiCorr, lambdam / lambdap (names crossed as :637-638 cross them) and the face pass.
//   limit          :748-813: phiBD = phi*(w*(psiP - psiN) + psiN), w = pos(phi); phiCorr = phiPsi - phiBD; lambda = 1; the result
//                  phiBD + lambda*phiCorr (product rounded first) or lambda*phiCorr.
//   explicitSolve  :36-78 static mesh: surfaceIntegrate (own +, losort -, boundary +, then /V), then
//                  (rho0*psi0*rDeltaT + Su - that)/(rho*rDeltaT - Sp).
// A cell meets its faces in the order of 3.5k: own faces ascending, neighbour-side faces in losort order, boundary faces by patch then by face.
// An absent rho / Sp / Su is the reference's geometricOneField / zeroField: its operation is NOT performed (one*x = x, x - zero = x,
// zero - x = -x).  max / min are (a > b) ? a : b and (a < b) ? a : b (label.H:285-297), not fmax / fmin.  Everything is rounded operation by
// operation (-ffp-contract=off).  Restated in tests/mules_support.py, not pinned by a compiled reference.
namespace mi {

constexpr double MU_VSMALL = 1.0e-300, MU_SMALL = 1.0e-15;    // doubleScalar.H:55-57
enum { MU_OTHER = 0, MU_COUPLED = 1, MU_WEDGE = 2 };            // the kind of a boundary face's patch (mi_mules_s::bKind)

__device__ __forceinline__ double mu_max(double a, double b) { return (a > b) ? a : b; }
__device__ __forceinline__ double mu_min(double a, double b) { return (a < b) ? a : b; }

// the cell fields of mi_mules_fields and the handle's work arrays
struct MuCells {
    const double *rdtField, *rho, *rhoOld, *sp, *su, *vol, *psi, *psiOld, *bpsi;
    double rdt, psiMax, psiMin;
    double ec;                                        // CMULES: extremaCoeff*(psiMax - psiMin), formed once on the host
    double *maxn, *minn, *sumPhip, *mSumPhim, *lambdap, *lambdam;
    const uint8_t* bKind;
    const int32_t* bCell;
};
struct MuFlux {
    const double *phi, *bphi, *phiPsi, *bphiPsi;      // the limit form's inputs
    double *phiBD, *bphiBD, *phiCorr, *bphiCorr, *lambda, *blambda;
    double *out, *bout;
    int nf, nb, xcd, returnCorr;
};
struct MuArgs { RowTables r; MuCells q; MuFlux x; };  // one kernel argument, as row_launch passes it

// k_gauss_grad's / k_reconstruct's skeleton for NA staged face arrays: the block's own faces of src[0..NA) through LDS, the first four
// neighbour-side faces in registers before the one barrier, then per live cell own(f, v) for its own faces ascending, nei(f, v) for its
// neighbour-side faces in losort order, bnd(bf) for its boundary faces, done(); init(c) comes first
template <int BS, int NA, class Init, class Own, class Nei, class Bnd, class Done>
__device__ __forceinline__ void mu_rows(const RowTables& r, const double* const (&src)[NA], Init init, Own own, Nei nei, Bnd bnd, Done done)
{
    extern __shared__ __attribute__((aligned(16))) double mu_smem[];
    const int lb = r.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (r.blockStart) { c0 = r.blockStart[lb]; cEnd = r.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, r.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = r.os[c0], nf = r.os[cEnd] - f0;
    const bool staged = nf <= r.cap;
    if (staged) {
#pragma unroll
        for (int k = 0; k < NA; ++k) stage_dma8<BS>(src[k] + f0, mu_smem + k * r.cap, nf, tid);
    }
    int nb = 0, ne = 0;
    if (live) { nb = r.ls[c]; ne = r.ls[c + 1]; }
    const int cnt = ne - nb;
    int nfk[4]; double nv[4][NA];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                     // before the barrier: the faces LDS will not hold
        nfk[k] = (k < cnt) ? r.losort[nb + k] : 0;
        const bool cut = k < cnt && (!staged || nfk[k] < f0);
#pragma unroll
        for (int i = 0; i < NA; ++i) nv[k][i] = cut ? src[i][nfk[k]] : 0.0;
    }
    __syncthreads();
    if (!live) return;
    init(c);
    auto load = [&](int f, double (&v)[NA]) {
#pragma unroll
        for (int i = 0; i < NA; ++i) v[i] = (staged && f >= f0) ? mu_smem[i * r.cap + (f - f0)] : src[i][f];
    };
    const int ob = r.os[c], oe = r.os[c + 1];
    for (int f = ob; f < oe; ++f) { double v[NA]; load(f, v); own(c, f, v); }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) {
        if (staged && nfk[k] >= f0) {
#pragma unroll
            for (int i = 0; i < NA; ++i) nv[k][i] = mu_smem[i * r.cap + (nfk[k] - f0)];
        }
        nei(c, nfk[k], nv[k]);
    }
    for (int j = nb + 4; j < ne; ++j) { const int f = r.losort[j]; double v[NA]; load(f, v); nei(c, f, v); }
    if (r.bStart) for (int j = r.bStart[c]; j < r.bStart[c + 1]; ++j) bnd(c, r.bFace[j]);
    done(c);
}

// the opening row pass.  FORM_BD: the staged arrays are phi and phiPsi and the pass forms phiBD and phiCorr itself -- the owner side
// writes them (and lambda = 1) for its own faces, the neighbour side recomputes the same expression from the same operands, hence the same
// bits; a cell writes its boundary faces.  Otherwise the staged arrays are phiBD and phiCorr as given.
template <int BS, bool FORM_BD, bool LTS>
__global__ __launch_bounds__(BS) void k_mules_bounds(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    const double* const src[2] = {FORM_BD ? x.phi : x.phiBD, FORM_BD ? x.phiPsi : x.phiCorr};
    double psiC = 0.0, hi = q.psiMin, lo = q.psiMax, sumBD = 0.0, sp = MU_VSMALL, sm = MU_VSMALL;
    // phiBD and phiCorr of a face between P (owner) and N from phi and phiPsi: upwind weights 0 or 1, so a contracted w*(P - N) + N
    // would give the same bits
    auto form = [&](double phi, double phiPsi, double P, double N, double& bd, double& corr) {
        const double w = phi >= 0 ? 1.0 : 0.0, d = P - N, t = w * d, s = t + N;
        bd = phi * s; corr = phiPsi - bd;
    };
    auto plus = [&](double bd, double corr) { sumBD = sumBD + bd; if (corr > 0.0) sp = sp + corr; else sm = sm - corr; };
    mu_rows<BS, 2>(r, src,
        [&](int c) { if (FORM_BD) psiC = q.psi[c]; },
        [&](int, int f, const double (&v)[2]) {
            const double pn = q.psi[r.up[f]];
            double bd = v[0], corr = v[1];
            if (FORM_BD) { form(v[0], v[1], psiC, pn, bd, corr); x.phiBD[f] = bd; x.phiCorr[f] = corr; x.lambda[f] = 1.0; }
            hi = mu_max(hi, pn); lo = mu_min(lo, pn);
            plus(bd, corr);
        },
        [&](int, int f, const double (&v)[2]) {
            const double po = q.psi[r.lo[f]];
            double bd = v[0], corr = v[1];
            if (FORM_BD) form(v[0], v[1], po, psiC, bd, corr);
            hi = mu_max(hi, po); lo = mu_min(lo, po);
            sumBD = sumBD - bd;
            if (corr > 0.0) sm = sm + corr; else sp = sp - corr;
        },
        [&](int, int bf) {
            const double pf = q.bpsi[bf];
            double bd, corr;
            if (FORM_BD) {
                const double phi = x.bphi[bf];
                double face = pf;                     // surfaceInterpolationScheme.C:357-371
                if (q.bKind[bf] == MU_COUPLED) { const double w = phi >= 0 ? 1.0 : 0.0, a = w * psiC, b = (1.0 - w) * pf; face = a + b; }
                bd = phi * face; corr = x.bphiPsi[bf] - bd;
                x.bphiBD[bf] = bd; x.bphiCorr[bf] = corr; x.blambda[bf] = 1.0;
            } else { bd = x.bphiBD[bf]; corr = x.bphiCorr[bf]; }
            hi = mu_max(hi, pf); lo = mu_min(lo, pf);
            plus(bd, corr);
        },
        [&](int c) {
            hi = mu_min(hi, q.psiMax); lo = mu_max(lo, q.psiMin);
            const double rdt = LTS ? q.rdtField[c] : q.rdt;
            double coef = q.rho ? q.rho[c] * rdt : rdt;
            if (q.sp) coef = coef - q.sp[c];
            const double old = (q.rho ? q.rhoOld[c] * rdt : rdt) * q.psiOld[c], V = q.vol[c];
            double up = coef * hi;                    // :538-545
            if (q.su) up = up - q.su[c];
            up = up - old;
            up = V * up;
            q.maxn[c] = up + sumBD;
            double dn = coef * lo;                    // :547-554
            dn = q.su ? q.su[c] - dn : -dn;
            dn = dn + old;
            dn = V * dn;
            q.minn[c] = dn - sumBD;
            q.sumPhip[c] = sp; q.mSumPhim[c] = sm;
        });
}

// one limiter iteration's row pass: sumlPhip / mSumlPhim over lambda*phiCorr (the product rounded, its sign tested with > 0.0), then
// sumlPhipFinalMULESFunctor: lambdam from sumlPhip, psiMaxn and mSumPhim, lambdap from mSumlPhim, psiMinn and sumPhip
template <int BS>
__global__ __launch_bounds__(BS) void k_mules_sums(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    const double* const src[2] = {x.lambda, x.phiCorr};
    double slp = 0.0, mslm = 0.0;
    mu_rows<BS, 2>(r, src, [](int) {},
        [&](int, int, const double (&v)[2]) { const double p = v[0] * v[1]; if (p > 0.0) slp = slp + p; else mslm = mslm - p; },
        [&](int, int, const double (&v)[2]) { const double p = v[0] * v[1]; if (p > 0.0) mslm = mslm + p; else slp = slp - p; },
        [&](int, int bf) { const double p = x.blambda[bf] * x.bphiCorr[bf]; if (p > 0.0) slp = slp + p; else mslm = mslm - p; },
        [&](int c) {
            q.lambdam[c] = mu_max(mu_min((slp + q.maxn[c]) / (q.mSumPhim[c] - MU_SMALL), 1.0), 0.0);
            q.lambdap[c] = mu_max(mu_min((mslm + q.minn[c]) / (q.sumPhip[c] + MU_SMALL), 1.0), 0.0);
        });
}

// one limiter iteration's face pass (lambdaIfMULESFunctor and the three patch branches of :672-741), lambda in place: the internal faces
// in XCD-aware chunks as k_limited_weights, then the boundary faces grid-stride in the same launch.  CORR: the one rule CMULES changes
// (patchLambdaPfCMULESFunctor, CMULESTemplates.C:345-371): a face of a patch that is neither coupled nor wedge is limited where the boundary
// value of phi is > SMALL*SMALL, not phiBD + phiCorr; phiBD is then never read
template <bool CORR>
__global__ __launch_bounds__(256) void k_mules_lambda(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    int f0, f1; block_chunk(x.nf, x.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = r.lo[f], N = r.up[f];
        const double l = x.lambda[f];
        x.lambda[f] = x.phiCorr[f] > 0.0 ? mu_min(l, mu_min(q.lambdap[P], q.lambdam[N])) : mu_min(l, mu_min(q.lambdam[P], q.lambdap[N]));
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < x.nb; i += (int64_t)gridDim.x * blockDim.x) {
        const int kind = q.bKind[i];
        if (kind == MU_WEDGE) { x.blambda[i] = 0.0; continue; }
        const double corr = x.bphiCorr[i];
        if (kind != MU_COUPLED && !((CORR ? x.bphi[i] : x.bphiBD[i] + corr) > MU_SMALL * MU_SMALL)) continue;   // limit outlet faces only
        const int c = q.bCell[i];
        x.blambda[i] = mu_min(x.blambda[i], corr > 0.0 ? q.lambdap[c] : q.lambdam[c]);
    }
}

// the opening row pass of limiterCorr (limiterCMULESFunctor, patchMinMaxCMULESFunctor, CMULESTemplates.C:160-343, :441-517): one staged
// array, phiCorr.  As the explicit pass the bounds run over the NEIGHBOUR cells' psi and the boundary psiPf from the global psiMin / psiMax
// (the cell's own value is not among them) and sumPhip / mSumPhim from VSMALL; there is no phiBD.  The clamp adds q.ec even when it is 0.0
// (-0.0 + 0.0 = +0.0), and the old-value term is (rho*psi)*rDeltaT of the CURRENT psi and rho.  ONES (limitCorr): lambda = 1 as well, the
// owner side writes its own faces and a cell its boundary faces.
template <int BS, bool ONES, bool LTS>
__global__ __launch_bounds__(BS) void k_mules_corr_bounds(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    const double* const src[1] = {x.phiCorr};
    double hi = q.psiMin, lo = q.psiMax, sp = MU_VSMALL, sm = MU_VSMALL;
    mu_rows<BS, 1>(r, src, [](int) {},
        [&](int, int f, const double (&v)[1]) {
            const double pn = q.psi[r.up[f]];
            if (ONES) x.lambda[f] = 1.0;
            hi = mu_max(hi, pn); lo = mu_min(lo, pn);
            if (v[0] > 0.0) sp = sp + v[0]; else sm = sm - v[0];
        },
        [&](int, int f, const double (&v)[1]) {
            const double po = q.psi[r.lo[f]];
            hi = mu_max(hi, po); lo = mu_min(lo, po);
            if (v[0] > 0.0) sm = sm + v[0]; else sp = sp - v[0];     // :246-254
        },
        [&](int, int bf) {
            const double pf = q.bpsi[bf], corr = x.bphiCorr[bf];
            if (ONES) x.blambda[bf] = 1.0;
            hi = mu_max(hi, pf); lo = mu_min(lo, pf);
            if (corr > 0.0) sp = sp + corr; else sm = sm - corr;
        },
        [&](int c) {
            hi = mu_min(hi + q.ec, q.psiMax); lo = mu_max(lo - q.ec, q.psiMin);   // :496-497
            const double rdt = LTS ? q.rdtField[c] : q.rdt, psiC = q.psi[c];
            double coef = q.rho ? q.rho[c] * rdt : rdt;
            if (q.sp) coef = coef - q.sp[c];
            const double old = (q.rho ? q.rho[c] * psiC : psiC) * rdt, V = q.vol[c];
            double up = coef * hi;                    // :503-509
            if (q.su) up = up - q.su[c];
            up = up - old;
            q.maxn[c] = V * up;
            double dn = coef * lo;                    // :511-517
            dn = q.su ? q.su[c] - dn : -dn;
            dn = dn + old;
            q.minn[c] = V * dn;
            q.sumPhip[c] = sp; q.mSumPhim[c] = sm;
        });
}

// phiBD + lambda*phiCorr, or lambda*phiCorr with returnCorr: internal and boundary faces in one launch.  out may be phiCorr itself
// (limitCorr's phiCorr *= lambda): a face reads and writes its own element only
__global__ __launch_bounds__(256) void k_mules_apply(const MuFlux x)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t f = t0; f < x.nf; f += step) { const double p = x.lambda[f] * x.phiCorr[f]; x.out[f] = x.returnCorr ? p : x.phiBD[f] + p; }
    for (int64_t i = t0; i < x.nb; i += step) { const double p = x.blambda[i] * x.bphiCorr[i]; x.bout[i] = x.returnCorr ? p : x.bphiBD[i] + p; }
}

// explicitSolve: surfaceIntegrate(x.phiPsi) and the final expression; x.out is the new psi, a cell array.  MULES::correct
// (CMULESTemplates.C:35-74) is the same expression with rho and psi in the places of rho0 and psi0, x.out psi itself: a cell reads its own
// psi before it writes it and no other cell's
template <int BS, bool LTS>
__global__ __launch_bounds__(BS) void k_mules_solve(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    const double* const src[1] = {x.phiPsi};
    double s = 0.0;
    mu_rows<BS, 1>(r, src, [](int) {},
        [&](int, int, const double (&v)[1]) { s = s + v[0]; },
        [&](int, int, const double (&v)[1]) { s = s - v[0]; },
        [&](int, int bf) { s = s + x.bphiPsi[bf]; },
        [&](int c) {
            const double rdt = LTS ? q.rdtField[c] : q.rdt, integ = s / q.vol[c];
            double num = q.rho ? q.rhoOld[c] * q.psiOld[c] : q.psiOld[c];
            num = num * rdt;
            if (q.su) num = num + q.su[c];
            num = num - integ;
            double den = q.rho ? q.rho[c] * rdt : rdt;
            if (q.sp) den = den - q.sp[c];
            x.out[c] = num / den;
        });
}

// the cell of every boundary face from the per-cell lists, once per handle
__global__ __launch_bounds__(256) void k_mules_bcell(const int32_t* bStart, const int32_t* bFace, int32_t* bCell, int n)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (int j = bStart[c]; j < bStart[c + 1]; ++j) bCell[bFace[j]] = c;
}

__global__ __launch_bounds__(RB) void k_vmin(const double* x, const double* y, double* out, int64_t n) // out may alias x or y
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = mu_min(x[i], y[i]);
}

} // namespace mi

// explicit MULES on one mesh: the six cell work arrays and the boundary faces' kinds and cells
struct mi_mules_s : RowHandle {
    bool coupled = false, begun = false;
    bool corr = false;                                // the last begin was mi_mules_begin_corr: the iteration takes the CMULES patch rule
    bool hasOther = false;                            // a face on a patch that is neither coupled nor wedge: the CMULES rule reads b_phi there
    DevBuf<double> work[6];                           // psiMaxn, psiMinn (transformed), sumPhip, mSumPhim, lambdap, lambdam
    DevBuf<uint8_t> bKind;
    DevBuf<int32_t> bCell;
};

namespace {
enum { MU_CELL, MU_FACE, MU_BFACE };                 // what an array of a checked call is indexed by
struct MuCall {                                       // one checked call: the kernels' arguments
    MuArgs a{};
    bool lts = false;
};
// the checks every staged entry shares: the handle, the fields, the listed flux arrays (in: read, out: written); fills c
// mode: which cell fields the call reads.  MU_EXPLICIT: all of them.  MU_CORR (semi-implicit MULES): psi and rho are the current ones,
// psi_old_dev and rho_old_dev are not looked at.  MU_CORRECT (mi_mules_correct): psi is the output array, psi_dev is not looked at either.
enum { MU_EXPLICIT, MU_CORR, MU_CORRECT };
int mu_check(const std::string& who, mi_mules_s* h, const mi_mules_fields* fl, const double* const* in, const int* inKind, int nIn,
             double* const* out, const int* outKind, int nOut, MuCall& c, int mode = MU_EXPLICIT)
{
    mi_addr_s* a = h->addr;
    MICHK(row_handle_check(who, h));
    if (!fl) return fail(MI_ERR_ARG, who + ": the fields are missing");
    const bool old = mode == MU_EXPLICIT;
    const double* psi = mode == MU_CORRECT ? nullptr : fl->psi_dev;
    if (!fl->vol_dev || (mode != MU_CORRECT && !psi) || (old && !fl->psi_old_dev)) return fail(MI_ERR_ARG, who + ": a cell array is missing");
    if (old && (fl->rho_dev != nullptr) != (fl->rho_old_dev != nullptr)) return fail(MI_ERR_ARG, who + ": rho and rho_old come together or not at all");
    const bool hasF = h->nFaces > 0, hasB = h->nBFaces > 0;
    auto present = [&](int kind) { return kind == MU_CELL || (kind == MU_FACE ? hasF : hasB); };   // an empty array may be NULL and is never read
    const double* bpsi = (hasB && mode != MU_CORRECT) ? fl->b_psi_dev : nullptr;     // correct reads no boundary psi
    if (hasB && mode != MU_CORRECT && !bpsi) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary psi needed");
    const double* all[40];
    int m = 0;
    const double* cells[9] = {fl->r_delta_t_dev, fl->rho_dev, old ? fl->rho_old_dev : nullptr, fl->sp_dev, fl->su_dev, fl->vol_dev, psi,
                              old ? fl->psi_old_dev : nullptr, bpsi};
    for (const double* p : cells) if (p) all[m++] = p;
    for (int i = 0; i < nIn; ++i) {
        if (!present(inKind[i])) continue;
        if (!in[i]) return fail(MI_ERR_ARG, who + (inKind[i] != MU_BFACE ? ": an input array is missing" : ": the boundary has faces: boundary flux arrays needed"));
        all[m++] = in[i];
    }
    for (int i = 0; i < 6; ++i) all[m++] = h->work[i].p;
    double* outs[8];
    int mo = 0;
    for (int i = 0; i < nOut; ++i) {
        if (!present(outKind[i])) continue;
        if (!out[i]) return fail(MI_ERR_ARG, who + (outKind[i] != MU_BFACE ? ": an output array is missing" : ": the boundary has faces: boundary flux arrays needed"));
        outs[mo++] = out[i];
    }
    MICHK(arrays_aligned8(who, (const void* const*)all, m));
    MICHK(arrays_aligned8(who, (const void* const*)outs, mo));
    MICHK(outputs_distinct(who, all, m, outs, mo));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    c.a.r = row_tables(a, h->boundary);
    MuCells& q = c.a.q;
    q.rdtField = fl->r_delta_t_dev; q.rdt = fl->r_delta_t; q.rho = fl->rho_dev; q.rhoOld = old ? fl->rho_old_dev : fl->rho_dev; q.sp = fl->sp_dev; q.su = fl->su_dev;
    q.vol = fl->vol_dev; q.psi = psi; q.psiOld = old ? fl->psi_old_dev : psi; q.bpsi = bpsi; q.psiMax = fl->psi_max; q.psiMin = fl->psi_min;
    q.maxn = h->work[0].p; q.minn = h->work[1].p; q.sumPhip = h->work[2].p; q.mSumPhim = h->work[3].p; q.lambdap = h->work[4].p; q.lambdam = h->work[5].p;
    q.bKind = h->bKind.p; q.bCell = h->bCell.p;
    c.lts = fl->r_delta_t_dev != nullptr;
    c.a.x.nf = h->nFaces; c.a.x.nb = h->nBFaces; c.a.x.xcd = a->ctx->xcdRows;
    return MI_OK;
}
const int kMuFB[8] = {MU_FACE, MU_BFACE, MU_FACE, MU_BFACE, MU_FACE, MU_BFACE, MU_FACE, MU_BFACE};

int mu_begin(const std::string& who, mi_mules_s* h, int form, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c)
{
    if (form != MI_MULES_LIMITER && form != MI_MULES_LIMIT) return fail(MI_ERR_ARG, who + ": form must be MI_MULES_LIMITER or MI_MULES_LIMIT");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    if (form == MI_MULES_LIMIT) {
        const double* in[4] = {fx->phi_dev, fx->b_phi_dev, fx->phi_psi_dev, fx->b_phi_psi_dev};
        double* out[6] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev, fx->lambda_dev, fx->b_lambda_dev};
        MICHK(mu_check(who, h, fl, in, kMuFB, 4, out, kMuFB, 6, c));
    } else {
        const double* in[6] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev, fx->lambda_dev, fx->b_lambda_dev};
        MICHK(mu_check(who, h, fl, in, kMuFB, 6, nullptr, nullptr, 0, c));
    }
    return MI_OK;
}
void mu_flux(const mi_mules_flux* fx, MuFlux& x)
{
    x.phi = fx->phi_dev; x.bphi = fx->b_phi_dev; x.phiPsi = fx->phi_psi_dev; x.bphiPsi = fx->b_phi_psi_dev;
    x.phiBD = fx->phi_bd_dev; x.bphiBD = fx->b_phi_bd_dev; x.phiCorr = fx->phi_corr_dev; x.bphiCorr = fx->b_phi_corr_dev;
    x.lambda = fx->lambda_dev; x.blambda = fx->b_lambda_dev; x.out = fx->out_dev; x.bout = fx->b_out_dev;
}
int mu_launch_begin(mi_mules_s* h, int form, MuCall& c)
{
    if (h->nCells == 0) { h->begun = true; h->corr = false; return MI_OK; }
    mi_addr_s* a = h->addr;
    int r;
    if (form == MI_MULES_LIMIT) r = c.lts ? row_launch_bs(a, 2, ROW_BS(k_mules_bounds, true, true), c.a) : row_launch_bs(a, 2, ROW_BS(k_mules_bounds, true, false), c.a);
    else r = c.lts ? row_launch_bs(a, 2, ROW_BS(k_mules_bounds, false, true), c.a) : row_launch_bs(a, 2, ROW_BS(k_mules_bounds, false, false), c.a);
    if (r == MI_OK) { h->begun = true; h->corr = false; }
    return r;
}
// the CMULES patch rule reads the boundary value of phi on every face of a patch that is neither coupled nor wedge
int mu_needs_bphi(const std::string& who, const mi_mules_s* h, const mi_mules_flux* fx)
{
    if (h->hasOther && !fx->b_phi_dev)
        return fail(MI_ERR_ARG, who + ": the boundary has a patch that is neither coupled nor wedge: b_phi_dev needed");
    return MI_OK;
}
// the opening of limiterCorr: phi_corr (and, on the patches the rule reads it, b_phi) as given; lambda written (CORR_LIMIT) or as given
int mu_begin_corr(const std::string& who, mi_mules_s* h, int form, double extremaCoeff, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c)
{
    if (form != MI_MULES_CORR_LIMITER && form != MI_MULES_CORR_LIMIT)
        return fail(MI_ERR_ARG, who + ": form must be MI_MULES_CORR_LIMITER or MI_MULES_CORR_LIMIT");
    if (!std::isfinite(extremaCoeff) || extremaCoeff < 0) return fail(MI_ERR_ARG, who + ": extrema_coeff must be a finite number and not negative");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    MICHK(mu_needs_bphi(who, h, fx));
    const int kind[5] = {MU_FACE, MU_BFACE, MU_BFACE, MU_FACE, MU_BFACE};
    const double* in[5] = {fx->phi_corr_dev, fx->b_phi_corr_dev, fx->b_phi_dev, fx->lambda_dev, fx->b_lambda_dev};
    double* out[2] = {fx->lambda_dev, fx->b_lambda_dev};
    const int nIn = h->hasOther ? 3 : 2;
    if (form == MI_MULES_CORR_LIMIT) {
        MICHK(mu_check(who, h, fl, in, kind, nIn, out, kMuFB, 2, c, MU_CORR));
    } else {
        const double* given[5] = {in[0], in[1], in[3], in[4], in[2]};
        const int givenKind[5] = {MU_FACE, MU_BFACE, MU_FACE, MU_BFACE, MU_BFACE};
        MICHK(mu_check(who, h, fl, given, givenKind, nIn + 2, nullptr, nullptr, 0, c, MU_CORR));
    }
    c.a.q.ec = extremaCoeff * (fl->psi_max - fl->psi_min);
    return MI_OK;
}
int mu_launch_begin_corr(mi_mules_s* h, int form, MuCall& c)
{
    int r = MI_OK;
    if (h->nCells > 0) {
        mi_addr_s* a = h->addr;
        if (form == MI_MULES_CORR_LIMIT) r = c.lts ? row_launch_bs(a, 1, ROW_BS(k_mules_corr_bounds, true, true), c.a) : row_launch_bs(a, 1, ROW_BS(k_mules_corr_bounds, true, false), c.a);
        else r = c.lts ? row_launch_bs(a, 1, ROW_BS(k_mules_corr_bounds, false, true), c.a) : row_launch_bs(a, 1, ROW_BS(k_mules_corr_bounds, false, false), c.a);
    }
    if (r == MI_OK) { h->begun = true; h->corr = true; }
    return r;
}
// corr: the state the iteration runs in (the handle's, or the one the convenience is about to open)
int mu_check_iterate(const std::string& who, mi_mules_s* h, int n, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c, bool begunByCaller, bool corr)
{
    if (n < 0) return fail(MI_ERR_ARG, who + ": n must not be negative");
    if (!begunByCaller && !h->begun) return fail(MI_ERR_ARG, who + ": called before mi_mules_begin");
    if (n > 1 && h->coupled)
        return fail(MI_ERR_ARG, who + ": the boundary has coupled patches: the minOp sync between iterations is the caller's, iterate one at a time");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    double* out[2] = {fx->lambda_dev, fx->b_lambda_dev};
    if (corr) {
        MICHK(mu_needs_bphi(who, h, fx));
        const int kind[3] = {MU_FACE, MU_BFACE, MU_BFACE};
        const double* in[3] = {fx->phi_corr_dev, fx->b_phi_corr_dev, fx->b_phi_dev};
        return mu_check(who, h, fl, in, kind, h->hasOther ? 3 : 2, out, kMuFB, 2, c, MU_CORR);
    }
    const double* in[4] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev};
    return mu_check(who, h, fl, in, kMuFB, 4, out, kMuFB, 2, c);
}
int mu_launch_iterate(mi_mules_s* h, int n, MuCall& c, bool corr)
{
    if (h->nCells == 0) return MI_OK;
    mi_addr_s* a = h->addr;
    const int64_t faces = std::max<int64_t>(h->nFaces, h->nBFaces);
    for (int j = 0; j < n; ++j) {
        MICHK(row_launch_bs(a, 2, ROW_BS(k_mules_sums), c.a));
        if (faces > 0) {
            if (corr) k_mules_lambda<true><<<grid_for(a->ctx, (int)faces), 256, 0, a->ctx->stream>>>(c.a);
            else k_mules_lambda<false><<<grid_for(a->ctx, (int)faces), 256, 0, a->ctx->stream>>>(c.a);
            HIPCHK(hipGetLastError());
        }
    }
    return MI_OK;
}
int mu_check_apply(const std::string& who, mi_mules_s* h, int returnCorr, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c, bool begunByCaller,
                   bool corr)
{
    if (!begunByCaller && !h->begun) return fail(MI_ERR_ARG, who + ": called before mi_mules_begin");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    double* out[2] = {fx->out_dev, fx->b_out_dev};
    if (corr) {                                       // phiCorr *= lambda: there is no phiBD; out may be phi_corr, b_out b_phi_corr
        if (!returnCorr) return fail(MI_ERR_ARG, who + ": after mi_mules_begin_corr there is no phi_bd: return_corr must be 1");
        if ((h->nFaces > 0 && !fx->phi_corr_dev) || (h->nBFaces > 0 && !fx->b_phi_corr_dev))
            return fail(MI_ERR_ARG, who + (h->nFaces > 0 && !fx->phi_corr_dev ? ": an input array is missing" : ": the boundary has faces: boundary flux arrays needed"));
        const double* in[4] = {fx->lambda_dev, fx->b_lambda_dev, nullptr, nullptr};
        int n = 2;
        int k[4] = {MU_FACE, MU_BFACE, 0, 0};
        if (fx->out_dev != fx->phi_corr_dev) { in[n] = fx->phi_corr_dev; k[n++] = MU_FACE; }
        if (fx->b_out_dev != fx->b_phi_corr_dev) { in[n] = fx->b_phi_corr_dev; k[n++] = MU_BFACE; }
        const double* pa[2] = {fx->phi_corr_dev, fx->b_phi_corr_dev};     // an aliased one is an output to the checks below: aligned like them
        MICHK(arrays_aligned8(who, (const void* const*)pa, 2));
        return mu_check(who, h, fl, in, k, n, out, kMuFB, 2, c, MU_CORR);
    }
    const double* in[6] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev, fx->lambda_dev, fx->b_lambda_dev};
    return mu_check(who, h, fl, in, kMuFB, 6, out, kMuFB, 2, c);
}
int mu_launch_apply(mi_mules_s* h, int returnCorr, MuCall& c)
{
    const int64_t faces = std::max<int64_t>(h->nFaces, h->nBFaces);
    if (h->nCells == 0 || faces == 0) return MI_OK;
    c.a.x.returnCorr = returnCorr ? 1 : 0;
    k_mules_apply<<<grid_for(h->ctx, (int)faces), 256, 0, h->ctx->stream>>>(c.a.x);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
int mu_no_couples(const std::string& who, const mi_mules_s* h)
{
    if (h->coupled) return fail(MI_ERR_ARG, who + ": the boundary has coupled patches: the minOp sync between iterations is the caller's, use "
                                                  "mi_mules_begin, mi_mules_iterate one at a time and mi_mules_apply");
    return MI_OK;
}
} // namespace

extern "C" int mi_mules_create(mi_addr_t a, mi_grad_boundary_t b, const int32_t* patch_is_wedge_host_or_null, mi_mules_t* out)
{
    const std::string who = "mi_mules_create";
    std::unique_ptr<mi_mules_s> h(new mi_mules_s());
    MICHK(row_handle_open(who, a, b, out, *h));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (h->nCells == 0) { *out = h.release(); return MI_OK; }
    for (int i = 0; i < 6; ++i) MICHK(h->work[i].alloc((size_t)h->nCells));
    if (h->nBFaces > 0) {
        Table<uint8_t> kind((size_t)h->nBFaces);
        size_t off = 0;
        for (size_t p = 0; p < b->patchSizes.size(); ++p) {
            const bool wedge = patch_is_wedge_host_or_null && patch_is_wedge_host_or_null[p] != 0;
            const bool cpl = b->patchKinds[p] == MI_GRAD_PATCH_COUPLED;
            if (cpl && !wedge && b->patchSizes[p] > 0) h->coupled = true;
            if (!cpl && !wedge && b->patchSizes[p] > 0) h->hasOther = true;
            for (int32_t i = 0; i < b->patchSizes[p]; ++i) kind[off++] = wedge ? MU_WEDGE : cpl ? MU_COUPLED : MU_OTHER;
        }
        hipStream_t s = a->ctx->stream;
        MICHK(h->bKind.upload(kind, s));
        MICHK(h->bCell.alloc((size_t)h->nBFaces));
        k_mules_bcell<<<(h->nCells + 255) / 256, 256, 0, s>>>(b->allStart.p, b->all.p, h->bCell.p, h->nCells);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    *out = h.release();
    return MI_OK;
}
extern "C" int mi_mules_destroy(mi_mules_t h) { delete h; return MI_OK; }

extern "C" int mi_mules_work(mi_mules_t h, double* const* out_dev)
{
    const std::string who = "mi_mules_work";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    if (h->nCells == 0) return MI_OK;
    if (!out_dev) return fail(MI_ERR_ARG, who + ": output arrays missing");
    const double* in[6];
    for (int i = 0; i < 6; ++i) in[i] = h->work[i].p;
    MICHK(outputs_distinct(who, in, 6, out_dev, 6));
    MICHK(arrays_aligned8(who, (const void* const*)out_dev, 6));
    HIPCHK(hipSetDevice(h->ctx->device));
    for (int i = 0; i < 6; ++i)
        HIPCHK(hipMemcpyAsync(out_dev[i], h->work[i].p, (size_t)h->nCells * sizeof(double), hipMemcpyDeviceToDevice, h->ctx->stream));
    return MI_OK;
}

extern "C" int mi_mules_begin(mi_mules_t h, int32_t form, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_begin";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MuCall c;
    MICHK(mu_begin(who, h, form, fields, flux, c));
    mu_flux(flux, c.a.x);
    return mu_launch_begin(h, form, c);
}

extern "C" int mi_mules_iterate(mi_mules_t h, int32_t n, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_iterate";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MuCall c;
    MICHK(mu_check_iterate(who, h, n, fields, flux, c, false, h->corr));
    mu_flux(flux, c.a.x);
    return mu_launch_iterate(h, n, c, h->corr);
}

extern "C" int mi_mules_apply(mi_mules_t h, int32_t return_corr, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_apply";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MuCall c;
    MICHK(mu_check_apply(who, h, return_corr, fields, flux, c, false, h->corr));
    mu_flux(flux, c.a.x);
    return mu_launch_apply(h, return_corr, c);
}

extern "C" int mi_mules_limiter(mi_mules_t h, int32_t n_limiter_iter, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_limiter";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(mu_no_couples(who, h));
    MuCall c, ci;                                     // every check before the first launch
    MICHK(mu_begin(who, h, MI_MULES_LIMITER, fields, flux, c));
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true, false));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x);
    MICHK(mu_launch_begin(h, MI_MULES_LIMITER, c));
    return mu_launch_iterate(h, n_limiter_iter, ci, false);
}

extern "C" int mi_mules_limit(mi_mules_t h, int32_t n_limiter_iter, int32_t return_corr, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_limit";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(mu_no_couples(who, h));
    MuCall c, ci, ca;
    MICHK(mu_begin(who, h, MI_MULES_LIMIT, fields, flux, c));
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true, false));
    MICHK(mu_check_apply(who, h, return_corr, fields, flux, ca, true, false));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x); mu_flux(flux, ca.a.x);
    MICHK(mu_launch_begin(h, MI_MULES_LIMIT, c));
    MICHK(mu_launch_iterate(h, n_limiter_iter, ci, false));
    return mu_launch_apply(h, return_corr, ca);
}

// ---- semi-implicit MULES (CMULESTemplates.C:35-758; DESIGN 3.5m) -----------------------------------------------------------------------
extern "C" int mi_mules_begin_corr(mi_mules_t h, int32_t form, double extrema_coeff, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_begin_corr";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MuCall c;
    MICHK(mu_begin_corr(who, h, form, extrema_coeff, fields, flux, c));
    mu_flux(flux, c.a.x);
    return mu_launch_begin_corr(h, form, c);
}

extern "C" int mi_mules_limiter_corr(mi_mules_t h, int32_t n_limiter_iter, double extrema_coeff, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_limiter_corr";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(mu_no_couples(who, h));
    MuCall c, ci;                                     // every check before the first launch
    MICHK(mu_begin_corr(who, h, MI_MULES_CORR_LIMITER, extrema_coeff, fields, flux, c));
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true, true));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x);
    MICHK(mu_launch_begin_corr(h, MI_MULES_CORR_LIMITER, c));
    return mu_launch_iterate(h, n_limiter_iter, ci, true);
}

// limitCorr (:706-758): lambda = 1, limiterCorr, phiCorr *= lambda in place
extern "C" int mi_mules_limit_corr(mi_mules_t h, int32_t n_limiter_iter, double extrema_coeff, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_limit_corr";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(mu_no_couples(who, h));
    MuCall c, ci, ca;
    MICHK(mu_begin_corr(who, h, MI_MULES_CORR_LIMIT, extrema_coeff, fields, flux, c));
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true, true));
    mi_mules_flux inPlace = *flux;
    inPlace.out_dev = flux->phi_corr_dev; inPlace.b_out_dev = flux->b_phi_corr_dev;
    MICHK(mu_check_apply(who, h, 1, fields, &inPlace, ca, true, true));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x); mu_flux(&inPlace, ca.a.x);
    MICHK(mu_launch_begin_corr(h, MI_MULES_CORR_LIMIT, c));
    MICHK(mu_launch_iterate(h, n_limiter_iter, ci, true));
    return mu_launch_apply(h, 1, ca);
}

// MULES::correct (:35-74): psi = (rho*psi*rDeltaT + Su - surfaceIntegrate(phiCorr))/(rho*rDeltaT - Sp) in place, on k_mules_solve
extern "C" int mi_mules_correct(mi_mules_t h, const mi_mules_fields* fields, const double* phi_corr_dev, const double* b_phi_corr_dev, double* psi_inout_dev)
{
    const std::string who = "mi_mules_correct";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    if (h->nCells == 0) return MI_OK;
    MuCall c;
    const double* in[2] = {phi_corr_dev, b_phi_corr_dev};
    double* out[1] = {psi_inout_dev};
    const int cellOut[1] = {MU_CELL};
    MICHK(mu_check(who, h, fields, in, kMuFB, 2, out, cellOut, 1, c, MU_CORRECT));
    c.a.q.psiOld = psi_inout_dev;                     // rhoOld is rho already
    c.a.x.phiPsi = phi_corr_dev; c.a.x.bphiPsi = b_phi_corr_dev; c.a.x.out = psi_inout_dev;
    mi_addr_s* a = h->addr;
    return c.lts ? row_launch_bs(a, 1, ROW_BS(k_mules_solve, true), c.a) : row_launch_bs(a, 1, ROW_BS(k_mules_solve, false), c.a);
}

extern "C" int mi_mules_explicit_solve(mi_mules_t h, const mi_mules_fields* fields, const double* phi_psi_dev, const double* b_phi_psi_dev,
                                       double* psi_out_dev)
{
    const std::string who = "mi_mules_explicit_solve";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    if (h->nCells == 0) return MI_OK;
    MuCall c;
    const double* in[2] = {phi_psi_dev, b_phi_psi_dev};
    double* out[1] = {psi_out_dev};
    const int cellOut[1] = {MU_CELL};
    // the solve reads no psi: it may be NULL or psi_out itself (the reference overwrites psi.internalField())
    mi_mules_fields fl{};
    if (fields) { fl = *fields; if (!fl.psi_dev || fl.psi_dev == psi_out_dev) fl.psi_dev = fl.psi_old_dev; fields = &fl; }
    MICHK(mu_check(who, h, fields, in, kMuFB, 2, out, cellOut, 1, c));
    c.a.x.phiPsi = phi_psi_dev; c.a.x.bphiPsi = b_phi_psi_dev; c.a.x.out = psi_out_dev;
    mi_addr_s* a = h->addr;
    return c.lts ? row_launch_bs(a, 1, ROW_BS(k_mules_solve, true), c.a) : row_launch_bs(a, 1, ROW_BS(k_mules_solve, false), c.a);
}

extern "C" int mi_vec_min(mi_ctx_t c, int64_t n, const double* x_dev, const double* y_dev, double* out_dev)
{
    if (!c || n < 0 || (n > 0 && (!x_dev || !y_dev || !out_dev))) return fail(MI_ERR_ARG, "mi_vec_min: bad argument");
    if (!al8(x_dev) || !al8(y_dev) || !al8(out_dev)) return fail(MI_ERR_ARG, "mi_vec_min: arrays must be aligned to 8 bytes");
    if (n == 0) return MI_OK;
    return cell_launch(c, k_vmin, x_dev, y_dev, out_dev, n);
}

// ---- the interfaceCompression scheme and the compression flux of alphaEqn.H (DESIGN 3.5m) ------------------------------------------------
// interfaceCompression.H:58-77 inside PhiScheme.C:52-197: the limiter reads the two cell values only; the weights are
// limitedSurfaceInterpolationScheme's blend, as k_limited_weights forms it.  A device functor, so the rule of 3.5a / 3.5b: 4*x is exact and
// 1 - (4*x)*(1 - x) one product under a sum, hence one fma; sqr a plain product; max / min the reference's ternaries.
namespace mi {

__device__ __forceinline__ double ic_limiter(double P, double N)
{
    const double a = fma(-(4.0 * P), 1.0 - P, 1.0), b = fma(-(4.0 * N), 1.0 - N, 1.0);
    return rmin(rmax(1.0 - rmax(a * a, b * b), 0.0), 1.0);
}
__device__ __forceinline__ double ic_weight(double lim, double cdw, double fl) { return fma(lim, cdw, (1.0 - lim) * (fl >= 0 ? 1.0 : 0.0)); }

// fvc::flux(-fvc::flux(-phir, alpha2, interfaceCompression), alpha1, interfaceCompression) on one face, alpha2 = 1.0 - alpha1 per cell: the
// unfused sequence operation for operation.  PATCH: a coupled patch face interpolates as surfaceInterpolationScheme.C:361-366 does,
// w*P + (1 - w)*N with every operator rounded; an internal face as mi_face_interpolate does (:273-279, one fma)
template <bool PATCH>
__device__ __forceinline__ double ic_compression_flux(double cdw, double phir, double a1P, double a1N)
{
    auto interpolate = [](double w, double P, double N) { return PATCH ? w * P + (1.0 - w) * N : fma(w, P - N, N); };
    const double a2P = 1.0 - a1P, a2N = 1.0 - a1N;
    const double n = -phir;
    const double g = n * interpolate(ic_weight(ic_limiter(a2P, a2N), cdw, n), a2P, a2N);
    const double m = -g;
    return m * interpolate(ic_weight(ic_limiter(a1P, a1N), cdw, m), a1P, a1N);
}

struct IcArgs {
    const int32_t *lo, *up;                           // internal faces; the patch form: lo = faceCells, nbr the patchNeighbourField
    const double *cdw, *flux, *alpha, *nbr;
    double *w, *limOut;                               // the flux form writes w only
    int nf, xcd;
};
// the internal faces: XCD-aware chunks as k_limited_weights; cdw and the flux streamed, alpha gathered twice
template <bool FLUX>
__global__ __launch_bounds__(256) void k_interface_compression(const IcArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const double P = a.alpha[a.lo[f]], N = a.alpha[a.up[f]], fl = a.flux[f], cdw = a.cdw[f];
        if (FLUX) a.w[f] = ic_compression_flux<false>(cdw, fl, P, N);
        else {
            const double lim = ic_limiter(P, N);
            if (a.limOut) a.limOut[f] = lim;
            a.w[f] = ic_weight(lim, cdw, fl);
        }
    }
}
// one COUPLED patch (PhiScheme.C:145-189): patchInternalField through faceCells, patchNeighbourField the caller's
template <bool FLUX>
__global__ __launch_bounds__(256) void k_patch_interface_compression(const IcArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nf) return;
    const double P = a.alpha[a.lo[i]], N = a.nbr[i], fl = a.flux[i], cdw = a.cdw[i];
    if (FLUX) a.w[i] = ic_compression_flux<true>(cdw, fl, P, N);
    else {
        const double lim = ic_limiter(P, N);
        if (a.limOut) a.limOut[i] = lim;
        a.w[i] = ic_weight(lim, cdw, fl);
    }
}

} // namespace mi

namespace {
template <bool FLUX>
int ic_internal(const char* who, mi_addr_s* a, const double* cdw, const double* flux, const double* alpha, double* out, double* limOut)
{
    if (!a) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (!alpha) return fail(MI_ERR_ARG, std::string(who) + ": input arrays missing");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    const double* in[3] = {cdw, flux, alpha};
    MICHK(lim_outputs(who, in, 3, out, limOut));
    if (!al16(cdw) || !al16(flux) || !al16(out) || (limOut && !al16(limOut)) || !al8(alpha))
        return fail(MI_ERR_ARG, std::string(who) + ": face fields must be 16-byte aligned, the cell field to 8 bytes");
    IcArgs q{};
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.cdw = cdw; q.flux = flux; q.alpha = alpha; q.w = out; q.limOut = limOut;
    q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    k_interface_compression<FLUX><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
template <bool FLUX>
int ic_patch(const char* who, mi_patch_s* p, const double* cdw, const double* flux, const double* alpha, const double* nbr, double* out, double* limOut)
{
    if (!p) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    if (p->nFaces == 0) return MI_OK;
    const double* in[4] = {cdw, flux, alpha, nbr};
    MICHK(lim_outputs(who, in, 4, out, limOut));
    const void* al[6] = {cdw, flux, alpha, nbr, out, limOut};
    MICHK(arrays_aligned8(who, al, 6));
    HIPCHK(hipSetDevice(p->ctx->device));
    IcArgs q{};
    q.lo = p->faceCells.p; q.cdw = cdw; q.flux = flux; q.alpha = alpha; q.nbr = nbr; q.w = out; q.limOut = limOut; q.nf = p->nFaces;
    k_patch_interface_compression<FLUX><<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace

// PhiScheme registers the bare word: `Gauss interfaceCompression` takes no coefficient
extern "C" int mi_interface_compression_parse(const char* scheme)
{
    if (!scheme) return fail(MI_ERR_ARG, "mi_interface_compression_parse: bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, "mi_interface_compression_parse: empty scheme");
    if (tok[0] != "interfaceCompression") return fail(MI_ERR_ARG, "mi_interface_compression_parse: '" + tok[0] + "' is not interfaceCompression");
    if (tok.size() > 1) return fail(MI_ERR_ARG, "mi_interface_compression_parse: interfaceCompression takes no coefficient: extra '" + tok[1] + "'");
    return MI_OK;
}

extern "C" int mi_interface_compression_weights(mi_addr_t a, const double* cd_weights_dev, const double* face_flux_dev, const double* alpha_dev,
                                                double* weights_out_dev, double* limiter_out_dev_or_null)
{
    return ic_internal<false>("mi_interface_compression_weights", a, cd_weights_dev, face_flux_dev, alpha_dev, weights_out_dev, limiter_out_dev_or_null);
}

extern "C" int mi_patch_interface_compression_weights(mi_patch_t p, const double* patch_cd_weights_dev, const double* patch_flux_dev,
                                                      const double* alpha_dev, const double* nbr_alpha_dev, double* weights_out_dev,
                                                      double* limiter_out_dev_or_null)
{
    return ic_patch<false>("mi_patch_interface_compression_weights", p, patch_cd_weights_dev, patch_flux_dev, alpha_dev, nbr_alpha_dev, weights_out_dev,
                           limiter_out_dev_or_null);
}

extern "C" int mi_alpha_compression_flux(mi_addr_t a, const double* cd_weights_dev, const double* phir_dev, const double* alpha1_dev, double* out_dev)
{
    return ic_internal<true>("mi_alpha_compression_flux", a, cd_weights_dev, phir_dev, alpha1_dev, out_dev, nullptr);
}

extern "C" int mi_patch_alpha_compression_flux(mi_patch_t p, const double* patch_cd_weights_dev, const double* patch_phir_dev, const double* alpha1_dev,
                                               const double* nbr_alpha1_dev, double* out_dev)
{
    return ic_patch<true>("mi_patch_alpha_compression_flux", p, patch_cd_weights_dev, patch_phir_dev, alpha1_dev, nbr_alpha1_dev, out_dev, nullptr);
}
