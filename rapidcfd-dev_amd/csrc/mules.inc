// mules.inc -- explicit MULES: limiter, limit and explicitSolve (included by engine.hip after reconstruct.inc; DESIGN 3.5l).
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

// what every row pass of this file walks: the caller-order row tables, the block mapping and the per-cell boundary lists
struct MuRow {
    const int32_t *os, *ls, *losort, *blockStart, *lo, *up;
    const int32_t *bStart, *bFace;
    int n, cap, xcd;
};
// the cell fields of mi_mules_fields and the handle's work arrays
struct MuCells {
    const double *rdtField, *rho, *rhoOld, *sp, *su, *vol, *psi, *psiOld, *bpsi;
    double rdt, psiMax, psiMin;
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
struct MuArgs { MuRow r; MuCells q; MuFlux x; };      // one kernel argument, as row_launch passes it

// k_gauss_grad's / k_reconstruct's skeleton for NA staged face arrays: the block's own faces of src[0..NA) through LDS, the first four
// neighbour-side faces in registers before the one barrier, then per live cell own(f, v) for its own faces ascending, nei(f, v) for its
// neighbour-side faces in losort order, bnd(bf) for its boundary faces, done(); init(c) comes first
template <int BS, int NA, class Init, class Own, class Nei, class Bnd, class Done>
__device__ __forceinline__ void mu_rows(const MuRow& r, const double* const (&src)[NA], Init init, Own own, Nei nei, Bnd bnd, Done done)
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
    const MuRow& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
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
    const MuRow& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
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
// in XCD-aware chunks as k_limited_weights, then the boundary faces grid-stride in the same launch
__global__ __launch_bounds__(256) void k_mules_lambda(const MuArgs a)
{
    const MuRow& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
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
        if (kind != MU_COUPLED && !((x.bphiBD[i] + corr) > MU_SMALL * MU_SMALL)) continue;   // limit outlet faces only
        const int c = q.bCell[i];
        x.blambda[i] = mu_min(x.blambda[i], corr > 0.0 ? q.lambdap[c] : q.lambdam[c]);
    }
}

// phiBD + lambda*phiCorr, or lambda*phiCorr with returnCorr: internal and boundary faces in one launch
__global__ __launch_bounds__(256) void k_mules_apply(const MuFlux x)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t f = t0; f < x.nf; f += step) { const double p = x.lambda[f] * x.phiCorr[f]; x.out[f] = x.returnCorr ? p : x.phiBD[f] + p; }
    for (int64_t i = t0; i < x.nb; i += step) { const double p = x.blambda[i] * x.bphiCorr[i]; x.bout[i] = x.returnCorr ? p : x.bphiBD[i] + p; }
}

// explicitSolve: surfaceIntegrate(x.phiPsi) and the final expression; x.out is the new psi, a cell array
template <int BS, bool LTS>
__global__ __launch_bounds__(BS) void k_mules_solve(const MuArgs a)
{
    const MuRow& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
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
struct mi_mules_s {
    mi_ctx_s* ctx = nullptr;
    mi_addr_s* addr = nullptr;
    mi_grad_boundary_s* boundary = nullptr;
    int32_t nCells = 0, nFaces = 0, nBFaces = 0;
    bool coupled = false, begun = false;
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
int mu_check(const std::string& who, mi_mules_s* h, const mi_mules_fields* fl, const double* const* in, const int* inKind, int nIn,
             double* const* out, const int* outKind, int nOut, MuCall& c)
{
    mi_addr_s* a = h->addr;
    if (h->nCells != a->L.nCells || h->nFaces != a->L.nFaces || (h->boundary && h->boundary->addr != a))
        return fail(MI_ERR_ARG, who + ": the handle was built for another addressing");
    if (!fl) return fail(MI_ERR_ARG, who + ": the fields are missing");
    if (!fl->vol_dev || !fl->psi_dev || !fl->psi_old_dev) return fail(MI_ERR_ARG, who + ": a cell array is missing");
    if ((fl->rho_dev != nullptr) != (fl->rho_old_dev != nullptr)) return fail(MI_ERR_ARG, who + ": rho and rho_old come together or not at all");
    const bool hasF = h->nFaces > 0, hasB = h->nBFaces > 0;
    auto present = [&](int kind) { return kind == MU_CELL || (kind == MU_FACE ? hasF : hasB); };   // an empty array may be NULL and is never read
    if (hasB && !fl->b_psi_dev) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary psi needed");
    const double* all[40];
    int m = 0;
    const double* cells[9] = {fl->r_delta_t_dev, fl->rho_dev, fl->rho_old_dev, fl->sp_dev, fl->su_dev, fl->vol_dev, fl->psi_dev, fl->psi_old_dev,
                              hasB ? fl->b_psi_dev : nullptr};
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
    MICHK(rc_aligned(who, (const void* const*)all, m));
    MICHK(rc_aligned(who, (const void* const*)outs, mo));
    MICHK(ls_outputs(who, all, m, outs, mo));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    MuRow& r = c.a.r;
    r.os = a->ownerStartC.p; r.ls = a->losortStartC.p; r.losort = a->losortC.p; r.lo = a->lowerAddr.p; r.up = a->upperAddr.p;
    r.blockStart = a->rowPlan[1].tiles ? a->tileCellStart.p : nullptr;
    if (hasB) { r.bStart = h->boundary->allStart.p; r.bFace = h->boundary->all.p; }
    r.n = a->L.nCells; r.xcd = a->ctx->xcdRows;
    MuCells& q = c.a.q;
    q.rdtField = fl->r_delta_t_dev; q.rdt = fl->r_delta_t; q.rho = fl->rho_dev; q.rhoOld = fl->rho_old_dev; q.sp = fl->sp_dev; q.su = fl->su_dev;
    q.vol = fl->vol_dev; q.psi = fl->psi_dev; q.psiOld = fl->psi_old_dev; q.bpsi = fl->b_psi_dev; q.psiMax = fl->psi_max; q.psiMin = fl->psi_min;
    q.maxn = h->work[0].p; q.minn = h->work[1].p; q.sumPhip = h->work[2].p; q.mSumPhim = h->work[3].p; q.lambdap = h->work[4].p; q.lambdam = h->work[5].p;
    q.bKind = h->bKind.p; q.bCell = h->bCell.p;
    c.lts = fl->r_delta_t_dev != nullptr;
    c.a.x.nf = h->nFaces; c.a.x.nb = h->nBFaces; c.a.x.xcd = a->ctx->xcdRows;
    return MI_OK;
}
const int kMuFB[8] = {MU_FACE, MU_BFACE, MU_FACE, MU_BFACE, MU_FACE, MU_BFACE, MU_FACE, MU_BFACE};

// a row pass of `arrays` staged face arrays on the gradient's plan
template <class K>
int mu_row_launch(mi_addr_s* a, int arrays, K k256, K k512, K k1024, MuArgs& q)
{
    const mi_addr_s::RowPlan& rp = a->rowPlan[1];
    q.r.cap = row_cap(rp, arrays);
    return row_launch(a, rp, rp.bs == 256 ? k256 : rp.bs == 512 ? k512 : k1024, q, (size_t)arrays * q.r.cap * sizeof(double));
}
#define MU_BS(K, ...) K<256, __VA_ARGS__>, K<512, __VA_ARGS__>, K<1024, __VA_ARGS__>

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
    if (h->nCells == 0) { h->begun = true; return MI_OK; }
    mi_addr_s* a = h->addr;
    int r;
    if (form == MI_MULES_LIMIT) r = c.lts ? mu_row_launch(a, 2, MU_BS(k_mules_bounds, true, true), c.a) : mu_row_launch(a, 2, MU_BS(k_mules_bounds, true, false), c.a);
    else r = c.lts ? mu_row_launch(a, 2, MU_BS(k_mules_bounds, false, true), c.a) : mu_row_launch(a, 2, MU_BS(k_mules_bounds, false, false), c.a);
    if (r == MI_OK) h->begun = true;
    return r;
}
int mu_check_iterate(const std::string& who, mi_mules_s* h, int n, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c, bool begunByCaller)
{
    if (n < 0) return fail(MI_ERR_ARG, who + ": n must not be negative");
    if (!begunByCaller && !h->begun) return fail(MI_ERR_ARG, who + ": called before mi_mules_begin");
    if (n > 1 && h->coupled)
        return fail(MI_ERR_ARG, who + ": the boundary has coupled patches: the minOp sync between iterations is the caller's, iterate one at a time");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    const double* in[4] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev};
    double* out[2] = {fx->lambda_dev, fx->b_lambda_dev};
    return mu_check(who, h, fl, in, kMuFB, 4, out, kMuFB, 2, c);
}
int mu_launch_iterate(mi_mules_s* h, int n, MuCall& c)
{
    if (h->nCells == 0) return MI_OK;
    mi_addr_s* a = h->addr;
    const int64_t faces = std::max<int64_t>(h->nFaces, h->nBFaces);
    for (int j = 0; j < n; ++j) {
        MICHK(mu_row_launch(a, 2, k_mules_sums<256>, k_mules_sums<512>, k_mules_sums<1024>, c.a));
        if (faces > 0) {
            k_mules_lambda<<<grid_for(a->ctx, (int)faces), 256, 0, a->ctx->stream>>>(c.a);
            HIPCHK(hipGetLastError());
        }
    }
    return MI_OK;
}
int mu_check_apply(const std::string& who, mi_mules_s* h, const mi_mules_fields* fl, const mi_mules_flux* fx, MuCall& c, bool begunByCaller)
{
    if (!begunByCaller && !h->begun) return fail(MI_ERR_ARG, who + ": called before mi_mules_begin");
    if (!fx) return fail(MI_ERR_ARG, who + ": the flux arrays are missing");
    const double* in[6] = {fx->phi_bd_dev, fx->b_phi_bd_dev, fx->phi_corr_dev, fx->b_phi_corr_dev, fx->lambda_dev, fx->b_lambda_dev};
    double* out[2] = {fx->out_dev, fx->b_out_dev};
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
    if (!a || !out) return fail(MI_ERR_ARG, who + ": bad argument");
    if (b && (b->addr != a || b->nCells != a->L.nCells)) return fail(MI_ERR_ARG, who + ": the boundary was built for another addressing");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    std::unique_ptr<mi_mules_s> h(new mi_mules_s());
    h->ctx = a->ctx; h->addr = a; h->boundary = b; h->nCells = a->L.nCells; h->nFaces = a->L.nFaces; h->nBFaces = b ? b->nFaces : 0;
    if (h->nCells == 0) { *out = h.release(); return MI_OK; }
    for (int i = 0; i < 6; ++i) MICHK(h->work[i].alloc((size_t)h->nCells));
    if (h->nBFaces > 0) {
        Table<uint8_t> kind((size_t)h->nBFaces);
        size_t off = 0;
        for (size_t p = 0; p < b->patchSizes.size(); ++p) {
            const bool wedge = patch_is_wedge_host_or_null && patch_is_wedge_host_or_null[p] != 0;
            const bool cpl = b->patchKinds[p] == MI_GRAD_PATCH_COUPLED;
            if (cpl && !wedge && b->patchSizes[p] > 0) h->coupled = true;
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
    MICHK(ls_outputs(who, in, 6, out_dev, 6));
    MICHK(rc_aligned(who, (const void* const*)out_dev, 6));
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
    MICHK(mu_check_iterate(who, h, n, fields, flux, c, false));
    mu_flux(flux, c.a.x);
    return mu_launch_iterate(h, n, c);
}

extern "C" int mi_mules_apply(mi_mules_t h, int32_t return_corr, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_apply";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MuCall c;
    MICHK(mu_check_apply(who, h, fields, flux, c, false));
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
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x);
    MICHK(mu_launch_begin(h, MI_MULES_LIMITER, c));
    return mu_launch_iterate(h, n_limiter_iter, ci);
}

extern "C" int mi_mules_limit(mi_mules_t h, int32_t n_limiter_iter, int32_t return_corr, const mi_mules_fields* fields, const mi_mules_flux* flux)
{
    const std::string who = "mi_mules_limit";
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(mu_no_couples(who, h));
    MuCall c, ci, ca;
    MICHK(mu_begin(who, h, MI_MULES_LIMIT, fields, flux, c));
    MICHK(mu_check_iterate(who, h, n_limiter_iter, fields, flux, ci, true));
    MICHK(mu_check_apply(who, h, fields, flux, ca, true));
    mu_flux(flux, c.a.x); mu_flux(flux, ci.a.x); mu_flux(flux, ca.a.x);
    MICHK(mu_launch_begin(h, MI_MULES_LIMIT, c));
    MICHK(mu_launch_iterate(h, n_limiter_iter, ci));
    return mu_launch_apply(h, return_corr, ca);
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
    return c.lts ? mu_row_launch(a, 1, MU_BS(k_mules_solve, true), c.a) : mu_row_launch(a, 1, MU_BS(k_mules_solve, false), c.a);
}

extern "C" int mi_vec_min(mi_ctx_t c, int64_t n, const double* x_dev, const double* y_dev, double* out_dev)
{
    if (!c || n < 0 || (n > 0 && (!x_dev || !y_dev || !out_dev))) return fail(MI_ERR_ARG, "mi_vec_min: bad argument");
    if (!al8(x_dev) || !al8(y_dev) || !al8(out_dev)) return fail(MI_ERR_ARG, "mi_vec_min: arrays must be aligned to 8 bytes");
    if (n == 0) return MI_OK;
    return cell_launch(c, k_vmin, x_dev, y_dev, out_dev, n);
}
