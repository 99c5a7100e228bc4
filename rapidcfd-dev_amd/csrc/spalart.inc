// spalart.inc -- incompressible::RASModels::SpalartAllmaras and the LES classes SpalartAllmaras (DES), SpalartAllmarasDDES and SpalartAllmarasIDDES
// with the nutUSpaldingWallFunction patch (turbulenceModels/incompressible/RAS/SpalartAllmaras/SpalartAllmaras.C:45-137, :269-275, :437-464;
// LES/SpalartAllmaras/SpalartAllmaras.C:45-172, :331-357; LES/SpalartAllmarasDDES/SpalartAllmarasDDES.C:45-93;
// LES/SpalartAllmarasIDDES/SpalartAllmarasIDDES.C:45-140; nutUSpaldingWallFunctionFvPatchScalarField.C:39-110; included by engine.hip after
// les.inc; DESIGN 3.5t).
//
//   terms      everything of correct() between the gradients and the assembly in ONE cell pass: chi, fv1, fv2, fv3, S, dTilda (min / the
//              delayed form / the IDDES blend), STilda, r, g, fw and the four fields the equation takes; kind and the Ashford switch are
//              template parameters, so no instantiation carries a transcendental it does not evaluate
//   nut        fv1*nuTilda with the fv1 of before the solve (RAS :463) or recomputed (updateSubGridScaleFields, LES :45-49)
//   wall       nutUSpaldingWallFunction::calcNut with calcUTau's Newton loop on every wall face in one launch on the mi_ke_t handle
// max is (a > b) ? a : b, min is (a < b) ? a : b, pos(x) is x >= 0, neg(x) is x < 0, pow3(s) = s*sqr(s), pow6(s) = pow3(sqr(s)).  Every field
// operator of the reference is rounded on its own (-ffp-contract=off); every fma below is written: magSqr of a vector (3.5s), magSqr of a
// symmetric tensor (3.5o), magSqr of a full tensor, the Newton step of the wall functor.  pow, tanh and exp are the device library's: each
// is evaluated once per cell (per iteration) and can be returned.  Restated in tests/spalart_support.py.
namespace mi {

constexpr double SA_SMALL = 1.0e-15, SA_ROOTVSMALL = 1.0e-150;   // doubleScalar.H:55-57

struct SaCell {
    const double* in[18];
    double* out[16];
    uint32_t n;                                       // the entries refuse more than INT32_MAX cells
    int vec;
    uint32_t want;                                    // bit k: output k is written (an optional output that is not wanted is NULL)
    double nu;
    mi_sa_coeffs K;
};
// the argument block in the kernel's argument segment, as sst_args: the IDDES pass has 34 array bases, which do not fit in scalar registers
// across the loop; they are read where the loads and where the stores need them
typedef const SaCell __attribute__((address_space(4)))* SaArgs;
typedef const mi_sa_coeffs __attribute__((address_space(4)))& SaCoeffs;
__device__ __forceinline__ SaArgs sa_args()
{
    SaArgs p = (SaArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// sst_map on an SaCell: a grid-stride walk, two cells per thread with 16-byte accesses when every array allows it (a.vec), one by one
// otherwise; outputs from NREQ on are written only when wanted (the mask is read with the bases).  32-bit counters: 2*q < n <= INT32_MAX.
// What differs from sst_map serves one end, no scalar register spilled beside the 50 to 60 that the library's pow / exp / tanh constants take:
// every thread walks the same number of rounds over the pairs, a thread past the last pair repeating it (the same loads, the same bits
// stored again; no output is an input), so that no saved exec mask is live across the arithmetic; the loop bounds sit in vector registers;
// the two cells of a thread are scheduled one after the other.
template <int NIN, int NOUT, int NREQ, class F>
__device__ __forceinline__ void sa_map(const SaCell& a, F f)
{
    const uint32_t n = a.n, np = a.vec ? n >> 1 : 0, t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    uint32_t last = np - 1, end = n, step = stride;   // np == 0: no round, last is not used
    asm volatile("" : "+v"(last), "+v"(end), "+v"(step));
    uint32_t q = t;
    for (uint32_t left = (np + stride - 1) / stride; left; --left, q += step) {
        const uint32_t i = 2 * (q < last ? q : last);
        double x[NIN], y[NIN], ox[NOUT], oy[NOUT];
        SaArgs p = sa_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) { const double2 v = ld2(p->in[k], i); x[k] = v.x; y[k] = v.y; }
        f(x, ox);
        __builtin_amdgcn_sched_barrier(0);
        f(y, oy);
        p = sa_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (p->want >> k & 1u)) st2(p->out[k], i, make_double2(ox[k], oy[k]));
    }
    for (uint32_t i = 2 * np + t; i < end; i += step) {
        double x[NIN], o[NOUT];
        SaArgs p = sa_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) x[k] = p->in[k][i];
        f(x, o);
        p = sa_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (p->want >> k & 1u)) p->out[k][i] = o[k];
    }
}

__device__ __forceinline__ double sa_pow3(double s) { return s * (s * s); }             // Scalar.H:183-186
__device__ __forceinline__ double sa_pow6(double s) { return sa_pow3(s * s); }          // Scalar.H:201-204
// mag(skew(gradU)) (TensorI.H:511-519, VectorSpaceI.H:336-355): magSqr of the nine components is fma(xx, xx, xy*xy) and then one fma per
// component; skew's diagonal is 0.0, so the first fma returns xy*xy and two others return their addend: six components remain
__device__ __forceinline__ double sa_mag_skew(const double* g)    // g[3*j + k] = d(U_j)/dx_k
{
    const double xy = 0.5 * (g[1] - g[3]), xz = 0.5 * (g[2] - g[6]), yx = 0.5 * (g[3] - g[1]);
    const double yz = 0.5 * (g[5] - g[7]), zx = 0.5 * (g[6] - g[2]), zy = 0.5 * (g[7] - g[5]);
    double s = xy * xy;
    s = fma(xz, xz, s);
    s = fma(yx, yx, s);
    s = fma(yz, yz, s);
    s = fma(zx, zx, s);
    s = fma(zy, zy, s);
    return sqrt(s);
}
// r of the LES classes and rd of DDES / IDDES: min(visc/(max(S, SMALL)*sqr(kappa*d) + ROOTVSMALL), 10)
__device__ __forceinline__ double sa_rd(double visc, double S, double kd2)
{
    return sst_min(visc / (mu_max(S, SA_SMALL) * kd2 + SA_ROOTVSMALL), 10.0);
}

enum { SA_RAS = 0, SA_DES = 1, SA_DDES = 2, SA_IDDES = 3 };
// outputs: su_grad, su_prod, sp, dnu, fv1 | S, dTilda, STilda, pow of fw | tanh of fd | exp, pow(., -11.09), pow(., -9.0), tanh of ft,
// pow(., 10), tanh of fl
__host__ __device__ constexpr int sa_nout(int kind) { return kind == SA_IDDES ? 16 : (kind == SA_DDES ? 10 : 9); }
__host__ __device__ constexpr int sa_nin(int kind, bool nuf) { return 14 + (nuf ? 1 : 0) + (kind >= SA_DES ? 1 : 0) + (kind >= SA_DDES ? 1 : 0) + (kind == SA_IDDES ? 1 : 0); }

// in: nuTilda, gradU[9], grad(nuTilda)[3], y, [nu], [delta], [nuSgs], [hmax]
template <int KIND, bool ASH, bool NUF>
__global__ __launch_bounds__(256) void k_sa_terms(const SaCell a)
{
    constexpr int NIN = sa_nin(KIND, NUF), NOUT = sa_nout(KIND);
    constexpr int I_DELTA = 14 + (NUF ? 1 : 0), I_NUSGS = I_DELTA + 1, I_HMAX = I_DELTA + 2;
    // the coefficients do not fit in scalar registers beside the library's constants either: each of the three parts of the cell's arithmetic
    // reads the ones it uses from the argument segment (scalar loads) behind a scheduling barrier, so none is live across another part
    sa_map<NIN, NOUT, 5>(a, [](const double (&x)[NIN], double (&o)[NOUT]) {
        const SaArgs p = sa_args();
        SaCoeffs K = p->K;
        const double nt = x[0], y = x[13];
        double nu;
        if constexpr (NUF) nu = x[14]; else nu = p->nu;
        const double* g = x + 1;
        const double chi = nt / nu;
        const double chi3 = sa_pow3(chi);
        const double fv1 = chi3 / (chi3 + K.Cv1_3);
        // S: the base classes' skew form; SpalartAllmarasDDES::S overrides it with symm (DDES.C:78-81), IDDES does not
        const double magG = (KIND == SA_DDES) ? sqrt(ke_magsqr_symm(g)) : sa_mag_skew(g);
        const double S = K.sqrt2 * magG;
        // fv2 and fv3: the RAS class works on a stored chi, the LES classes on nuTilda and nu
        double fv2, fv3 = 1.0;
        if (ASH) {
            const double t = (KIND == SA_RAS) ? 1.0 + chi / K.Cv2 : 1.0 + nt / (K.Cv2 * nu);
            fv2 = 1.0 / sa_pow3(t);
            const double c = (KIND == SA_RAS) ? K.invCv2 * chi : chi / K.Cv2, t3 = 1.0 + c;
            fv3 = (((1.0 + chi * fv1) * K.invCv2) * (3.0 * t3 + c * c)) / sa_pow3(t3);
        } else {
            fv2 = 1.0 - chi / (1.0 + chi * fv1);
        }
        const double ky = K.kappa * y, ky2 = ky * ky;
        // dTilda
        double dT = y;
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] SaCoeffs Kd = sa_args()->K;
        if constexpr (KIND == SA_DES) {
            dT = sst_min(Kd.CDES * x[I_DELTA], y);
        } else if constexpr (KIND == SA_DDES) {
            const double th = tanh(sa_pow3(8.0 * sa_rd(x[I_NUSGS] + nu, S, ky2))), fd = 1.0 - th;
            dT = mu_max(y - fd * mu_max(y - Kd.CDES * x[I_DELTA], 0.0), SA_SMALL);
            o[9] = th;
        } else if constexpr (KIND == SA_IDDES) {
            const double nuSgs = x[I_NUSGS];
            const double alpha = mu_max(0.25 - y / x[I_HMAX], -5.0);
            const double e = exp(alpha * alpha), p1 = pow(e, -11.09), p2 = pow(e, -9.0);
            const double fHill = 2.0 * (((alpha >= 0) ? 1.0 : 0.0) * p1 + ((alpha < 0) ? 1.0 : 0.0) * p2);
            const double fStep = sst_min(2.0 * p2, 1.0);
            const double th = tanh(sa_pow3(8.0 * sa_rd(nuSgs + nu, S, ky2))), fd = 1.0 - th;
            const double fHyb = mu_max(1.0 - fd, fStep);
            const double ft = tanh(sa_pow3(Kd.ct2 * sa_rd(nuSgs, S, ky2)));
            const double p10 = pow(Kd.cl2 * sa_rd(nu, S, ky2), 10.0), fl = tanh(p10);
            const double fAmp = 1.0 - mu_max(ft, fl);
            const double fRestore = mu_max(fHill - 1.0, 0.0) * fAmp;
            const double Psi = sqrt(sst_min(100.0, (1.0 - Kd.psiCoeff * fv2) / mu_max(SA_SMALL, fv1)));
            dT = mu_max(SA_SMALL, (fHyb * (1.0 + fRestore * Psi)) * y + (((1.0 - fHyb) * Kd.CDES) * Psi) * x[I_DELTA]);
            o[9] = th; o[10] = e; o[11] = p1; o[12] = p2; o[13] = ft; o[14] = p10; o[15] = fl;
        }
        __builtin_amdgcn_sched_barrier(0);
        SaCoeffs Ke = sa_args()->K;
        const double kd = Ke.kappa * dT, kd2 = kd * kd;
        // STilda: the RAS class multiplies fv3 by sqrt(2.0) before mag(skew(gradU)) (:442), the LES classes by the stored S (:123)
        const double ST = ((KIND == SA_RAS) ? (fv3 * Ke.sqrt2) * magG : fv3 * S) + (fv2 * nt) / kd2;
        // fw: the RAS r has no ROOTVSMALL (:116-131)
        const double r = (KIND == SA_RAS) ? sst_min(nt / (mu_max(ST, SA_SMALL) * kd2), 10.0) : sa_rd(nt, ST, kd2);
        const double gg = r + Ke.Cw2 * (sa_pow6(r) - r);
        const double pw = pow(Ke.onePlusCw3_6 / (sa_pow6(gg) + Ke.Cw3_6), 1.0 / 6.0);
        const double fw = gg * pw;
        o[0] = Ke.Cb2BySigmaNut * les_magsqr_v(x + 10);
        o[1] = (Ke.Cb1 * ST) * nt;
        o[2] = ((Ke.Cw1 * fw) * nt) / (dT * dT);
        o[3] = (nt + nu) / Ke.sigmaNut;
        o[4] = fv1;
        o[5] = S; o[6] = dT; o[7] = ST; o[8] = pw;
    });
}
// in: nuTilda, then fv1 (the stored one) or [nu] (recomputed); out: nut, optional fv1
template <bool RECOMPUTE, bool NUF>
__global__ __launch_bounds__(256) void k_sa_nut(const SaCell a)
{
    constexpr int NIN = (RECOMPUTE && !NUF) ? 1 : 2;
    const double Cv1_3 = a.K.Cv1_3, nu0 = a.nu;
    sa_map<NIN, 2, 1>(a, [=](const double (&x)[NIN], double (&o)[2]) {
        double fv1 = x[NIN - 1];
        if (RECOMPUTE) {
            const double chi3 = sa_pow3(x[0] / (NUF ? x[NIN - 1] : nu0));
            fv1 = chi3 / (chi3 + Cv1_3);
        }
        o[0] = fv1 * x[0]; o[1] = fv1;
    });
}

struct SaWallArgs {
    const int32_t *faces, *faceCell;
    const double *u[3], *buw[3], *bdc, *by, *bnuw;
    double *bnut, *bexp;
    int32_t* biter;
    double kappa, invE;
    int nFaces;
};
// calcNut (:93-110) with calcUTau's functor (:39-89): one thread per wall face.  The functor is one expression per line; its contraction is
// the one read from the compiled functor (an ASSUMPTION, DESIGN 3.5t): fkUu = fma(-kUu, fma(kUu, 0.5, 1.0), exp(kUu) - 1),
// f = fma(1/E, fma(-(1.0/6.0)*kUu, sqr(kUu), fkUu), magUp/ut - (ut*y)/nuw), df = (magUp/sqr(ut) + y/nuw) + (((1/E)*kUu)*fkUu)/ut
__global__ __launch_bounds__(256) void k_sa_nut_spalding_wall(const SaWallArgs a)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < a.nFaces; j += gridDim.x * blockDim.x) {
        const int bf = a.faces[j], c = a.faceCell[j];
        const double dc = a.bdc[bf], y = a.by[bf], nuw = a.bnuw[bf], nutw = a.bnut[bf];
        double d[3], sn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double uc = a.u[k][c], uw = a.buw[k][bf]; d[k] = uc - uw; sn[k] = dc * (uw - uc); }
        const double magUp = if_mag(d), magGradU = if_mag(sn);
        double ut = sqrt((nutw + nuw) * magGradU), uTau = 0.0;
        int taken = 0;
        if (ut > SA_ROOTVSMALL) {
            const double kM = a.kappa * magUp, yn = y / nuw;
            double err;
            do {
                const double kUu = sst_min(kM / ut, 50.0);
                const double e = exp(kUu);
                if (a.bexp) a.bexp[10 * (int64_t)bf + taken] = e;
                ++taken;
                const double fkUu = fma(-kUu, fma(kUu, 0.5, 1.0), e - 1.0);
                const double f = fma(a.invE, fma(-(1.0 / 6.0) * kUu, kUu * kUu, fkUu), magUp / ut - (ut * y) / nuw);
                const double df = (magUp / (ut * ut) + yn) + ((a.invE * kUu) * fkUu) / ut;
                const double uTauNew = ut + f / df;
                err = fabs((ut - uTauNew) / ut);
                ut = uTauNew;
            } while (ut > SA_ROOTVSMALL && err > 0.01 && taken < 10);   // ++iter < 10: at most ten steps
            uTau = mu_max(0.0, ut);
        }
        if (a.biter) a.biter[bf] = taken;
        a.bnut[bf] = mu_max(0.0, (uTau * uTau) / (magGradU + SA_ROOTVSMALL) - nuw);
    }
}

} // namespace mi

namespace {
int sa_coeffs_check(const std::string& who, const mi_sa_coeffs* k)
{
    if (!k) return fail(MI_ERR_ARG, who + ": the coefficients are missing");
    const double v[27] = {k->sigmaNut, k->kappa, k->Cb1, k->Cb2, k->Cw2, k->Cw3, k->Cv1, k->Cv2, k->CDES, k->ck, k->fwStar, k->cl, k->ct, k->wallKappa, k->E,
                          k->Cw1, k->Cb2BySigmaNut, k->Cv1_3, k->Cw3_6, k->onePlusCw3_6, k->invCv2, k->ct2, k->cl2, k->psiDen, k->psiCoeff, k->invE, k->sqrt2};
    for (double x : v) if (!ke_positive(x)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_sa_coeffs_init)");
    return MI_OK;
}
// les_cell_pass on an SaCell; outputs from nReq on are optional (NULL: not written)
template <class K>
int sa_cell_pass(const std::string& who, mi_ctx_s* c, int64_t n, K kernel, mi::SaCell& q, const double* const* in, int nIn, double* const* out, int nOut,
                 int nReq)
{
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n > INT32_MAX) return fail(MI_ERR_ARG, who + ": too many cells");
    if (n == 0) return MI_OK;
    MICHK(arrays_present(who, in, nIn));
    double* given[16];
    int nGiven = 0;
    q.want = 0;
    for (int i = 0; i < nOut; ++i) if (i < nReq || out[i]) { given[nGiven++] = out[i]; q.want |= 1u << i; }
    MICHK(outputs_distinct(who, in, nIn, given, nGiven));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)given, nGiven));
    for (int i = 0; i < nIn; ++i) q.in[i] = in[i];
    for (int i = 0; i < nOut; ++i) q.out[i] = out[i];
    q.n = (uint32_t)n; q.vec = all_aligned16(in, nIn, given, nGiven) ? 1 : 0;
    HIPCHK(hipSetDevice(c->device));
    kernel<<<grid_for(c, (int)((n + 1) / 2)), 256, 0, c->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
typedef void (*sa_kernel_t)(const mi::SaCell);
template <int KIND>
sa_kernel_t sa_terms_kernel(bool ash, bool nuf)
{
    if (ash) return nuf ? mi::k_sa_terms<KIND, true, true> : mi::k_sa_terms<KIND, true, false>;
    return nuf ? mi::k_sa_terms<KIND, false, true> : mi::k_sa_terms<KIND, false, false>;
}
} // namespace

extern "C" int mi_sa_coeffs_init(const double* model_or_null, const double* wall_or_null, mi_sa_coeffs* out)
{
    const std::string who = "mi_sa_coeffs_init";
    if (!out) return fail(MI_ERR_ARG, who + ": bad argument");
    // RAS SpalartAllmaras.C:153-226; LES SpalartAllmaras.C:188-278 (CDES, ck); SpalartAllmarasIDDES.C:173-199 (fwStar, cl, ct)
    const double model0[13] = {0.66666, 0.41, 0.1355, 0.622, 0.3, 2.0, 7.1, 5.0, 0.65, 0.07, 0.424, 3.55, 1.63};
    const double wall0[2] = {0.41, 9.8};              // nutWallFunctionFvPatchScalarField.C: kappa, E
    const double* m = model_or_null ? model_or_null : model0;
    const double* w = wall_or_null ? wall_or_null : wall0;
    for (int i = 0; i < 13; ++i) if (!ke_positive(m[i])) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    for (int i = 0; i < 2; ++i) if (!ke_positive(w[i])) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    mi_sa_coeffs k{};
    k.sigmaNut = m[0]; k.kappa = m[1]; k.Cb1 = m[2]; k.Cb2 = m[3]; k.Cw2 = m[4]; k.Cw3 = m[5]; k.Cv1 = m[6]; k.Cv2 = m[7]; k.CDES = m[8]; k.ck = m[9];
    k.fwStar = m[10]; k.cl = m[11]; k.ct = m[12];
    k.wallKappa = w[0]; k.E = w[1];
    // the products of dimensionedScalars, formed once in the reference's order
    const double kappa2 = k.kappa * k.kappa;
    k.Cw1 = k.Cb1 / kappa2 + (1.0 + k.Cb2) / k.sigmaNut;          // RAS :190, LES :260
    k.Cb2BySigmaNut = k.Cb2 / k.sigmaNut;                         // RAS :451, LES :345
    k.Cv1_3 = k.Cv1 * (k.Cv1 * k.Cv1);                            // pow3(Cv1_), RAS :54, LES :57
    const double cw3_2 = k.Cw3 * k.Cw3;
    k.Cw3_6 = cw3_2 * (cw3_2 * cw3_2);                            // pow6(Cw3_), RAS :136, LES :165
    k.onePlusCw3_6 = 1.0 + k.Cw3_6;
    k.invCv2 = 1 / k.Cv2;                                         // RAS :83, :87; LES :84
    k.ct2 = k.ct * k.ct; k.cl2 = k.cl * k.cl;                     // IDDES :60, :69
    k.psiDen = (k.Cw1 * kappa2) * k.fwStar;                       // IDDES :129
    k.psiCoeff = k.Cb1 / k.psiDen;
    k.invE = 1 / k.E;                                             // nutUSpalding :69, :74
    k.sqrt2 = std::sqrt(2.0);                                     // ::sqrt(2.0), RAS :442, LES :113
    MICHK(sa_coeffs_check(who, &k));
    *out = k;
    return MI_OK;
}

extern "C" int mi_sa_terms(mi_ctx_t c, int64_t n, const mi_sa_coeffs* coeffs, int kind, int ashford, const mi_sa_cells* x)
{
    const std::string who = "mi_sa_terms";
    MICHK(sa_coeffs_check(who, coeffs));
    if (kind < MI_SA_RAS || kind > MI_SA_IDDES) return fail(MI_ERR_ARG, who + ": kind must be MI_SA_RAS, MI_SA_DES, MI_SA_DDES or MI_SA_IDDES");
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    if (!x->nu_dev_or_null && !ke_positive(x->nu_value)) return fail(MI_ERR_ARG, who + ": nu must be a finite number above zero");
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n > 0 && kind >= MI_SA_DES && !x->delta_dev) return fail(MI_ERR_ARG, who + ": the DES kinds need delta: input arrays missing");
    if (n > 0 && kind >= MI_SA_DDES && !x->nusgs_dev) return fail(MI_ERR_ARG, who + ": DDES and IDDES need nuSgs: input arrays missing");
    if (n > 0 && kind == MI_SA_IDDES && !x->hmax_dev) return fail(MI_ERR_ARG, who + ": IDDES needs hmax: input arrays missing");
    SaCell q{};
    q.K = *coeffs; q.nu = x->nu_value;
    const bool nuf = x->nu_dev_or_null != nullptr;
    const double* in[18] = {x->nutilda_dev};
    for (int i = 0; i < 9; ++i) in[1 + i] = x->grad_dev[i];
    for (int i = 0; i < 3; ++i) in[10 + i] = x->grad_nutilda_dev[i];
    in[13] = x->y_dev;
    int nIn = 14;
    if (nuf) in[nIn++] = x->nu_dev_or_null;
    if (kind >= MI_SA_DES) in[nIn++] = x->delta_dev;
    if (kind >= MI_SA_DDES) in[nIn++] = x->nusgs_dev;
    if (kind == MI_SA_IDDES) in[nIn++] = x->hmax_dev;
    double* out[16] = {x->su_grad_out_dev, x->su_prod_out_dev, x->sp_out_dev, x->dnu_out_dev, x->fv1_out_dev,
                       x->s_out_dev_or_null, x->dtilda_out_dev_or_null, x->stilda_out_dev_or_null, x->pow_fw_out_dev_or_null, x->tanh_fd_out_dev_or_null,
                       x->exp_out_dev_or_null, x->pow_hill_pos_out_dev_or_null, x->pow_hill_neg_out_dev_or_null, x->tanh_ft_out_dev_or_null,
                       x->pow_fl_out_dev_or_null, x->tanh_fl_out_dev_or_null};
    const int nOut = sa_nout(kind);
    for (int i = nOut; i < 16; ++i) if (out[i]) return fail(MI_ERR_ARG, who + ": an optional output was given that this kind does not form");
    sa_kernel_t kernel = kind == MI_SA_RAS ? sa_terms_kernel<SA_RAS>(ashford != 0, nuf) : kind == MI_SA_DES ? sa_terms_kernel<SA_DES>(ashford != 0, nuf)
                       : kind == MI_SA_DDES ? sa_terms_kernel<SA_DDES>(ashford != 0, nuf) : sa_terms_kernel<SA_IDDES>(ashford != 0, nuf);
    return sa_cell_pass(who, c, n, kernel, q, in, nIn, out, nOut, 5);
}

extern "C" int mi_sa_nut(mi_ctx_t c, int64_t n, const mi_sa_coeffs* coeffs, int recompute_fv1, const double* nutilda_dev, const double* fv1_dev_or_null,
                         const double* nu_dev_or_null, double nu_value, double* nut_out_dev, double* fv1_out_dev_or_null)
{
    const std::string who = "mi_sa_nut";
    MICHK(sa_coeffs_check(who, coeffs));
    SaCell q{};
    q.K = *coeffs; q.nu = nu_value;
    double* out[2] = {nut_out_dev, fv1_out_dev_or_null};
    if (!recompute_fv1) {
        if (fv1_out_dev_or_null) return fail(MI_ERR_ARG, who + ": fv1 is an input of the stored form, not an output");
        const double* in[2] = {nutilda_dev, fv1_dev_or_null};
        return sa_cell_pass(who, c, n, k_sa_nut<false, true>, q, in, 2, out, 2, 1);
    }
    if (!nu_dev_or_null && !ke_positive(nu_value)) return fail(MI_ERR_ARG, who + ": nu must be a finite number above zero");
    const double* in[2] = {nutilda_dev, nu_dev_or_null};
    if (nu_dev_or_null) return sa_cell_pass(who, c, n, k_sa_nut<true, true>, q, in, 2, out, 2, 1);
    return sa_cell_pass(who, c, n, k_sa_nut<true, false>, q, in, 1, out, 2, 1);
}

extern "C" int mi_sa_nut_spalding_wall(mi_ke_t h, const mi_sa_coeffs* coeffs, const mi_sa_wall* x)
{
    const std::string who = "mi_sa_nut_spalding_wall";
    MICHK(row_handle_check(who, h));
    MICHK(sa_coeffs_check(who, coeffs));
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    if (h->nWallFaces == 0) return MI_OK;
    const double* in[10] = {x->u_dev[0], x->u_dev[1], x->u_dev[2], x->b_uw_dev[0], x->b_uw_dev[1], x->b_uw_dev[2], x->b_delta_coeffs_dev, x->b_y_dev, x->b_nuw_dev};
    double* out[2] = {x->b_nutw_inout_dev, x->b_exp_out_dev_or_null};
    const int nOut = x->b_exp_out_dev_or_null ? 2 : 1;
    MICHK(arrays_present(who, in, 9));
    MICHK(outputs_distinct(who, in, 9, out, nOut));
    MICHK(arrays_aligned8(who, (const void* const*)in, 9));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    if (x->b_iter_out_dev_or_null) {
        const void* it = x->b_iter_out_dev_or_null;
        for (int i = 0; i < 9; ++i) if (it == (const void*)in[i]) return fail(MI_ERR_ARG, who + ": an output must not alias an input");
        for (int i = 0; i < nOut; ++i) if (it == (const void*)out[i]) return fail(MI_ERR_ARG, who + ": the outputs must differ");
        if (((uintptr_t)it & 3u) != 0) return fail(MI_ERR_ARG, who + ": the iteration counts must be aligned to 4 bytes");
    }
    HIPCHK(hipSetDevice(h->ctx->device));
    SaWallArgs q{};
    q.faces = h->faces.p; q.faceCell = h->faceCell.p; q.nFaces = h->nWallFaces;
    q.kappa = coeffs->wallKappa; q.invE = coeffs->invE;
    for (int d = 0; d < 3; ++d) { q.u[d] = x->u_dev[d]; q.buw[d] = x->b_uw_dev[d]; }
    q.bdc = x->b_delta_coeffs_dev; q.by = x->b_y_dev; q.bnuw = x->b_nuw_dev;
    q.bnut = x->b_nutw_inout_dev; q.bexp = x->b_exp_out_dev_or_null; q.biter = x->b_iter_out_dev_or_null;
    k_sa_nut_spalding_wall<<<grid_for(h->ctx, h->nWallFaces), 256, 0, h->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
