// les.inc -- the sub-grid-scale models incompressible::LESModels::Smagorinsky, oneEqEddy and dynOneEqEddy with cubeRootVolDelta and the simple
// filter (turbulenceModels/incompressible/LES/Smagorinsky/Smagorinsky.C:45-49, Smagorinsky.H:117-120; oneEqEddy/oneEqEddy.C:46-50, :100-122;
// dynOneEqEddy/dynOneEqEddy.C:45-100, :134-137, :145-172; LES/LESfilters/simpleFilter/simpleFilter.C:64-125;
// LES/LESdeltas/cubeRootVolDelta/cubeRootVolDelta.C:42-76; included by engine.hip after central.inc; DESIGN 3.5s).
//
//   filter     simpleFilter.C:64-125  surfaceSum(magSf*interpolate(vf))/surfaceSum(magSf) for up to nine components in ONE row pass on the
//              mi_average_t handle: lambda and magSf staged once per face, the neighbour's components gathered, no face field written
//   delta      cubeRootVolDelta.C:48, :68
//   cell maps  Smagorinsky's k and nuSgs; the k equation's G, sp and DkEff; nuSgs of the one-equation models; the four maps of the dynamic
//              procedure between its three filter levels (dynOneEqEddy.C:56-100, :136, :151-152)
// A cell meets its faces in the order of 3.5k.  Symmetric tensors are six arrays xx, xy, xz, yy, yz, zz.  max is (a > b) ? a : b, mag is fabs.
// Everything is rounded operation by operation (-ffp-contract=off); every fma below is written: the interpolate (mi_face_interpolate's
// rule), magSqr of a vector and of a symmetric tensor (3.5o), the double inner product.  dev has none.  Restated in tests/les_support.py.
namespace mi {

constexpr double LES_SMALL = 1.0e-15, LES_VSMALL = 1.0e-300;   // doubleScalar.H:55-57

// ---- the filter -------------------------------------------------------------------------------------------------------------------------------
struct LesFilterArgs {
    RowTables r;
    const double *magSf, *bMagSf, *lambda, *sum;
    const double* v[9];
    const double* bv[9];
    double* out[9];
};
// per face i_k = fma(lambda, P_k - N_k, N_k), p = magSf*i_k rounded, s_k = s_k + p; the face value is formed on both sides of a face from the
// same operands, hence with the same bits; a cell reads its neighbours' INPUT values, so no output is an input
template <int BS, int NC>
__global__ __launch_bounds__(BS) void k_les_filter(const LesFilterArgs a)
{
    const double* const src[2] = {a.magSf, a.lambda};
    double s[NC], pc[NC];
    mu_rows<BS, 2>(a.r, src,
        [&](int c) {
#pragma unroll
            for (int k = 0; k < NC; ++k) { pc[k] = a.v[k][c]; s[k] = 0.0; }
        },
        [&](int, int f, const double (&v)[2]) {
            const int N = a.r.up[f];
#pragma unroll
            for (int k = 0; k < NC; ++k) { const double vn = a.v[k][N], i = fma(v[1], pc[k] - vn, vn), p = v[0] * i; s[k] = s[k] + p; }
        },
        [&](int, int f, const double (&v)[2]) {
            const int P = a.r.lo[f];
#pragma unroll
            for (int k = 0; k < NC; ++k) { const double vp = a.v[k][P], i = fma(v[1], vp - pc[k], pc[k]), p = v[0] * i; s[k] = s[k] + p; }
        },
        [&](int, int bf) {
            const double m = a.bMagSf[bf];
#pragma unroll
            for (int k = 0; k < NC; ++k) { const double p = m * a.bv[k][bf]; s[k] = s[k] + p; }
        },
        [&](int c) {
            const double t = a.sum[c];
#pragma unroll
            for (int k = 0; k < NC; ++k) a.out[k][c] = s[k] / t;     // VectorSpaceI.H:621-630 with divideOp3 (ops.H): a division per component
        });
}

// ---- the cell maps ----------------------------------------------------------------------------------------------------------------------------
struct LesCell {
    const double* in[20];
    double* out[16];
    uint32_t n;                                       // the entries refuse more than INT32_MAX cells
    int vec;
    uint32_t want;                                    // bit k: output k is written (an optional output that is not wanted is NULL)
    int flag;                                         // dyn_level1: clip; delta: 2-D
    double c[3];
};
// the argument block in the kernel's argument segment, as sst_args: the widest map has 35 array bases, which do not fit in scalar registers
// across the loop; they are read where the loads and where the stores need them
typedef const LesCell __attribute__((address_space(4)))* LesArgs;
__device__ __forceinline__ LesArgs les_args()
{
    LesArgs p = (LesArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// sst_map on a LesCell: two cells per thread with 16-byte accesses when every array allows it (a.vec), one by one otherwise; outputs from
// NREQ on are written only when wanted (the mask is read with the bases)
template <int NIN, int NOUT, int NREQ, class F>
__device__ __forceinline__ void les_map(const LesCell& a, F f)
{
    const uint32_t n = a.n, np = a.vec ? n >> 1 : 0, t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (uint32_t q = t; q < np; q += stride) {
        const uint32_t i = 2 * q;
        double x[NIN], y[NIN], ox[NOUT], oy[NOUT];
        LesArgs p = les_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) { const double2 v = ld2(p->in[k], i); x[k] = v.x; y[k] = v.y; }
        f(x, ox); f(y, oy);
        p = les_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (p->want >> k & 1u)) st2(p->out[k], i, make_double2(ox[k], oy[k]));
    }
    for (uint32_t i = 2 * np + t; i < n; i += stride) {
        double x[NIN], o[NOUT];
        LesArgs p = les_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) x[k] = p->in[k][i];
        f(x, o);
        p = les_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (p->want >> k & 1u)) p->out[k][i] = o[k];
    }
}

// symm (TensorI.H:483-491) of g[3*j + k] = d(U_j)/dx_k -> xx, xy, xz, yy, yz, zz
__device__ __forceinline__ void les_symm(const double* g, double* d)
{
    d[0] = g[0]; d[1] = 0.5 * (g[1] + g[3]); d[2] = 0.5 * (g[2] + g[6]); d[3] = g[4]; d[4] = 0.5 * (g[5] + g[7]); d[5] = g[8];
}
// dev (SymmTensorI.H:326-329): st - (1.0/3.0)*tr(st) with tr = (xx + yy) + zz; the product has three uses and is not contracted
__device__ __forceinline__ void les_dev(double* d)
{
    const double t = (1.0 / 3.0) * ((d[0] + d[3]) + d[5]);
    d[0] = d[0] - t; d[3] = d[3] - t; d[5] = d[5] - t;
}
// magSqr of a symmetric tensor (SymmTensorI.H:276-284): ke_magsqr_symm's chain on the six components
__device__ __forceinline__ double les_magsqr_st(const double* d)
{
    double s = fma(d[0], d[0], 2.0 * (d[1] * d[1]));
    s = fma(2.0, d[2] * d[2], s);
    s = fma(d[3], d[3], s);
    s = fma(2.0, d[4] * d[4], s);
    s = fma(d[5], d[5], s);
    return s;
}
// && (SymmTensorI.H:233-241): every product but the first contracted into the running sum
__device__ __forceinline__ double les_ddot(const double* a, const double* b)
{
    double s = fma(a[0], b[0], (2.0 * a[1]) * b[1]);
    s = fma(2.0 * a[2], b[2], s);
    s = fma(a[3], b[3], s);
    s = fma(2.0 * a[4], b[4], s);
    s = fma(a[5], b[5], s);
    return s;
}
// magSqr of a vector (VectorSpaceI.H:336-344): the contraction of 3.5a
__device__ __forceinline__ double les_magsqr_v(const double* u) { return fma(u[2], u[2], fma(u[0], u[0], u[1] * u[1])); }

// in: V; out: delta, the root (optional).  c[0] = deltaCoeff, c[1] = thickness (flag: 2-D)
__global__ __launch_bounds__(256) void k_les_delta(const LesCell a)
{
    const double dc = a.c[0], th = a.c[1];
    const int flat = a.flag;
    les_map<1, 2, 1>(a, [=](const double (&x)[1], double (&o)[2]) {
        const double p = flat ? sqrt(x[0] / th) : pow(x[0], 1.0 / 3.0);
        o[0] = dc * p; o[1] = p;
    });
}
// in: delta, gradU[9]; out: nuSgs, k (optional).  c[0] = (2.0*ck)/ce, c[1] = ck
__global__ __launch_bounds__(256) void k_les_smagorinsky(const LesCell a)
{
    const double c0 = a.c[0], ck = a.c[1];
    les_map<10, 2, 1>(a, [=](const double (&x)[10], double (&o)[2]) {
        double d[6];
        les_symm(x + 1, d); les_dev(d);
        const double k = (c0 * (x[0] * x[0])) * les_magsqr_st(d);
        o[0] = (ck * x[0]) * sqrt(k); o[1] = k;
    });
}
// in: nuSgs, gradU[9], k, delta, [nu], [ce]; out: G, sp, dk.  c[0] = ce, c[1] = nu
template <bool NUF, bool CEF>
__global__ __launch_bounds__(256) void k_les_k_terms(const LesCell a)
{
    constexpr int NIN = 12 + (NUF ? 1 : 0) + (CEF ? 1 : 0);
    const double ce0 = a.c[0], nu0 = a.c[1];
    les_map<NIN, 3, 3>(a, [=](const double (&x)[NIN], double (&o)[3]) {
        const double nu = NUF ? x[12] : nu0, ce = CEF ? x[NIN - 1] : ce0;
        o[0] = (x[0] * 2.0) * ke_magsqr_symm(x + 1);
        o[1] = (ce * sqrt(x[10])) / x[11];
        o[2] = x[0] + nu;
    });
}
// in: k, delta, [ck]; out: nuSgs = (ck*sqrt(k))*delta
template <bool CKF>
__global__ __launch_bounds__(256) void k_les_nusgs(const LesCell a)
{
    constexpr int NIN = CKF ? 3 : 2;
    const double ck0 = a.c[0];
    les_map<NIN, 1, 1>(a, [=](const double (&x)[NIN], double (&o)[1]) { o[0] = ((CKF ? x[NIN - 1] : ck0) * sqrt(x[0])) * x[1]; });
}
// in: U[3], gradU[9]; out: sqr(U)[6], magSqr(U), D[6], magSqr(D)
__global__ __launch_bounds__(256) void k_les_dyn_moments(const LesCell a)
{
    les_map<12, 14, 14>(a, [](const double (&x)[12], double (&o)[14]) {
        o[0] = x[0] * x[0]; o[1] = x[0] * x[1]; o[2] = x[0] * x[2]; o[3] = x[1] * x[1]; o[4] = x[1] * x[2]; o[5] = x[2] * x[2];
        o[6] = les_magsqr_v(x);
        les_symm(x + 3, o + 7);
        o[13] = les_magsqr_st(o + 7);
    });
}
// in: delta, nuEff, fU[3], fSqrU[6], fMagSqrU, fD[6], fMagSqrD; out: KK, LL[6], MM[6], ce_num, ce_den, pow(KK, 1.5) (optional)
__global__ __launch_bounds__(256) void k_les_dyn_level1(const LesCell a)
{
    les_map<19, 16, 15>(a, [](const double (&x)[19], double (&o)[16]) {
        const double delta = x[0], nuEff = x[1];
        const double *fU = x + 2, *fS = x + 5, *fD = x + 12;
        double KK = 0.5 * (x[11] - les_magsqr_v(fU));
        if (les_args()->flag) KK = mu_max(KK, LES_SMALL);     // read here, like the bases: not held across the loop
        double l[6];
        l[0] = fS[0] - fU[0] * fU[0]; l[1] = fS[1] - fU[0] * fU[1]; l[2] = fS[2] - fU[0] * fU[2];
        l[3] = fS[3] - fU[1] * fU[1]; l[4] = fS[4] - fU[1] * fU[2]; l[5] = fS[5] - fU[2] * fU[2];
        les_dev(l);
        const double m = (-2.0 * delta) * sqrt(KK), p = pow(KK, 1.5);
        o[0] = KK;
#pragma unroll
        for (int k = 0; k < 6; ++k) { o[1 + k] = l[k]; o[7 + k] = m * fD[k]; }
        o[13] = nuEff * (x[18] - les_magsqr_st(fD));
        o[14] = p / (2.0 * delta);
        o[15] = p;
    });
}
// in: fLL[6], fMM[6]; out: 0.5*(fLL && fMM), magSqr(fMM)
__global__ __launch_bounds__(256) void k_les_dyn_level2(const LesCell a)
{
    les_map<12, 2, 2>(a, [](const double (&x)[12], double (&o)[2]) { o[0] = 0.5 * les_ddot(x, x + 6); o[1] = les_magsqr_st(x + 6); });
}
// in: f_lm, f_mmmm, f_ce_num, f_ce_den; out: ck, ce
__global__ __launch_bounds__(256) void k_les_dyn_coeffs(const LesCell a)
{
    les_map<4, 2, 2>(a, [](const double (&x)[4], double (&o)[2]) {
        const double c = x[0] / (x[1] + LES_VSMALL), e = x[2] / x[3];
        o[0] = 0.5 * (fabs(c) + c);
        o[1] = 0.5 * (fabs(e) + e);
    });
}

} // namespace mi

namespace {
int les_coeffs_check(const std::string& who, const mi_les_coeffs* k)
{
    if (!k) return fail(MI_ERR_ARG, who + ": the coefficients are missing");
    if (!ke_positive(k->ck) || !ke_positive(k->ce)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_les_coeffs_init)");
    return MI_OK;
}
// ke_cell_pass on a LesCell; outputs from nReq on are optional (NULL: not written)
template <class K>
int les_cell_pass(const std::string& who, mi_ctx_s* c, int64_t n, K kernel, mi::LesCell& q, const double* const* in, int nIn, double* const* out, int nOut,
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
// the pointers of a caller's array of arrays, or NULLs when it is missing itself
template <class T>
void les_take(T* dst, T const* src, int n) { for (int i = 0; i < n; ++i) dst[i] = src ? src[i] : nullptr; }

template <int NC>
int les_filter_launch(mi_addr_s* a, mi::LesFilterArgs& q) { return row_launch_bs(a, 2, ROW_BS(mi::k_les_filter, NC), q); }
} // namespace

extern "C" int mi_les_coeffs_init(double ck, double ce, mi_les_coeffs* out)
{
    const std::string who = "mi_les_coeffs_init";
    if (!out) return fail(MI_ERR_ARG, who + ": bad argument");
    mi_les_coeffs k{};
    k.ck = ck; k.ce = ce;
    if (!ke_positive(ck) || !ke_positive(ce)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    *out = k;
    return MI_OK;
}

extern "C" int mi_les_simple_filter(mi_average_t h, int n_cmpt, const double* lambda_dev, const double* mag_sf_dev, const double* b_mag_sf_dev,
                                    const double* const* vf_dev, const double* const* b_face_dev, double* const* out_dev)
{
    const std::string who = "mi_les_simple_filter";
    MICHK(row_handle_check(who, h));
    if (n_cmpt < 1 || n_cmpt > 9) return fail(MI_ERR_ARG, who + ": n_cmpt must be 1 to 9");
    if (h->nCells == 0) return MI_OK;
    if (!vf_dev || !out_dev) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (h->nFaces > 0 && (!mag_sf_dev || !lambda_dev)) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (h->nBFaces > 0 && (!b_mag_sf_dev || !b_face_dev)) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary arrays needed");
    const double* in[21];                             // an empty array may be NULL and is never read
    int nIn = 0;
    if (h->nFaces > 0) { in[nIn++] = mag_sf_dev; in[nIn++] = lambda_dev; }
    for (int k = 0; k < n_cmpt; ++k) in[nIn++] = vf_dev[k];
    if (h->nBFaces > 0) {
        in[nIn++] = b_mag_sf_dev;
        for (int k = 0; k < n_cmpt; ++k) {
            if (!b_face_dev[k]) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary arrays needed");
            in[nIn++] = b_face_dev[k];
        }
    }
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out_dev, n_cmpt));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out_dev, n_cmpt));
    mi_addr_s* a = h->addr;
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    LesFilterArgs q{};
    q.r = row_tables(a, h->boundary);
    q.magSf = mag_sf_dev; q.bMagSf = b_mag_sf_dev; q.lambda = lambda_dev; q.sum = h->sum.p;
    for (int k = 0; k < n_cmpt; ++k) { q.v[k] = vf_dev[k]; q.bv[k] = h->nBFaces > 0 ? b_face_dev[k] : nullptr; q.out[k] = out_dev[k]; }
    switch (n_cmpt) {
    case 1: return les_filter_launch<1>(a, q);
    case 2: return les_filter_launch<2>(a, q);
    case 3: return les_filter_launch<3>(a, q);
    case 4: return les_filter_launch<4>(a, q);
    case 5: return les_filter_launch<5>(a, q);
    case 6: return les_filter_launch<6>(a, q);
    case 7: return les_filter_launch<7>(a, q);
    case 8: return les_filter_launch<8>(a, q);
    default: return les_filter_launch<9>(a, q);
    }
}

extern "C" int mi_les_delta_cube_root_vol(mi_ctx_t c, int64_t n, double delta_coeff, double thickness_or_0, const double* v_dev, double* out_dev,
                                          double* pow_out_dev_or_null)
{
    const std::string who = "mi_les_delta_cube_root_vol";
    if (!std::isfinite(delta_coeff) || !std::isfinite(thickness_or_0) || thickness_or_0 < 0) return fail(MI_ERR_ARG, who + ": deltaCoeff must be finite and the thickness finite and not negative");
    LesCell q{};
    q.c[0] = delta_coeff; q.c[1] = thickness_or_0; q.flag = thickness_or_0 > 0 ? 1 : 0;
    const double* in[1] = {v_dev};
    double* out[2] = {out_dev, pow_out_dev_or_null};
    return les_cell_pass(who, c, n, k_les_delta, q, in, 1, out, 2, 1);
}

extern "C" int mi_les_smagorinsky(mi_ctx_t c, int64_t n, const mi_les_coeffs* coeffs, const double* delta_dev, const double* const* grad_dev,
                                  double* k_out_dev_or_null, double* nusgs_out_dev)
{
    const std::string who = "mi_les_smagorinsky";
    MICHK(les_coeffs_check(who, coeffs));
    LesCell q{};
    q.c[0] = (2.0 * coeffs->ck) / coeffs->ce; q.c[1] = coeffs->ck;
    const double* in[10] = {delta_dev};
    les_take(in + 1, grad_dev, 9);
    double* out[2] = {nusgs_out_dev, k_out_dev_or_null};
    return les_cell_pass(who, c, n, k_les_smagorinsky, q, in, 10, out, 2, 1);
}

extern "C" int mi_les_k_terms(mi_ctx_t c, int64_t n, double ce, const double* ce_dev_or_null, const double* nusgs_dev, const double* const* grad_dev,
                              const double* k_dev, const double* delta_dev, const double* nu_dev_or_null, double nu_value, double* g_out_dev,
                              double* sp_out_dev, double* dk_out_dev)
{
    const std::string who = "mi_les_k_terms";
    if (!ce_dev_or_null && !ke_positive(ce)) return fail(MI_ERR_ARG, who + ": ce must be a finite number above zero");
    LesCell q{};
    q.c[0] = ce; q.c[1] = nu_value;
    const double* in[14] = {nusgs_dev};
    les_take(in + 1, grad_dev, 9);
    in[10] = k_dev; in[11] = delta_dev;
    int nIn = 12;
    if (nu_dev_or_null) in[nIn++] = nu_dev_or_null;
    if (ce_dev_or_null) in[nIn++] = ce_dev_or_null;
    double* out[3] = {g_out_dev, sp_out_dev, dk_out_dev};
    if (nu_dev_or_null) return ce_dev_or_null ? les_cell_pass(who, c, n, k_les_k_terms<true, true>, q, in, nIn, out, 3, 3)
                                              : les_cell_pass(who, c, n, k_les_k_terms<true, false>, q, in, nIn, out, 3, 3);
    return ce_dev_or_null ? les_cell_pass(who, c, n, k_les_k_terms<false, true>, q, in, nIn, out, 3, 3)
                          : les_cell_pass(who, c, n, k_les_k_terms<false, false>, q, in, nIn, out, 3, 3);
}

extern "C" int mi_les_nusgs(mi_ctx_t c, int64_t n, double ck, const double* ck_dev_or_null, const double* k_dev, const double* delta_dev, double* out_dev)
{
    const std::string who = "mi_les_nusgs";
    if (!ck_dev_or_null && !ke_positive(ck)) return fail(MI_ERR_ARG, who + ": ck must be a finite number above zero");
    LesCell q{};
    q.c[0] = ck;
    const double* in[3] = {k_dev, delta_dev, ck_dev_or_null};
    double* out[1] = {out_dev};
    if (ck_dev_or_null) return les_cell_pass(who, c, n, k_les_nusgs<true>, q, in, 3, out, 1, 1);
    return les_cell_pass(who, c, n, k_les_nusgs<false>, q, in, 2, out, 1, 1);
}

extern "C" int mi_les_dyn_moments(mi_ctx_t c, int64_t n, const double* const* u_dev, const double* const* grad_dev, double* const* sqr_u_out_dev,
                                  double* magsqr_u_out_dev, double* const* d_out_dev, double* magsqr_d_out_dev)
{
    const std::string who = "mi_les_dyn_moments";
    LesCell q{};
    const double* in[12];
    les_take(in, u_dev, 3); les_take(in + 3, grad_dev, 9);
    double* out[14];
    les_take(out, sqr_u_out_dev, 6); out[6] = magsqr_u_out_dev; les_take(out + 7, d_out_dev, 6); out[13] = magsqr_d_out_dev;
    return les_cell_pass(who, c, n, k_les_dyn_moments, q, in, 12, out, 14, 14);
}

extern "C" int mi_les_dyn_level1(mi_ctx_t c, int64_t n, int clip, const double* delta_dev, const double* nueff_dev, const double* const* f_u_dev,
                                 const double* const* f_sqr_u_dev, const double* f_magsqr_u_dev, const double* const* f_d_dev,
                                 const double* f_magsqr_d_dev, double* kk_out_dev, double* const* ll_out_dev, double* const* mm_out_dev,
                                 double* ce_num_out_dev, double* ce_den_out_dev, double* pow_out_dev_or_null)
{
    const std::string who = "mi_les_dyn_level1";
    LesCell q{};
    q.flag = clip ? 1 : 0;
    const double* in[19] = {delta_dev, nueff_dev};
    les_take(in + 2, f_u_dev, 3); les_take(in + 5, f_sqr_u_dev, 6); in[11] = f_magsqr_u_dev; les_take(in + 12, f_d_dev, 6); in[18] = f_magsqr_d_dev;
    double* out[16] = {kk_out_dev};
    les_take(out + 1, ll_out_dev, 6); les_take(out + 7, mm_out_dev, 6);
    out[13] = ce_num_out_dev; out[14] = ce_den_out_dev; out[15] = pow_out_dev_or_null;
    return les_cell_pass(who, c, n, k_les_dyn_level1, q, in, 19, out, 16, 15);
}

extern "C" int mi_les_dyn_level2(mi_ctx_t c, int64_t n, const double* const* f_ll_dev, const double* const* f_mm_dev, double* lm_out_dev,
                                 double* mmmm_out_dev)
{
    const std::string who = "mi_les_dyn_level2";
    LesCell q{};
    const double* in[12];
    les_take(in, f_ll_dev, 6); les_take(in + 6, f_mm_dev, 6);
    double* out[2] = {lm_out_dev, mmmm_out_dev};
    return les_cell_pass(who, c, n, k_les_dyn_level2, q, in, 12, out, 2, 2);
}

extern "C" int mi_les_dyn_coeffs(mi_ctx_t c, int64_t n, const double* f_lm_dev, const double* f_mmmm_dev, const double* f_ce_num_dev,
                                 const double* f_ce_den_dev, double* ck_out_dev, double* ce_out_dev)
{
    const std::string who = "mi_les_dyn_coeffs";
    LesCell q{};
    const double* in[4] = {f_lm_dev, f_mmmm_dev, f_ce_num_dev, f_ce_den_dev};
    double* out[2] = {ck_out_dev, ce_out_dev};
    return les_cell_pass(who, c, n, k_les_dyn_coeffs, q, in, 4, out, 2, 2);
}
