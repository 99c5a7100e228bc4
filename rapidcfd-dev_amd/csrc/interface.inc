// interface.inc -- interFoam's interfaceProperties (transportModels/interfaceProperties/interfaceProperties.C:58-159, :220-231; included by
// engine.hip after mules.inc; DESIGN 3.5n): the face unit interface normal flux nHatf with the contact-angle correction, the curvature
// K = -fvc::div(nHatf), the surface tension force fvc::interpolate(sigma*K)*fvc::snGrad(alpha1) and nearInterface.
//
//   nHatf      :127, :134, :143 in one face pass: g = interpolate(gradAlpha) (mi_face_interpolate's fma), m = mag(g) (the contracted magSqr of
//              3.5a under a correctly rounded sqrt), d = m + deltaN, n = g/d (three divisions: VectorSpace's operator/ divides component by
//              component, no reciprocal is formed), nHatf = n & Sf (the contracted dot of 3.5a).
//   patches    coupled: g = w*gP + (1 - w)*gNbr, every operator rounded (surfaceInterpolationScheme.C:361-366); other: g the boundary value of
//              gradAlpha as the caller evaluated it; a contact-angle patch then runs correctContactAngle :83-111 operation for operation.
//   curvature  :146: surfaceIntegrate in 3.5k's order (own faces ascending, losort faces, boundary faces patch by patch), /V, unary minus.
//   force      :223: sigmaK() is a cell product BEFORE the interpolate; snGrad = deltaCoeffs*(alphaN - alphaP) [+ the explicit correction].
// Everything is rounded operation by operation (-ffp-contract=off); every fma below is written.  Restated in tests/interface_support.py, not
// pinned by a compiled reference.
namespace mi {

__device__ __forceinline__ double if_dot(const double (&a)[3], const double (&b)[3]) { return fma(a[2], b[2], fma(a[0], b[0], a[1] * b[1])); }
__device__ __forceinline__ double if_mag(const double (&a)[3]) { return sqrt(if_dot(a, a)); }

// steps 2-4: g -> n = g/(mag(g) + deltaN); returns mag(g)
__device__ __forceinline__ double if_unit(const double (&g)[3], double deltaN, double (&n)[3])
{
    const double m = if_mag(g), d = m + deltaN;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = g[k] / d;
    return m;
}

struct NhArgs {
    const int32_t *lo, *up;                           // internal faces; the patch forms: lo = faceCells (coupled only)
    const double *lambda;                             // the patch forms: the patch weights, or NULL (g[] is then the boundary value itself)
    const double *sf[3], *g[3], *nbr[3];
    const double *magSf, *theta;                      // the contact-angle form
    double *nhatf, *nv[3], *gradient, *b1, *b2;
    double deltaN, toRad;
    int nf, xcd;
};

// the internal faces: XCD-aware chunks as k_interface_compression; lambda and Sf streamed, the gradient gathered twice
template <bool VEC>
__global__ __launch_bounds__(256) void k_interface_nhatf(const NhArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        const double w = a.lambda[f];
        double g[3], n[3], s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double gP = a.g[k][P], gN = a.g[k][N]; g[k] = fma(w, gP - gN, gN); s[k] = a.sf[k][f]; }
        if_unit(g, a.deltaN, n);
        if (VEC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.nv[k][f] = n[k];
        }
        a.nhatf[f] = if_dot(n, s);
    }
}

// one patch, one thread per face.  ANGLE: correctContactAngle (:83-111) between step 4 and step 5
template <bool ANGLE>
__global__ __launch_bounds__(256) void k_patch_interface_nhatf(const NhArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nf) return;
    double g[3], n[3], s[3];
    if (a.lambda) {
        const int c = a.lo[i];
        const double w = a.lambda[i], v = 1.0 - w;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double p = w * a.g[k][c], q = v * a.nbr[k][i]; g[k] = p + q; }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = a.g[k][i];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = a.sf[k][i];
    const double m = if_unit(g, a.deltaN, n);
    if (ANGLE) {
        const double theta = a.toRad * a.theta[i], ms = a.magSf[i];
        double nf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) nf[k] = s[k] / ms;                        // fvPatch::nf() divides on every call
        const double a12 = if_dot(n, nf);
        const double b1 = cos(theta);
        const double ac = acos(a12), b2 = cos(ac - theta);
        if (a.b1) { a.b1[i] = b1; a.b2[i] = b2; }
        const double sq = a12 * a12, det = 1.0 - sq;
        const double p1 = a12 * b2, p2 = a12 * b1;
        const double ca = (b1 - p1) / det, cb = (b2 - p2) / det;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double x = ca * nf[k], y = cb * n[k]; n[k] = x + y; }
        const double d = if_mag(n) + a.deltaN;
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = n[k] / d;
        if (a.gradient) a.gradient[i] = if_dot(nf, n) * m;
    }
    if (a.nv[0]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.nv[k][i] = n[k];
    }
    a.nhatf[i] = if_dot(n, s);
}

// K = -fvc::div(nHatf): k_mules_solve's walk, then /V and a true sign flip (a cell without flux gives -0.0)
template <int BS>
__global__ __launch_bounds__(BS) void k_interface_curvature(const MuArgs a)
{
    const RowTables& r = a.r; const MuCells& q = a.q; const MuFlux& x = a.x;
    const double* const src[1] = {x.phiPsi};
    double s = 0.0;
    mu_rows<BS, 1>(r, src, [](int) {},
        [&](int, int, const double (&v)[1]) { s = s + v[0]; },
        [&](int, int, const double (&v)[1]) { s = s - v[0]; },
        [&](int, int bf) { s = s + x.bphiPsi[bf]; },
        [&](int c) { const double d = s / q.vol[c]; x.out[c] = -d; });
}

struct StArgs {
    const int32_t *lo, *up;                           // the patch form: lo = faceCells
    const double *lambda, *dc, *K, *alpha, *corr, *nbrK, *nbrAlpha;
    double* out;
    double sigma;
    int nf, xcd;
};
template <bool CORR>
__global__ __launch_bounds__(256) void k_surface_tension_force(const StArgs a)
{
    int f0, f1; block_chunk(a.nf, a.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const int P = a.lo[f], N = a.up[f];
        const double sP = a.sigma * a.K[P], sN = a.sigma * a.K[N];
        const double i = fma(a.lambda[f], sP - sN, sN);
        const double d = a.alpha[N] - a.alpha[P];
        double sn = a.dc[f] * d;
        if (CORR) sn = sn + a.corr[f];
        a.out[f] = i * sn;
    }
}
// one COUPLED patch: the interpolate of surfaceInterpolationScheme.C:361-366, coupledFvPatchField::snGrad
template <bool CORR>
__global__ __launch_bounds__(256) void k_patch_surface_tension_force(const StArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nf) return;
    const int c = a.lo[i];
    const double w = a.lambda[i], sP = a.sigma * a.K[c], sN = a.sigma * a.nbrK[i];
    const double p = w * sP, q = (1.0 - w) * sN, ip = p + q;
    const double d = a.nbrAlpha[i] - a.alpha[c];
    double sn = a.dc[i] * d;
    if (CORR) sn = sn + a.corr[i];
    a.out[i] = ip * sn;
}

// pos(alpha - 0.01)*pos(0.99 - alpha), pos(x) = (x >= 0) ? 1 : 0
__global__ __launch_bounds__(RB) void k_near_interface(const double* alpha, double* out, int64_t n) // out may alias alpha
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = alpha[i], p = (x - 0.01) >= 0 ? 1.0 : 0.0, q = (0.99 - x) >= 0 ? 1.0 : 0.0;
        out[i] = p * q;
    }
}

} // namespace mi

// the curvature's row pass on one mesh: the addressing's row tables and the boundary's per-cell face lists (the lists the MULES handle walks)
struct mi_interface_s : RowHandle {};

namespace {
int if_delta_n(const std::string& who, double deltaN)
{
    if (!std::isfinite(deltaN) || !(deltaN > 0)) return fail(MI_ERR_ARG, who + ": delta_n must be a finite number above zero");
    return MI_OK;
}
} // namespace

extern "C" int mi_interface_nhatf(mi_addr_t a, double delta_n, const double* lambda_dev, const double* const* sf_dev, const double* const* grad_dev,
                                  double* nhatf_out_dev, double* const* nhatfv_out_dev_or_null)
{
    const std::string who = "mi_interface_nhatf";
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(if_delta_n(who, delta_n));
    if (!grad_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    if (!sf_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    const double* in[7] = {lambda_dev, sf_dev[0], sf_dev[1], sf_dev[2], grad_dev[0], grad_dev[1], grad_dev[2]};
    double* out[4] = {nhatf_out_dev, nullptr, nullptr, nullptr};
    int nOut = 1;
    if (nhatfv_out_dev_or_null) for (int k = 0; k < 3; ++k) out[nOut++] = nhatfv_out_dev_or_null[k];
    MICHK(arrays_present(who, in, 7));
    MICHK(outputs_distinct(who, in, 7, out, nOut));
    bool ok = true;
    for (int i = 0; i < 4; ++i) ok = ok && al16(in[i]);
    for (int i = 4; i < 7; ++i) ok = ok && al8(in[i]);
    for (int i = 0; i < nOut; ++i) ok = ok && al16(out[i]);
    if (!ok) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned, the cell fields to 8 bytes");
    NhArgs q{};
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.lambda = lambda_dev; q.nhatf = nhatf_out_dev; q.deltaN = delta_n;
    for (int k = 0; k < 3; ++k) { q.sf[k] = sf_dev[k]; q.g[k] = grad_dev[k]; q.nv[k] = nOut > 1 ? out[1 + k] : nullptr; }
    q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    if (nOut > 1) k_interface_nhatf<true><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    else k_interface_nhatf<false><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_patch_interface_nhatf(mi_patch_t p, double delta_n, const mi_patch_nhatf* x)
{
    const std::string who = "mi_patch_interface_nhatf";
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(if_delta_n(who, delta_n));
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    const bool coupled = x->patch_weights_dev != nullptr, angle = x->theta_deg_dev != nullptr;
    if (angle && coupled) return fail(MI_ERR_ARG, who + ": a contact-angle patch is not coupled: theta_deg with patch_weights NULL only");
    if (!angle && (x->gradient_out_dev || x->b1_out_dev || x->b2_out_dev))
        return fail(MI_ERR_ARG, who + ": gradient_out and b1_out / b2_out belong to the contact-angle form (theta_deg missing)");
    if ((x->b1_out_dev != nullptr) != (x->b2_out_dev != nullptr)) return fail(MI_ERR_ARG, who + ": b1_out and b2_out come together or not at all");
    if (p->nFaces == 0) return MI_OK;
    if (angle && !x->patch_magsf_dev) return fail(MI_ERR_ARG, who + ": the contact-angle form needs patch_magsf: input arrays missing");
    const double* in[12];
    int nIn = 0;
    for (int k = 0; k < 3; ++k) in[nIn++] = x->grad_dev[k];
    for (int k = 0; k < 3; ++k) in[nIn++] = x->patch_sf_dev[k];
    if (coupled) { in[nIn++] = x->patch_weights_dev; for (int k = 0; k < 3; ++k) in[nIn++] = x->nbr_grad_dev[k]; }
    if (angle) { in[nIn++] = x->patch_magsf_dev; in[nIn++] = x->theta_deg_dev; }
    double* out[7] = {x->nhatf_out_dev};
    int nOut = 1;
    const bool vec = x->nhatfv_out_dev[0] || x->nhatfv_out_dev[1] || x->nhatfv_out_dev[2];
    if (vec) for (int k = 0; k < 3; ++k) out[nOut++] = x->nhatfv_out_dev[k];
    if (x->gradient_out_dev) out[nOut++] = x->gradient_out_dev;
    if (x->b1_out_dev) { out[nOut++] = x->b1_out_dev; out[nOut++] = x->b2_out_dev; }
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out, nOut));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    HIPCHK(hipSetDevice(p->ctx->device));
    NhArgs q{};
    q.lo = p->faceCells.p; q.lambda = x->patch_weights_dev; q.magSf = x->patch_magsf_dev; q.theta = x->theta_deg_dev;
    for (int k = 0; k < 3; ++k) { q.sf[k] = x->patch_sf_dev[k]; q.g[k] = x->grad_dev[k]; q.nbr[k] = x->nbr_grad_dev[k]; q.nv[k] = vec ? x->nhatfv_out_dev[k] : nullptr; }
    q.nhatf = x->nhatf_out_dev; q.gradient = x->gradient_out_dev; q.b1 = x->b1_out_dev; q.b2 = x->b2_out_dev;
    q.deltaN = delta_n; q.toRad = 3.14159265358979323846 / 180.0;         // convertToRad (unitConversion.H), formed on the host
    q.nf = p->nFaces;
    const int g = (p->nFaces + 255) / 256;
    if (angle) k_patch_interface_nhatf<true><<<g, 256, 0, p->ctx->stream>>>(q);
    else k_patch_interface_nhatf<false><<<g, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_interface_create(mi_addr_t a, mi_grad_boundary_t b, mi_interface_t* out)
{
    const std::string who = "mi_interface_create";
    std::unique_ptr<mi_interface_s> h(new mi_interface_s());
    MICHK(row_handle_open(who, a, b, out, *h));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    *out = h.release();
    return MI_OK;
}
extern "C" int mi_interface_destroy(mi_interface_t h) { delete h; return MI_OK; }

extern "C" int mi_interface_curvature(mi_interface_t h, const double* nhatf_dev, const double* b_nhatf_dev, const double* vol_dev, double* k_out_dev)
{
    const std::string who = "mi_interface_curvature";
    MICHK(row_handle_check(who, h));
    mi_addr_s* a = h->addr;
    if (h->nCells == 0) return MI_OK;
    if (!vol_dev) return fail(MI_ERR_ARG, who + ": a cell array is missing");
    if (h->nFaces > 0 && !nhatf_dev) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (h->nBFaces > 0 && !b_nhatf_dev) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary flux arrays needed");
    const double* in[3] = {vol_dev};                  // an empty array may be NULL and is never read
    int nIn = 1;
    if (h->nFaces > 0) in[nIn++] = nhatf_dev;
    if (h->nBFaces > 0) in[nIn++] = b_nhatf_dev;
    double* out[1] = {k_out_dev};
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out, 1));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, 1));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    MuArgs q{};
    q.r = row_tables(a, h->boundary);
    q.q.vol = vol_dev; q.x.phiPsi = nhatf_dev; q.x.bphiPsi = b_nhatf_dev; q.x.out = k_out_dev;
    return row_launch_bs(a, 1, ROW_BS(k_interface_curvature), q);
}

extern "C" int mi_surface_tension_force(mi_addr_t a, double sigma, const double* lambda_dev, const double* delta_coeffs_dev, const double* k_dev,
                                        const double* alpha_dev, const double* sngrad_corr_dev_or_null, double* out_dev)
{
    const std::string who = "mi_surface_tension_force";
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    if (!k_dev || !alpha_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    const double* in[5] = {lambda_dev, delta_coeffs_dev, k_dev, alpha_dev, sngrad_corr_dev_or_null};
    double* out[1] = {out_dev};
    MICHK(arrays_present(who, in, sngrad_corr_dev_or_null ? 5 : 4));
    MICHK(outputs_distinct(who, in, sngrad_corr_dev_or_null ? 5 : 4, out, 1));
    if (!al16(lambda_dev) || !al16(delta_coeffs_dev) || !al16(sngrad_corr_dev_or_null) || !al16(out_dev) || !al8(k_dev) || !al8(alpha_dev))
        return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned, the cell fields to 8 bytes");
    StArgs q{};
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.lambda = lambda_dev; q.dc = delta_coeffs_dev; q.K = k_dev; q.alpha = alpha_dev;
    q.corr = sngrad_corr_dev_or_null; q.out = out_dev; q.sigma = sigma; q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    if (q.corr) k_surface_tension_force<true><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    else k_surface_tension_force<false><<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_patch_surface_tension_force(mi_patch_t p, double sigma, const double* patch_weights_dev, const double* patch_delta_coeffs_dev,
                                              const double* k_dev, const double* nbr_k_dev, const double* alpha_dev, const double* nbr_alpha_dev,
                                              const double* patch_sngrad_corr_dev_or_null, double* out_dev)
{
    const std::string who = "mi_patch_surface_tension_force";
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    if (p->nFaces == 0) return MI_OK;
    const double* in[7] = {patch_weights_dev, patch_delta_coeffs_dev, k_dev, nbr_k_dev, alpha_dev, nbr_alpha_dev, patch_sngrad_corr_dev_or_null};
    double* out[1] = {out_dev};
    const int nIn = patch_sngrad_corr_dev_or_null ? 7 : 6;
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out, 1));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, 1));
    HIPCHK(hipSetDevice(p->ctx->device));
    StArgs q{};
    q.lo = p->faceCells.p; q.lambda = patch_weights_dev; q.dc = patch_delta_coeffs_dev; q.K = k_dev; q.nbrK = nbr_k_dev; q.alpha = alpha_dev;
    q.nbrAlpha = nbr_alpha_dev; q.corr = patch_sngrad_corr_dev_or_null; q.out = out_dev; q.sigma = sigma; q.nf = p->nFaces;
    const int g = (p->nFaces + 255) / 256;
    if (q.corr) k_patch_surface_tension_force<true><<<g, 256, 0, p->ctx->stream>>>(q);
    else k_patch_surface_tension_force<false><<<g, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_near_interface(mi_ctx_t c, int64_t n, const double* alpha_dev, double* out_dev)
{
    if (!c || n < 0 || (n > 0 && (!alpha_dev || !out_dev))) return fail(MI_ERR_ARG, "mi_near_interface: bad argument");
    if (!al8(alpha_dev) || !al8(out_dev)) return fail(MI_ERR_ARG, "mi_near_interface: arrays must be aligned to 8 bytes");
    if (n == 0) return MI_OK;
    return cell_launch(c, k_near_interface, alpha_dev, out_dev, n);
}
