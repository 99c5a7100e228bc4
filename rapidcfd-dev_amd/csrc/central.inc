// central.inc -- rhoCentralFoam's Kurganov and Tadmor face fluxes (applications/solvers/compressible/rhoCentralFoam/rhoCentralFoam.C:60-185,
// readFluxScheme.H, createFields.H:76-98, compressibleCourantNo.H:35-47; included by engine.hip after thermo.inc; DESIGN 3.5r).
//
//   faces      mi_central_flux: the ten limited interpolations (rho, rhoU, rPsi, e, c towards pos and towards neg) and the field operators of
//              :107-185 in ONE face pass: phi, phiUp, phiEp and the final amaxSf (:161), optionally a_pos and aU = a_pos*U_pos + a_neg*U_neg
//   patches    mi_patch_central_flux: a coupled patch (the limiter as k_patch_limited_weights calls it, w*vP + (1 - w)*vNbr with every operator
//              rounded) or any other patch (the boundary value for both directions, the same algebra operation for operation)
//   cells      mi_central_sound_speed: rPsi = 1.0/psi (:84) and c = sqrt((Cp/Cv)*rPsi) (:116)
//   Courant    mi_central_courant: max over internal and boundary faces of (deltaCoeffs*amaxSf)/magSf, sum over the internal faces of
//              deltaCoeffs*amaxSf, on the reduction trees of mi_min_max and mi_sum with the product formed on load
// The limiter is lim_face (assembly.inc) with faceFlux = +1.0 towards pos and -1.0 towards neg, the weight k_limited_weights' fma, the
// interpolate mi_face_interpolate's fma(w, vP - vN, vN).  After the interpolations every operator of the reference is a field operator of its
// own and is rounded on its own (-ffp-contract=off); the fma written are the dot product U & Sf and magSqr(U) (the contraction of DESIGN
// 3.5a: an ASSUMPTION, as 3.5n item 2).  max / min are the reference's ternaries.  Restated in tests/central_support.py, not pinned by a
// compiled reference.
namespace mi {

struct CfSlot { LimCoef k; int kind, vec; };          // one reconstruct(...) entry: lim_face's coefficients, its KIND, the V form
// the fields of one side of a face: cell arrays (internal faces, the owner side of a coupled patch), the patchNeighbourFields (the
// other side of a coupled patch) or the patch's boundary values (any other patch: the seven value arrays only)
struct CfCells {
    const double *rho, *rhoU[3], *rPsi, *e, *c;
    const double *gRho[3], *gRhoU[9], *gRPsi[3], *gE[3], *gC[3];
    const double *limU, *gLimU[3];                    // a scalar reconstruct(U): magSqr(rhoU) and its gradient
};
struct CfOut { double *phi, *phiUp[3], *phiEp, *amaxSf, *aPos, *aU[3]; };
struct CfArgs {
    const int32_t *lo, *up;                           // the patch form: lo = faceCells (coupled only)
    const double *cdw;                                // the patch form: the patch weights, or NULL
    const double *sf[3], *magSf;
    const double *cc[3];                              // the cell centres; the patch form: the patch delta
    CfCells own, nbr;                                 // internal faces: own only
    CfOut o;
    CfSlot sRho, sU, sT;
    int nf, xcd;
};

// the interpolated fields of one face, [0] towards pos, [1] towards neg
struct CfFace { double rho[2], rhoU[2][3], rPsi[2], e[2], c[2]; };
struct CfFlux { double phi, phiUp[3], phiEp, amaxSf, aPos, aU[3]; };

// the limited weights of one field in both directions through the slot's limiter: a launch-uniform switch into lim_face<KIND, VEC>.
// (A dedicated vanLeer / vanLeerV / vanLeer instantiation without the switch was measured: 76 vector registers and 6 waves per SIMD against
// 104 and 4, and 1.026 x the switch's time on the 216^3 box -- not faster, so it is not here; DESIGN 3.5r.)
template <bool VEC, class PHI, class GRAD>
__device__ __forceinline__ void cf_weights(const CfSlot& s, double cdw, const PHI& phi, const GRAD& grad, double dx, double dy, double dz, double (&w)[2])
{
    double lp = 0.0, ln = 0.0;
    switch (s.kind) {
#define MI_CF_KIND(K) case K: lp = lim_face<K, VEC>(s.k, cdw, 1.0, phi, grad, dx, dy, dz); ln = lim_face<K, VEC>(s.k, cdw, -1.0, phi, grad, dx, dy, dz); break;
        MI_CF_KIND(LIM_LINEAR) MI_CF_KIND(LIM_VANLEER) MI_CF_KIND(LIM_MUSCL) MI_CF_KIND(LIM_MINMOD) MI_CF_KIND(LIM_SUPERBEE) MI_CF_KIND(LIM_UMIST)
        MI_CF_KIND(LIM_VANALBADA) MI_CF_KIND(LIM_OSPRE) MI_CF_KIND(LIM_QUICK) MI_CF_KIND(LIM_CUBIC) MI_CF_KIND(LIM_GAMMA) MI_CF_KIND(LIM_SFCD)
#undef MI_CF_KIND
    }
    w[0] = fma(lp, cdw, (1.0 - lp) * 1.0);            // k_limited_weights' blend at pos(+1.0) = 1.0 and pos(-1.0) = 0.0
    w[1] = fma(ln, cdw, (1.0 - ln) * 0.0);
}
// internal faces: surfaceInterpolationScheme.C:274-279; a coupled patch: :361-366, every operator rounded
template <bool COUPLED>
__device__ __forceinline__ double cf_interp(double w, double vP, double vN)
{
    if (COUPLED) { const double p = w * vP, q = (1.0 - w) * vN; return p + q; }
    return fma(w, vP - vN, vN);
}
// one scalar field under a scalar limiter
template <bool COUPLED>
__device__ __forceinline__ void cf_scalar(const CfSlot& s, double cdw, const double* fP, const double* const* gP, int iP, const double* fN,
                                          const double* const* gN, int iN, double dx, double dy, double dz, double (&out)[2])
{
    const double vP = fP[iP], vN = fN[iN];
    double w[2];
    cf_weights<false>(s, cdw, [&](bool p, int) { return p ? vP : vN; }, [&](bool p, int c) { return p ? gP[c][iP] : gN[c][iN]; }, dx, dy, dz, w);
    out[0] = cf_interp<COUPLED>(w[0], vP, vN); out[1] = cf_interp<COUPLED>(w[1], vP, vN);
}
// the ten interpolations, one field at a time: side A at index iA is the owner (P), side B at iB the neighbour (N)
template <bool COUPLED>
__device__ __forceinline__ void cf_reconstruct(const CfArgs& a, double cdw, const CfCells& A, int iA, const CfCells& B, int iB, double dx, double dy,
                                               double dz, CfFace& v)
{
    cf_scalar<COUPLED>(a.sRho, cdw, A.rho, A.gRho, iA, B.rho, B.gRho, iB, dx, dy, dz, v.rho);
    {
        double uP[3], uN[3], w[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) { uP[k] = A.rhoU[k][iA]; uN[k] = B.rhoU[k][iB]; }
        if (a.sU.vec)
            cf_weights<true>(a.sU, cdw, [&](bool p, int j) { return p ? uP[j] : uN[j]; }, [&](bool p, int c) { return p ? A.gRhoU[c][iA] : B.gRhoU[c][iB]; },
                             dx, dy, dz, w);
        else {                                        // LimitFuncs.C:39-54: limited on the caller's magSqr(rhoU)
            const double mP = A.limU[iA], mN = B.limU[iB];
            cf_weights<false>(a.sU, cdw, [&](bool p, int) { return p ? mP : mN; }, [&](bool p, int c) { return p ? A.gLimU[c][iA] : B.gLimU[c][iB]; },
                              dx, dy, dz, w);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { v.rhoU[0][k] = cf_interp<COUPLED>(w[0], uP[k], uN[k]); v.rhoU[1][k] = cf_interp<COUPLED>(w[1], uP[k], uN[k]); }
    }
    cf_scalar<COUPLED>(a.sT, cdw, A.rPsi, A.gRPsi, iA, B.rPsi, B.gRPsi, iB, dx, dy, dz, v.rPsi);
    cf_scalar<COUPLED>(a.sT, cdw, A.e, A.gE, iA, B.e, B.gE, iB, dx, dy, dz, v.e);
    cf_scalar<COUPLED>(a.sT, cdw, A.c, A.gC, iA, B.c, B.gC, iB, dx, dy, dz, v.c);
}
// rhoCentralFoam.C:107-185 on one face, an operator a line
template <bool TADMOR, bool OPT>
__device__ __forceinline__ void cf_flux(const CfFace& v, const double (&s)[3], double magSf, CfFlux& o)
{
    double U[2][3], p[2], phiv[2], cSf[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
        for (int k = 0; k < 3; ++k) U[d][k] = v.rhoU[d][k] / v.rho[d];        // :107-108: three divisions, no reciprocal
        p[d] = v.rho[d] * v.rPsi[d];                                          // :110-111
        phiv[d] = if_dot(U[d], s);                                            // :113-114
        cSf[d] = v.c[d] * magSf;                                              // :117-126
    }
    const double ap = rmax(rmax(phiv[0] + cSf[0], phiv[1] + cSf[1]), 0.0);    // :128-132
    const double am = rmin(rmin(phiv[0] - cSf[0], phiv[1] - cSf[1]), 0.0);    // :133-137
    double aPos = ap / (ap - am);                                             // :139
    double amaxSf = rmax(fabs(am), fabs(ap));                                 // :141
    double aSf = am * aPos;                                                   // :143
    if (TADMOR) { aSf = -0.5 * amaxSf; aPos = 0.5; }                          // :145-149
    const double aNeg = 1.0 - aPos;                                           // :151
    phiv[0] = phiv[0] * aPos;                                                 // :153-154
    phiv[1] = phiv[1] * aNeg;
    const double fp = phiv[0] - aSf, fn = phiv[1] + aSf;                      // :156-157 aphiv_pos, aphiv_neg
    amaxSf = rmax(fabs(fp), fabs(fn));                                        // :161
    o.amaxSf = amaxSf;
    {
        const double x = fp * v.rho[0], y = fn * v.rho[1];                    // :171
        o.phi = x + y;
    }
    {
        const double x = aPos * p[0], y = aNeg * p[1], pf = x + y;            // :173-177
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double m = fp * v.rhoU[0][k], n = fn * v.rhoU[1][k], q = pf * s[k];
            o.phiUp[k] = (m + n) + q;
        }
    }
    {
        const double kp = 0.5 * if_dot(U[0], U[0]), kn = 0.5 * if_dot(U[1], U[1]);   // magSqr contracts as the dot product does (assumption)
        const double hp = v.rho[0] * (v.e[0] + kp) + p[0], hn = v.rho[1] * (v.e[1] + kn) + p[1];
        const double t1 = fp * hp, t2 = fn * hn, t3 = aSf * p[0], t4 = aSf * p[1];   // :179-185, added left to right
        o.phiEp = ((t1 + t2) + t3) - t4;
    }
    if (OPT) {
        o.aPos = aPos;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double x = aPos * U[0][k], y = aNeg * U[1][k]; o.aU[k] = x + y; }
    }
}
template <bool OPT>
__device__ __forceinline__ void cf_store(const CfOut& o, int f, const CfFlux& r)
{
    o.phi[f] = r.phi; o.phiEp[f] = r.phiEp; o.amaxSf[f] = r.amaxSf;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.phiUp[k][f] = r.phiUp[k];
    if (OPT) {
        o.aPos[f] = r.aPos;
#pragma unroll
        for (int k = 0; k < 3; ++k) o.aU[k][f] = r.aU[k];
    }
}

// The kernel's own argument block, read where it is used.  Some sixty pointers and the three slots' coefficients are twice what the scalar
// registers hold: loaded once and held across the pass they would be spilled.  The argument block is the start of the kernarg segment
// (constant memory, scalar loads); the empty asm keeps the compiler from moving its loads out of the face loop.
__device__ __forceinline__ const CfArgs& cf_args()
{
    typedef const CfArgs __attribute__((address_space(4))) * K;
    K q = (K)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return *(const CfArgs*)q;
}

// the internal faces: XCD-aware chunks as k_limited_weights; cdw, Sf and magSf streamed, the cell fields, their gradients and C gathered
template <bool TADMOR, bool OPT>
__global__ __launch_bounds__(256) void k_central_flux(const CfArgs args)
{
    int f0, f1; block_chunk(args.nf, args.xcd, f0, f1);
    for (int f = f0 + threadIdx.x; f < f1; f += blockDim.x) {
        const CfArgs& a = cf_args();
        const int P = a.lo[f], N = a.up[f];
        const double cdw = a.cdw[f];
        const double dx = a.cc[0][N] - a.cc[0][P], dy = a.cc[1][N] - a.cc[1][P], dz = a.cc[2][N] - a.cc[2][P];
        CfFace v;
        cf_reconstruct<false>(a, cdw, a.own, P, a.own, N, dx, dy, dz, v);
        const double s[3] = {a.sf[0][f], a.sf[1][f], a.sf[2][f]};
        CfFlux r;
        cf_flux<TADMOR, OPT>(v, s, a.magSf[f], r);
        cf_store<OPT>(a.o, f, r);
    }
}
// one patch, one thread per face.  cdw given: a COUPLED patch (LimitedScheme.C:145-195, surfaceInterpolationScheme.C:361-366), the owner
// side through faceCells, the other side the patchNeighbourFields, d the patch delta.  cdw NULL: own holds the boundary values, which are
// the face values of both directions (surfaceInterpolationScheme.C:261-264); nothing of the algebra is simplified
template <bool TADMOR, bool OPT>
__global__ __launch_bounds__(256) void k_patch_central_flux(const CfArgs args)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= args.nf) return;
    const CfArgs& a = cf_args();
    CfFace v;
    if (a.cdw) cf_reconstruct<true>(a, a.cdw[i], a.own, a.lo[i], a.nbr, i, a.cc[0][i], a.cc[1][i], a.cc[2][i], v);
    else {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            v.rho[d] = a.own.rho[i]; v.rPsi[d] = a.own.rPsi[i]; v.e[d] = a.own.e[i]; v.c[d] = a.own.c[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) v.rhoU[d][k] = a.own.rhoU[k][i];
        }
    }
    const double s[3] = {a.sf[0][i], a.sf[1][i], a.sf[2][i]};
    CfFlux r;
    cf_flux<TADMOR, OPT>(v, s, a.magSf[i], r);
    cf_store<OPT>(a.o, i, r);
}

// rPsi = 1.0/psi; c = sqrt((Cp/Cv)*rPsi): in = {Cp, Cv, psi}, out = {rPsi, c}
__global__ __launch_bounds__(256) void k_central_sound_speed(const KeCell a)
{
    ke_map<3, 2>(a, [](const double (&x)[3], double (&o)[2]) {
        const double r = 1.0 / x[2], g = x[0] / x[1];
        o[0] = r;
        o[1] = sqrt(g * r);
    });
}

// compressibleCourantNo.H:35-47.  The sum: k_reduce<RED_SUM>'s chunks, accumulators and block sum over deltaCoeffs*amaxSf formed on load,
// so the partials are those of mi_sum over the stored product.  The max of (deltaCoeffs*amaxSf)/magSf over the internal faces of the
// block's chunk and its share of the boundary faces goes to pmax: k_min_max_final's tree ends it
__global__ __launch_bounds__(RB) void k_central_courant(const double* __restrict__ dc, const double* __restrict__ magSf, const double* __restrict__ amax, int64_t n,
                                                        const double* __restrict__ bdc, const double* __restrict__ bMagSf, const double* __restrict__ bAmax,
                                                        int64_t nb, double* __restrict__ psum, double* __restrict__ pmax)
{
    __shared__ double red[RB / 64];
    double acc0 = 0, acc1 = 0, hi = -INFINITY;
    auto take = [&](double v) { hi = (v > hi) ? v : hi; };
    chunk_loop(n, [&](int64_t i) { const double2 d = ld2(dc, i), x = ld2(amax, i), m = ld2(magSf, i);
          const double p = d.x * x.x, q = d.y * x.y;
          acc0 += p; acc1 += q; take(p / m.x); take(q / m.y); },
        [&](int64_t i) { const double p = dc[i] * amax[i]; acc0 += p; take(p / magSf[i]); });
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (int64_t)gridDim.x * blockDim.x) {
        const double p = bdc[i] * bAmax[i];
        take(p / bMagSf[i]);
    }
    const double t = block_sum<RB>(acc0 + acc1, red);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const double h = __shfl_xor(hi, m, 64); hi = (h > hi) ? h : hi; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < RB / 64; ++w) hi = (red[w] > hi) ? red[w] : hi;
        psum[blockIdx.x] = t;
        pmax[blockIdx.x] = hi;
    }
}

} // namespace mi

namespace {
// what mi_central_scheme_parse refuses, on a caller-filled scheme too; fills the three slots
int cf_scheme_check(const std::string& who, const mi_central_scheme* s, mi::CfSlot (&slot)[3])
{
    if (!s) return fail(MI_ERR_ARG, who + ": the scheme is missing");
    if (s->flux_scheme != MI_CENTRAL_KURGANOV && s->flux_scheme != MI_CENTRAL_TADMOR) return fail(MI_ERR_ARG, who + ": invalid mi_central_scheme: unknown flux scheme");
    const mi_limiter* l[3] = {&s->rho, &s->U, &s->T};
    const char* name[3] = {"reconstruct(rho)", "reconstruct(U)", "reconstruct(T)"};
    for (int j = 0; j < 3; ++j) {
        if (lim_check(who.c_str(), l[j], slot[j].k) != MI_OK) return fail(MI_ERR_ARG, who + ": invalid mi_central_scheme: " + name[j] + ": " + mi_last_error());
        if (j != 1 && l[j]->vector_form) return fail(MI_ERR_ARG, who + ": invalid mi_central_scheme: " + name[j] + " limits a scalar field: a V scheme is refused");
        slot[j].kind = l[j]->kind; slot[j].vec = l[j]->vector_form;
    }
    return MI_OK;
}
void cf_cells(const mi_central_cells* x, mi::CfCells& q)
{
    q.rho = x->rho_dev; q.rPsi = x->rpsi_dev; q.e = x->e_dev; q.c = x->c_dev; q.limU = x->lim_u_dev;
    for (int k = 0; k < 3; ++k) {
        q.rhoU[k] = x->rhou_dev[k]; q.gRho[k] = x->grad_rho_dev[k]; q.gRPsi[k] = x->grad_rpsi_dev[k]; q.gE[k] = x->grad_e_dev[k]; q.gC[k] = x->grad_c_dev[k];
        q.gLimU[k] = x->grad_lim_u_dev[k];
    }
    for (int k = 0; k < 9; ++k) q.gRhoU[k] = x->grad_rhou_dev[k];
}
// the arrays one side must hold: the seven values, and with grads the gradients the U slot reads
int cf_collect(const std::string& who, const mi::CfCells& q, bool grads, bool vecU, const double** in, int& n)
{
    in[n++] = q.rho; in[n++] = q.rPsi; in[n++] = q.e; in[n++] = q.c;
    for (int k = 0; k < 3; ++k) in[n++] = q.rhoU[k];
    if (!grads) return MI_OK;
    for (int k = 0; k < 3; ++k) { in[n++] = q.gRho[k]; in[n++] = q.gRPsi[k]; in[n++] = q.gE[k]; in[n++] = q.gC[k]; }
    if (vecU) for (int k = 0; k < 9; ++k) in[n++] = q.gRhoU[k];
    else {
        if (!q.limU || !q.gLimU[0] || !q.gLimU[1] || !q.gLimU[2])
            return fail(MI_ERR_ARG, who + ": a scalar reconstruct(U) is limited on magSqr(rhoU): lim_u and its gradient are missing");
        in[n++] = q.limU;
        for (int k = 0; k < 3; ++k) in[n++] = q.gLimU[k];
    }
    return MI_OK;
}
// the outputs: six, or ten with a_pos and aU (all or none)
int cf_outputs(const std::string& who, const mi_central_out* o, mi::CfOut& q, double** out, int& nOut, bool& opt)
{
    const int given = (o->a_pos_out_dev ? 1 : 0) + (o->au_out_dev[0] ? 1 : 0) + (o->au_out_dev[1] ? 1 : 0) + (o->au_out_dev[2] ? 1 : 0);
    if (given != 0 && given != 4) return fail(MI_ERR_ARG, who + ": a_pos_out and the three au_out come together or not at all");
    opt = given == 4;
    q.phi = o->phi_out_dev; q.phiEp = o->phiep_out_dev; q.amaxSf = o->amaxsf_out_dev; q.aPos = o->a_pos_out_dev;
    for (int k = 0; k < 3; ++k) { q.phiUp[k] = o->phiup_out_dev[k]; q.aU[k] = o->au_out_dev[k]; }
    nOut = 0;
    out[nOut++] = q.phi; out[nOut++] = q.phiEp; out[nOut++] = q.amaxSf;
    for (int k = 0; k < 3; ++k) out[nOut++] = q.phiUp[k];
    if (opt) { out[nOut++] = q.aPos; for (int k = 0; k < 3; ++k) out[nOut++] = q.aU[k]; }
    return MI_OK;
}
using CfKernel = void (*)(const mi::CfArgs);
CfKernel cf_kernel(bool patch, bool tadmor, bool opt)
{
    if (patch) return tadmor ? (opt ? k_patch_central_flux<true, true> : k_patch_central_flux<true, false>) : (opt ? k_patch_central_flux<false, true> : k_patch_central_flux<false, false>);
    return tadmor ? (opt ? k_central_flux<true, true> : k_central_flux<true, false>) : (opt ? k_central_flux<false, true> : k_central_flux<false, false>);
}
} // namespace

extern "C" int mi_central_scheme_parse(const char* flux_scheme, const char* reconstruct_rho, const char* reconstruct_U, const char* reconstruct_T,
                                       mi_central_scheme* out)
{
    const std::string who = "mi_central_scheme_parse";
    if (!flux_scheme || !reconstruct_rho || !reconstruct_U || !reconstruct_T || !out) return fail(MI_ERR_ARG, who + ": bad argument");
    mi_central_scheme s{};
    const std::vector<std::string> tok = scheme_words(flux_scheme);
    if (tok.size() == 1 && tok[0] == "Kurganov") s.flux_scheme = MI_CENTRAL_KURGANOV;
    else if (tok.size() == 1 && tok[0] == "Tadmor") s.flux_scheme = MI_CENTRAL_TADMOR;
    else return fail(MI_ERR_ARG, who + ": fluxScheme '" + flux_scheme + "' is not a valid choice. Options are: Tadmor, Kurganov");   // readFluxScheme.H
    const char* text[3] = {reconstruct_rho, reconstruct_U, reconstruct_T};
    mi_limiter* l[3] = {&s.rho, &s.U, &s.T};
    const char* name[3] = {"reconstruct(rho)", "reconstruct(U)", "reconstruct(T)"};
    for (int j = 0; j < 3; ++j)
        if (mi_limiter_parse(text[j], l[j]) != MI_OK) return fail(MI_ERR_ARG, who + ": " + name[j] + ": " + mi_last_error());
    mi::CfSlot slot[3];
    MICHK(cf_scheme_check(who, &s, slot));
    *out = s;
    return MI_OK;
}

extern "C" int mi_central_flux(mi_addr_t a, const mi_central_scheme* scheme, const double* cd_weights_dev, const double* const* sf_dev, const double* mag_sf_dev,
                               const mi_central_cells* cells, const double* const* c_dev, const mi_central_out* out)
{
    const std::string who = "mi_central_flux";
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    mi::CfSlot slot[3];
    MICHK(cf_scheme_check(who, scheme, slot));
    if (!out) return fail(MI_ERR_ARG, who + ": output arrays missing");
    CfArgs q{};
    double* o[10];
    int nOut = 0;
    bool opt = false;
    MICHK(cf_outputs(who, out, q.o, o, nOut, opt));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nFaces == 0) return MI_OK;
    if (!cells || !sf_dev || !c_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    cf_cells(cells, q.own);
    const double* in[48];
    int nIn = 0;
    in[nIn++] = q.cdw = cd_weights_dev; in[nIn++] = q.magSf = mag_sf_dev;
    for (int k = 0; k < 3; ++k) in[nIn++] = q.sf[k] = sf_dev[k];
    const int nFace = nIn;
    for (int k = 0; k < 3; ++k) in[nIn++] = q.cc[k] = c_dev[k];
    MICHK(cf_collect(who, q.own, true, slot[1].vec != 0, in, nIn));
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, o, nOut));
    bool ok = true;
    for (int i = 0; i < nFace; ++i) ok = ok && al16(in[i]);
    for (int i = nFace; i < nIn; ++i) ok = ok && al8(in[i]);
    for (int i = 0; i < nOut; ++i) ok = ok && al16(o[i]);
    if (!ok) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned, the cell fields to 8 bytes");
    q.lo = a->lowerAddr.p; q.up = a->upperAddr.p; q.sRho = slot[0]; q.sU = slot[1]; q.sT = slot[2];
    q.nf = a->L.nFaces; q.xcd = a->ctx->xcdRows;
    cf_kernel(false, scheme->flux_scheme == MI_CENTRAL_TADMOR, opt)<<<grid_for(a->ctx, a->L.nFaces), 256, 0, a->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_patch_central_flux(mi_patch_t p, const mi_central_scheme* scheme, const double* patch_weights_dev_or_null, const double* const* patch_sf_dev,
                                     const double* patch_mag_sf_dev, const mi_central_cells* values, const mi_central_cells* nbr_or_null,
                                     const double* const* patch_delta_dev_or_null, const mi_central_out* out)
{
    const std::string who = "mi_patch_central_flux";
    if (!p) return fail(MI_ERR_ARG, who + ": bad argument");
    mi::CfSlot slot[3];
    MICHK(cf_scheme_check(who, scheme, slot));
    if (!out) return fail(MI_ERR_ARG, who + ": output arrays missing");
    CfArgs q{};
    double* o[10];
    int nOut = 0;
    bool opt = false;
    MICHK(cf_outputs(who, out, q.o, o, nOut, opt));
    if (p->nFaces == 0) return MI_OK;
    const bool coupled = patch_weights_dev_or_null != nullptr;
    if (!values || !patch_sf_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    if (coupled && (!nbr_or_null || !patch_delta_dev_or_null)) return fail(MI_ERR_ARG, who + ": a coupled patch needs the patchNeighbourFields and the patch delta: input arrays missing");
    cf_cells(values, q.own);
    const double* in[96];
    int nIn = 0;
    in[nIn++] = q.magSf = patch_mag_sf_dev;
    for (int k = 0; k < 3; ++k) in[nIn++] = q.sf[k] = patch_sf_dev[k];
    MICHK(cf_collect(who, q.own, coupled, slot[1].vec != 0, in, nIn));
    if (coupled) {
        cf_cells(nbr_or_null, q.nbr);
        in[nIn++] = q.cdw = patch_weights_dev_or_null;
        for (int k = 0; k < 3; ++k) in[nIn++] = q.cc[k] = patch_delta_dev_or_null[k];
        MICHK(cf_collect(who, q.nbr, true, slot[1].vec != 0, in, nIn));
    }
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, o, nOut));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)o, nOut));
    HIPCHK(hipSetDevice(p->ctx->device));
    q.lo = p->faceCells.p; q.sRho = slot[0]; q.sU = slot[1]; q.sT = slot[2]; q.nf = p->nFaces;
    cf_kernel(true, scheme->flux_scheme == MI_CENTRAL_TADMOR, opt)<<<(p->nFaces + 255) / 256, 256, 0, p->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_central_sound_speed(mi_ctx_t c, int64_t n, const double* cp_dev, const double* cv_dev, const double* psi_dev, double* rpsi_out_dev,
                                      double* c_out_dev)
{
    KeCell q{};
    const double* in[3] = {cp_dev, cv_dev, psi_dev};
    double* out[2] = {rpsi_out_dev, c_out_dev};
    return ke_cell_pass("mi_central_sound_speed", c, n, k_central_sound_speed, q, in, 3, out, 2);
}

extern "C" int mi_central_courant(mi_addr_t a, const double* delta_coeffs_dev, const double* mag_sf_dev, const double* amaxsf_dev, int64_t n_boundary,
                                  const double* b_delta_coeffs_dev, const double* b_mag_sf_dev, const double* b_amaxsf_dev, double* max_out_host,
                                  double* sum_out_host)
{
    const std::string who = "mi_central_courant";
    if (!a || n_boundary < 0 || !max_out_host || !sum_out_host) return fail(MI_ERR_ARG, who + ": bad argument");
    mi_ctx_s* c = a->ctx;
    const int64_t n = a->L.nFaces;
    if (n == 0) { *max_out_host = 0.0; *sum_out_host = 0.0; return MI_OK; }   // if (mesh.nInternalFaces())
    const double* in[6] = {delta_coeffs_dev, mag_sf_dev, amaxsf_dev, b_delta_coeffs_dev, b_mag_sf_dev, b_amaxsf_dev};
    MICHK(arrays_present(who, in, n_boundary > 0 ? 6 : 3));
    if (!al16(delta_coeffs_dev) || !al16(mag_sf_dev) || !al16(amaxsf_dev)) return fail(MI_ERR_ARG, who + ": face fields must be 16-byte aligned");
    MICHK(arrays_aligned8(who, (const void* const*)in, 6));
    if (c->session) return fail(MI_ERR_STATE, who + ": a PCG session (mi_pcg_begin) is active on this context and owns its reduction scratch; call mi_pcg_end first");
    HIPCHK(hipSetDevice(c->device));
    double* P = c->partial.p;
    k_central_courant<<<RG, RB, 0, c->stream>>>(delta_coeffs_dev, mag_sf_dev, amaxsf_dev, n, b_delta_coeffs_dev, b_mag_sf_dev, b_amaxsf_dev, n_boundary, P, P + RG);
    k_reduce_final<<<1, RB, 0, c->stream>>>(P, c->scalars.p);
    k_min_max_final<<<1, 256, 0, c->stream>>>(P + RG, P + RG, RG, c->scalars.p + 1);   // the largest of the partial maxima lands in scalars[2]
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->hostScal, c->scalars.p, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *sum_out_host = c->hostScal[0];
    *max_out_host = c->hostScal[2];
    return MI_OK;
}
