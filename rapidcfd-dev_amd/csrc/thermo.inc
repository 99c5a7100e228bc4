// thermo.inc -- hePsiThermo / heRhoThermo ::calculate() for one pure mixture: T from he by Newton's iteration, then psi, mu, alpha and rho
// (thermophysicalModels/basic/psiThermo/hePsiThermo.C:31-171, rhoThermo/heRhoThermo.C:31-177, heThermo/heThermo.C:131-145;
// specie/thermo/thermo/thermoI.H:42-90 and the members below it; hConst/hConstThermoI.H:93-140, eConst/eConstThermoI.H:94-143,
// janaf/janafThermoI.H:58-71, :119-141, :188-241; equationOfState/perfectGas/perfectGasI.H:80-106; transport/const/constTransportI.H:98-128,
// sutherland/sutherlandTransportI.H:133-164; included by engine.hip after turbulence.inc; DESIGN 3.5q).
//
//   cells      mi_thermo_calculate: one streaming pass, 24 bytes in and 32 (40 with rho) out per cell
//   boundary   mi_thermo_calculate_boundary: every patch in one launch, the branch chosen per run of patches of one kind
// The model travels by value in the kernel arguments; janaf's two coefficient sets and the boundary pass's run table are staged in LDS once per
// workgroup, so that no instantiation spills a scalar register (profiles/thermo.md).
//   he         mi_thermo_he: he = HE(p, T), heThermo::init
//   property   mi_thermo_property: Cp, Cv, gamma, Cpv, CpByCpv or kappa
// Nothing here calls a transcendental function: + - * /, sqrt, min / max and comparisons only, so every result is the reference's bit for bit
// given the contraction below.  Everything is rounded operation by operation (-ffp-contract=off); every fma is written:
//   janaf cp   8314.4621*fma(fma(fma(fma(a4, T, a3), T, a2), T, a1), T, a0)
//   janaf hs   fma(8314.4621, fma(fma(fma(fma(fma(a4/5.0, T, a3/4.0), T, a2/3.0), T, a1/2.0), T, a0), T, a5), -hc), hc the same chain of the low
//              set at 298.15 times 8314.4621, rounded (formed once by mi_thermo_model_init, as are the four quotients of each set)
//   es         hConst: fma(Cp_, T, -q), eConst: fma(Cv_ + cpMcv, T, -q), q = (p*W)/rho(p, T); janaf: hs - q (hs ends in an fma already)
//   janaf cv   fma(8314.4621, chain of cp, -cpMcv) wherever Cv is formed (the Newton divisor of the internal energy, sutherland's Cv_, the Cv /
//              Cpv / kappa properties): cp's product has that one use; NOT in gamma = cp/(cp - cpMcv), where cp is used twice and stays rounded
// and NO fma in Cv_ + cpMcv, in 1.32 + (1.77*R)/Cv_ or in the Newton update, where a division stands between product and sum.  This is what
// the x86 compiler's contraction makes of the reference's expressions, taken for nvcc's: an ASSUMPTION (DESIGN 3.5q).
// min / max are doubleFloat.H's, mag is fabs.  Restated in tests/thermo_support.py, not pinned by a compiled reference.
namespace mi {

constexpr double TH_RR = 8314.4621;                   // specie::RR and perfectGas::cpMcv

// what the device functions see of a model: the struct in the kernel arguments (read with scalar loads where it is used) and, for janaf, the two
// coefficient sets in LDS -- per set a0..a5, then a1/2.0, a2/3.0, a3/4.0, a4/5.0 -- so that a lane picks its set with an address, not with
// twenty-two scalar registers held across the Newton loop
constexpr int TH_SET = 10;
struct ThM {
    const mi_thermo_model& m;
    const double* tab;                                // [2][TH_SET]: the low set, the high set; unused by hConst / eConst
};
template <int TH>
__device__ __forceinline__ void th_stage(const mi_thermo_model& m, double* tab)
{
    if constexpr (TH == MI_THERMO_JANAF) {
#pragma unroll
        for (int k = 0; k < 6; ++k) if (threadIdx.x == k) { tab[k] = m.lowCpCoeffs[k]; tab[TH_SET + k] = m.highCpCoeffs[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (threadIdx.x == 6 + k) { tab[6 + k] = m.lowH[k]; tab[TH_SET + 6 + k] = m.highH[k]; }
        __syncthreads();
    }
}
// janaf's coefficient set is chosen by T < Tcommon at every evaluation (a NaN takes the high set)
__device__ __forceinline__ const double* th_set(const ThM& x, double T) { return x.tab + (T < x.m.Tcommon ? 0 : TH_SET); }

__device__ __forceinline__ double th_rho(const ThM& x, double p, double T) { return p / (x.m.R * T); }
__device__ __forceinline__ double th_psi(const ThM& x, double T) { return 1.0 / (x.m.R * T); }

// janaf's Horner chain of cp without its factor 8314.4621
__device__ __forceinline__ double th_cp_chain(const ThM& x, double T)
{
    const double* a = th_set(x, T);
    return fma(fma(fma(fma(a[4], T, a[3]), T, a[2]), T, a[1]), T, a[0]);
}
// cp of the thermodynamics [J/(kmol K)], rounded: what Cp, gamma and hConst's / eConst's hs meet
template <int TH>
__device__ __forceinline__ double th_cp(const ThM& x, double T)
{
    if constexpr (TH == MI_THERMO_HCONST) return x.m.CpW;
    else if constexpr (TH == MI_THERMO_ECONST) return x.m.cpE;
    else return TH_RR * th_cp_chain(x, T);
}
// cv = cp - cpMcv [J/(kmol K)] as Cv meets it: janaf's product 8314.4621*chain has this one use and contracts with the subtraction
template <int TH>
__device__ __forceinline__ double th_cv(const ThM& x, double T)
{
    if constexpr (TH == MI_THERMO_JANAF) return fma(TH_RR, th_cp_chain(x, T), -x.m.cpMcv);
    else return th_cp<TH>(x, T) - x.m.cpMcv;
}
// hs - q: q is (p*W)/rho for the internal energy (ES), not looked at for the enthalpy
template <int TH, bool ES>
__device__ __forceinline__ double th_hs_minus(const ThM& x, double T, double q)
{
    if constexpr (TH == MI_THERMO_JANAF) {
        const double* a = th_set(x, T);
        const double hs = fma(TH_RR, fma(fma(fma(fma(fma(a[9], T, a[8]), T, a[7]), T, a[6]), T, a[0]), T, a[5]), -x.m.hc);
        return ES ? hs - q : hs;
    } else {
        const double cp = th_cp<TH>(x, T);
        return ES ? fma(cp, T, -q) : cp * T;
    }
}
// HE(p, T) [J/kg]: Hs = hs/W, Es = (hs - (p*W)/rho(p, T))/W
template <int E, int TH>
__device__ __forceinline__ double th_he(const ThM& x, double p, double T)
{
    if constexpr (E == MI_THERMO_ENTHALPY) return th_hs_minus<TH, false>(x, T, 0.0) / x.m.W;
    else return th_hs_minus<TH, true>(x, T, (p * x.m.W) / th_rho(x, p, T)) / x.m.W;
}
// Cpv(p, T) [J/(kg K)]: Cp = cp/W, Cv = cv/W
template <int E, int TH>
__device__ __forceinline__ double th_cpv(const ThM& x, double T)
{
    return (E == MI_THERMO_ENTHALPY ? th_cp<TH>(x, T) : th_cv<TH>(x, T)) / x.m.W;
}
template <int TH>
__device__ __forceinline__ double th_limit(const ThM& x, double T)
{
    if constexpr (TH == MI_THERMO_JANAF) {
        if (T < x.m.Tlow || T > x.m.Thigh) { const double a = (T > x.m.Tlow) ? T : x.m.Tlow; return (a < x.m.Thigh) ? a : x.m.Thigh; }
    }
    return T;
}
// thermo::T (thermoI.H:42-90): the 102nd evaluation returns NaN as the reference's device branch does; evals counts the evaluations
template <int E, int TH>
__device__ __forceinline__ double th_the(const ThM& x, double f, double p, double T0, int& evals)
{
    double Test = T0, Tnew = T0;
    const double Ttol = T0 * 1.0e-4;
    int iter = 0;
    do {
        Test = Tnew;
        Tnew = th_limit<TH>(x, Test - (th_he<E, TH>(x, p, Test) - f) / th_cpv<E, TH>(x, Test));
        if (iter++ > 100) { Tnew = __builtin_nan(""); break; }
    } while (fabs(Tnew - Test) > Ttol);
    evals = iter;
    return Tnew;
}
// the transport's mu(p, T) and kappa(p, T) (constTransportI.H:98-117, sutherlandTransportI.H:133-152)
template <int TR>
__device__ __forceinline__ double th_mu(const ThM& x, double T)
{
    if constexpr (TR == MI_THERMO_CONST) return x.m.mu;
    else return (x.m.As * sqrt(T)) / (1.0 + x.m.Ts / T);
}
template <int E, int TH, int TR>
__device__ __forceinline__ double th_kappa(const ThM& x, double T, double mu)
{
    if constexpr (TR == MI_THERMO_CONST) return (th_cpv<E, TH>(x, T) * mu) * x.m.rPr;
    else { const double Cv_ = th_cv<TH>(x, T) / x.m.W; return (mu * Cv_) * (1.32 + (1.77 * x.m.R) / Cv_); }
}
// mu and alphah of the transport at (p, T)
template <int E, int TH, int TR>
__device__ __forceinline__ void th_transport(const ThM& x, double T, double& mu, double& alpha)
{
    mu = th_mu<TR>(x, T);
    if constexpr (TR == MI_THERMO_CONST) alpha = mu * x.m.rPr;
    else alpha = th_kappa<E, TH, TR>(x, T, mu) / th_cpv<E, TH>(x, T);
}
__device__ __forceinline__ double th_rho_out(const ThM& x, int form, double p, double T, double psi)
{
    return form == 1 ? th_rho(x, p, T) : psi * p;
}

struct ThCell {
    const double *he, *p, *t0;
    double *t, *psi, *mu, *alpha, *rho;
    int32_t* iters;
    int64_t n;
    int vec, rhoForm;
    mi_thermo_model m;
};
template <int E, int TH, int TR>
__device__ __forceinline__ void th_cell(const ThM& x, int rhoForm, double he, double p, double t0, double (&o)[5], int& evals)
{
    const double T = th_the<E, TH>(x, he, p, t0, evals);
    o[0] = T; o[1] = th_psi(x, T);
    th_transport<E, TH, TR>(x, T, o[2], o[3]);
    o[4] = rhoForm ? th_rho_out(x, rhoForm, p, T, o[1]) : 0.0;
}
// the cell pass: a thread takes two cells with 16-byte accesses when every array allows it, the odd last cell and every cell of a
// not-so-aligned call one by one.  Every load of a cell precedes its stores, so t may be t0 or he.
template <int E, int TH, int TR>
__global__ __launch_bounds__(256) void k_thermo_calculate(const ThCell a)
{
    __shared__ double tab[2 * TH_SET];
    th_stage<TH>(a.m, tab);
    const ThM x{a.m, tab};
    const int64_t n = a.n, np = a.vec ? n >> 1 : 0, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = t; q < np; q += stride) {
        const int64_t i = 2 * q;
        const double2 he = ld2(a.he, i), p = ld2(a.p, i), t0 = ld2(a.t0, i);
        double u[5], v[5];
        int eu, ev;
        th_cell<E, TH, TR>(x, a.rhoForm, he.x, p.x, t0.x, u, eu);
        th_cell<E, TH, TR>(x, a.rhoForm, he.y, p.y, t0.y, v, ev);
        st2(a.t, i, make_double2(u[0], v[0])); st2(a.psi, i, make_double2(u[1], v[1]));
        st2(a.mu, i, make_double2(u[2], v[2])); st2(a.alpha, i, make_double2(u[3], v[3]));
        if (a.rhoForm) st2(a.rho, i, make_double2(u[4], v[4]));
        if (a.iters) { a.iters[i] = eu; a.iters[i + 1] = ev; }
    }
    for (int64_t i = 2 * np + t; i < n; i += stride) {
        const double he = a.he[i], p = a.p[i], t0 = a.t0[i];
        double u[5];
        int eu;
        th_cell<E, TH, TR>(x, a.rhoForm, he, p, t0, u, eu);
        a.t[i] = u[0]; a.psi[i] = u[1]; a.mu[i] = u[2]; a.alpha[i] = u[3];
        if (a.rhoForm) a.rho[i] = u[4];
        if (a.iters) a.iters[i] = eu;
    }
}

// the boundary pass: the patches of kind 1 and 2 as runs of consecutive faces, at most TH_RUNS runs a launch; one thread per face.  The run
// table travels in the kernel arguments and is staged in LDS, where a thread finds its run with a loop
constexpr int TH_RUNS = 16;
struct ThBoundary {
    double *he;                                       // read on kind 2, written on kind 1
    const double *p, *t;
    double *tOut, *psi, *mu, *alpha, *rho;
    int32_t first[TH_RUNS], face0[TH_RUNS], kind[TH_RUNS];   // per run: its first thread, its first boundary face, its kind
    int nRuns, total, rhoForm;
    mi_thermo_model m;
};
template <int E, int TH, int TR>
__global__ __launch_bounds__(256) void k_thermo_boundary(const ThBoundary a)
{
    __shared__ double tab[2 * TH_SET];
    __shared__ int32_t first[TH_RUNS], face0[TH_RUNS], kinds[TH_RUNS];
#pragma unroll
    for (int r = 0; r < TH_RUNS; ++r) if (threadIdx.x == r) { first[r] = a.first[r]; face0[r] = a.face0[r]; kinds[r] = a.kind[r]; }
    th_stage<TH>(a.m, tab);
    __syncthreads();
    const ThM x{a.m, tab};
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < a.total; j += gridDim.x * blockDim.x) {
        int run = 0;
        for (int r = 1; r < a.nRuns; ++r) if (j >= first[r]) run = r;
        const int bf = j - first[run] + face0[run], kind = kinds[run];
        const double p = a.p[bf];
        double T;
        if (kind == 1) {                              // fixesValue: he = HE(p, T), the properties at the given T
            T = a.t[bf];
            a.he[bf] = th_he<E, TH>(x, p, T);
        } else {                                      // T = THE(he, p, T), the properties at the new T
            int evals;
            T = th_the<E, TH>(x, a.he[bf], p, a.t[bf], evals);
            a.tOut[bf] = T;
        }
        const double psi = th_psi(x, T);
        double mu, alpha;
        th_transport<E, TH, TR>(x, T, mu, alpha);
        a.psi[bf] = psi; a.mu[bf] = mu; a.alpha[bf] = alpha;
        if (a.rhoForm) a.rho[bf] = th_rho_out(x, a.rhoForm, p, T, psi);
    }
}

// he = HE(p, T) and one property of (p, T): cell passes of ke_map's shape; the energy form, the transport and the kind are uniform branches
struct ThMap {
    KeCell c;
    int kind;
    mi_thermo_model m;
};
template <int TH>
__global__ __launch_bounds__(256) void k_thermo_he(const ThMap a)
{
    __shared__ double tab[2 * TH_SET];
    th_stage<TH>(a.m, tab);
    const ThM x{a.m, tab};
    if (a.m.energy == MI_THERMO_ENTHALPY)
        ke_map<2, 1>(a.c, [&](const double (&v)[2], double (&o)[1]) { o[0] = th_he<MI_THERMO_ENTHALPY, TH>(x, v[0], v[1]); });
    else
        ke_map<2, 1>(a.c, [&](const double (&v)[2], double (&o)[1]) { o[0] = th_he<MI_THERMO_INTERNAL_ENERGY, TH>(x, v[0], v[1]); });
}
// Cp = cp/W; Cv = cv/W; gamma = cp/(cp - cpMcv) with cp rounded (thermoI.H:148-149: the product has two uses there and stays a product);
// Cpv and CpByCpv by the energy form; kappa the TRANSPORT's kappa(p, T), not heThermo::kappa()
template <int TH>
__global__ __launch_bounds__(256) void k_thermo_property(const ThMap a)
{
    __shared__ double tab[2 * TH_SET];
    th_stage<TH>(a.m, tab);
    const ThM x{a.m, tab};
    const bool h = a.m.energy == MI_THERMO_ENTHALPY, constTr = a.m.transport == MI_THERMO_CONST;
    const int kind = a.kind;
    ke_map<2, 1>(a.c, [&](const double (&v)[2], double (&o)[1]) {
        const double T = v[1];
        double r;
        if (kind == MI_THERMO_CP || (kind == MI_THERMO_CPV && h)) r = th_cp<TH>(x, T) / x.m.W;
        else if (kind == MI_THERMO_CV || kind == MI_THERMO_CPV) r = th_cv<TH>(x, T) / x.m.W;
        else if (kind == MI_THERMO_GAMMA || (kind == MI_THERMO_CPBYCPV && !h)) { const double cp = th_cp<TH>(x, T); r = cp / (cp - x.m.cpMcv); }
        else if (kind == MI_THERMO_CPBYCPV) r = 1.0;
        else if (constTr) r = h ? th_kappa<MI_THERMO_ENTHALPY, TH, MI_THERMO_CONST>(x, T, x.m.mu) : th_kappa<MI_THERMO_INTERNAL_ENERGY, TH, MI_THERMO_CONST>(x, T, x.m.mu);
        else r = th_kappa<MI_THERMO_ENTHALPY, TH, MI_THERMO_SUTHERLAND>(x, T, th_mu<MI_THERMO_SUTHERLAND>(x, T));
        o[0] = r;
    });
}

} // namespace mi

namespace {
bool th_finite(double x) { return std::isfinite(x); }
bool th_positive(double x) { return std::isfinite(x) && x > 0; }
// what mi_thermo_model_init refuses, on a finished model too
int th_model_check(const std::string& who, const mi_thermo_model* m)
{
    if (!m) return fail(MI_ERR_ARG, who + ": the model is missing");
    if (m->energy != MI_THERMO_ENTHALPY && m->energy != MI_THERMO_INTERNAL_ENERGY) return fail(MI_ERR_ARG, who + ": unknown energy form");
    if (m->thermo != MI_THERMO_HCONST && m->thermo != MI_THERMO_ECONST && m->thermo != MI_THERMO_JANAF) return fail(MI_ERR_ARG, who + ": unknown thermodynamics");
    if (m->transport != MI_THERMO_CONST && m->transport != MI_THERMO_SUTHERLAND) return fail(MI_ERR_ARG, who + ": unknown transport");
    bool pos = th_positive(m->W) && th_positive(m->R) && th_positive(m->cpMcv), fin = true;
    if (m->thermo == MI_THERMO_HCONST) { pos = pos && th_positive(m->Cp) && th_positive(m->CpW); fin = th_finite(m->Hf) && th_finite(m->HfW); }
    else if (m->thermo == MI_THERMO_ECONST) { pos = pos && th_positive(m->Cv) && th_positive(m->CvW) && th_positive(m->cpE); fin = th_finite(m->Hf) && th_finite(m->HfW); }
    else {
        pos = pos && th_positive(m->Tlow) && th_positive(m->Thigh) && th_positive(m->Tcommon);
        for (int i = 0; i < 7; ++i) fin = fin && th_finite(m->highCpCoeffs[i]) && th_finite(m->lowCpCoeffs[i]);
        for (int i = 0; i < 4; ++i) fin = fin && th_finite(m->highH[i]) && th_finite(m->lowH[i]);
        fin = fin && th_finite(m->hc);
    }
    if (m->transport == MI_THERMO_CONST) pos = pos && th_positive(m->mu) && th_positive(m->Pr) && th_positive(m->rPr);
    else pos = pos && th_positive(m->As) && th_positive(m->Ts);
    if (!pos || !fin) return fail(MI_ERR_ARG, who + ": every member of the model must be finite, and all but Hf and the janaf coefficients above zero (mi_thermo_model_init)");
    if (m->thermo == MI_THERMO_JANAF) {               // janafThermo::checkInputData (janafThermo.C:31-53)
        if (m->Tlow >= m->Thigh) return fail(MI_ERR_ARG, who + ": janaf: Tlow >= Thigh");
        if (m->Tcommon <= m->Tlow) return fail(MI_ERR_ARG, who + ": janaf: Tcommon <= Tlow");
        if (m->Tcommon > m->Thigh) return fail(MI_ERR_ARG, who + ": janaf: Tcommon > Thigh");
    }
    return MI_OK;
}
bool th_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}
// every output clear of every input and of every other output; allowedA / allowedB: the output that may BE one of two inputs
int th_outputs_clear(const std::string& who, const void* const* in, int nIn, size_t inBytes, const void* const* out, const size_t* outBytes, int nOut,
                     const void* allowedOut, const void* allowedA, const void* allowedB)
{
    for (int o = 0; o < nOut; ++o) {
        for (int i = 0; i < nIn; ++i) {
            if (out[o] == allowedOut && out[o] == in[i] && (in[i] == allowedA || in[i] == allowedB)) continue;
            if (th_overlap(out[o], outBytes[o], in[i], inBytes)) return fail(MI_ERR_ARG, who + ": an output must not overlap an input (the temperature may be written over t0 or over he)");
        }
        for (int q = 0; q < o; ++q) if (th_overlap(out[o], outBytes[o], out[q], outBytes[q])) return fail(MI_ERR_ARG, who + ": the outputs must not overlap");
    }
    return MI_OK;
}
// the instantiation of a model's (energy form, thermodynamics, transport): the cell and the boundary kernel
struct ThKernels {
    void (*cell)(const mi::ThCell);
    void (*boundary)(const mi::ThBoundary);
};
using ThMapKernel = void (*)(const mi::ThMap);
template <int E, int TH>
ThKernels th_kernels(int tr)
{
    if (tr == MI_THERMO_CONST) return {k_thermo_calculate<E, TH, MI_THERMO_CONST>, k_thermo_boundary<E, TH, MI_THERMO_CONST>};
    return {k_thermo_calculate<E, TH, MI_THERMO_SUTHERLAND>, k_thermo_boundary<E, TH, MI_THERMO_SUTHERLAND>};
}
template <int E>
ThKernels th_kernels(int th, int tr)
{
    return th == MI_THERMO_HCONST ? th_kernels<E, MI_THERMO_HCONST>(tr) : th == MI_THERMO_ECONST ? th_kernels<E, MI_THERMO_ECONST>(tr) : th_kernels<E, MI_THERMO_JANAF>(tr);
}
ThKernels th_kernels(const mi_thermo_model* m)
{
    return m->energy == MI_THERMO_ENTHALPY ? th_kernels<MI_THERMO_ENTHALPY>(m->thermo, m->transport) : th_kernels<MI_THERMO_INTERNAL_ENERGY>(m->thermo, m->transport);
}
// the two-input, one-output passes: the checks of a kEpsilon cell pass, then the launch
int th_map_pass(const std::string& who, mi_ctx_s* c, const mi_thermo_model* m, int kind, int64_t n, const double* p, const double* T, double* out, bool he)
{
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(th_model_check(who, m));
    if (!he && (kind < MI_THERMO_CP || kind > MI_THERMO_KAPPA)) return fail(MI_ERR_ARG, who + ": unknown property kind");
    if (n > INT32_MAX) return fail(MI_ERR_ARG, who + ": too many elements");
    if (n == 0) return MI_OK;
    const double* in[2] = {p, T};
    double* o[1] = {out};
    MICHK(arrays_present(who, in, 2));
    if (!out) return fail(MI_ERR_ARG, who + ": output arrays missing");
    MICHK(arrays_aligned8(who, (const void* const*)in, 2));
    MICHK(arrays_aligned8(who, (const void* const*)o, 1));
    const size_t bytes = (size_t)n * sizeof(double);
    const void* outs[1] = {out};
    MICHK(th_outputs_clear(who, (const void* const*)in, 2, bytes, outs, &bytes, 1, nullptr, nullptr, nullptr));
    mi::ThMap q{};
    q.c.in[0] = p; q.c.in[1] = T; q.c.out[0] = out; q.c.n = n; q.c.vec = all_aligned16(in, 2, o, 1) ? 1 : 0;
    q.kind = kind; q.m = *m;
    ThMapKernel k = he ? (m->thermo == MI_THERMO_HCONST ? k_thermo_he<MI_THERMO_HCONST> : m->thermo == MI_THERMO_ECONST ? k_thermo_he<MI_THERMO_ECONST> : k_thermo_he<MI_THERMO_JANAF>)
                       : (m->thermo == MI_THERMO_HCONST ? k_thermo_property<MI_THERMO_HCONST> : m->thermo == MI_THERMO_ECONST ? k_thermo_property<MI_THERMO_ECONST> : k_thermo_property<MI_THERMO_JANAF>);
    HIPCHK(hipSetDevice(c->device));
    k<<<grid_for(c, (int)((n + 1) / 2)), 256, 0, c->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace

extern "C" int mi_thermo_model_init(int energy, int thermo, int transport, double W, const double* thermo_values, const double* transport_values,
                                    mi_thermo_model* out)
{
    const std::string who = "mi_thermo_model_init";
    if (!out || !thermo_values || !transport_values) return fail(MI_ERR_ARG, who + ": bad argument");
    mi_thermo_model m{};
    m.energy = energy; m.thermo = thermo; m.transport = transport;
    m.W = W; m.R = mi::TH_RR / W; m.cpMcv = mi::TH_RR;           // specieI.H:97-100, perfectGasI.H:104-106
    if (thermo == MI_THERMO_HCONST) {
        m.Cp = thermo_values[0]; m.Hf = thermo_values[1];
        m.CpW = m.Cp * W; m.HfW = m.Hf * W;                       // hConstThermo.C:40-41: Cp_ *= W, Hf_ *= W
    } else if (thermo == MI_THERMO_ECONST) {
        m.Cv = thermo_values[0]; m.Hf = thermo_values[1];
        m.CvW = m.Cv * W; m.HfW = m.Hf * W;                       // eConstThermo.C likewise
        m.cpE = m.CvW + m.cpMcv;                                  // eConstThermoI.H:111, no product: no fma
    } else if (thermo == MI_THERMO_JANAF) {                       // janafThermo.C:56-86 does not scale its coefficients
        m.Tlow = thermo_values[0]; m.Thigh = thermo_values[1]; m.Tcommon = thermo_values[2];
        for (int i = 0; i < 7; ++i) { m.highCpCoeffs[i] = thermo_values[3 + i]; m.lowCpCoeffs[i] = thermo_values[10 + i]; }
        const double d[4] = {2.0, 3.0, 4.0, 5.0};
        for (int i = 0; i < 4; ++i) { m.highH[i] = m.highCpCoeffs[1 + i] / d[i]; m.lowH[i] = m.lowCpCoeffs[1 + i] / d[i]; }
        const double Tstd = 298.15;                               // janafThermoI.H:230-241
        const double s = std::fma(std::fma(std::fma(std::fma(std::fma(m.lowH[3], Tstd, m.lowH[2]), Tstd, m.lowH[1]), Tstd, m.lowH[0]), Tstd, m.lowCpCoeffs[0]), Tstd,
                                  m.lowCpCoeffs[5]);
        m.hc = mi::TH_RR * s;
    }
    if (transport == MI_THERMO_CONST) { m.mu = transport_values[0]; m.Pr = transport_values[1]; m.rPr = 1.0 / m.Pr; }   // constTransport.C:47
    else if (transport == MI_THERMO_SUTHERLAND) { m.As = transport_values[0]; m.Ts = transport_values[1]; }
    MICHK(th_model_check(who, &m));
    *out = m;
    return MI_OK;
}

extern "C" int mi_thermo_calculate(mi_ctx_t c, const mi_thermo_model* model, int rho_form, int64_t n, const double* he_dev, const double* p_dev,
                                   const double* t0_dev, double* t_out_dev, double* psi_out_dev, double* mu_out_dev, double* alpha_out_dev,
                                   double* rho_out_dev_or_null, int32_t* iters_out_or_null)
{
    const std::string who = "mi_thermo_calculate";
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(th_model_check(who, model));
    if (rho_form < 0 || rho_form > 2) return fail(MI_ERR_ARG, who + ": unknown rho_form");
    if (n > INT32_MAX) return fail(MI_ERR_ARG, who + ": too many cells");
    if (n == 0) return MI_OK;
    if (rho_form != 0 && !rho_out_dev_or_null) return fail(MI_ERR_ARG, who + ": rho_form asks for rho: the rho array is missing");
    const double* in[3] = {he_dev, p_dev, t0_dev};
    double* out[5] = {t_out_dev, psi_out_dev, mu_out_dev, alpha_out_dev, rho_out_dev_or_null};
    const int nOut = rho_form ? 5 : 4;
    MICHK(arrays_present(who, in, 3));
    for (int o = 0; o < nOut; ++o) if (!out[o]) return fail(MI_ERR_ARG, who + ": output arrays missing");
    MICHK(arrays_aligned8(who, (const void* const*)in, 3));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    if ((reinterpret_cast<uintptr_t>(iters_out_or_null) & 3u) != 0) return fail(MI_ERR_ARG, who + ": the iteration counts must be aligned to 4 bytes");
    const size_t bytes = (size_t)n * sizeof(double);
    const void* outs[6] = {t_out_dev, psi_out_dev, mu_out_dev, alpha_out_dev, nullptr, nullptr};
    size_t outBytes[6] = {bytes, bytes, bytes, bytes, bytes, bytes};
    int m = 4;
    if (rho_form) outs[m++] = rho_out_dev_or_null;
    if (iters_out_or_null) { outs[m] = iters_out_or_null; outBytes[m++] = (size_t)n * sizeof(int32_t); }
    MICHK(th_outputs_clear(who, (const void* const*)in, 3, bytes, outs, outBytes, m, t_out_dev, t0_dev, he_dev));
    mi::ThCell q{};
    q.he = he_dev; q.p = p_dev; q.t0 = t0_dev; q.t = t_out_dev; q.psi = psi_out_dev; q.mu = mu_out_dev; q.alpha = alpha_out_dev;
    q.rho = rho_form ? rho_out_dev_or_null : nullptr; q.iters = iters_out_or_null;
    q.n = n; q.vec = all_aligned16(in, 3, out, nOut) ? 1 : 0; q.rhoForm = rho_form; q.m = *model;
    HIPCHK(hipSetDevice(c->device));
    th_kernels(model).cell<<<grid_for(c, (int)((n + 1) / 2)), 256, 0, c->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_thermo_calculate_boundary(mi_addr_t a, mi_grad_boundary_t b, const mi_thermo_model* model, const int32_t* patch_kind, int rho_form,
                                            double* b_he_inout_dev, const double* b_p_dev, const double* b_t_dev, double* b_t_out_dev,
                                            double* b_psi_out_dev, double* b_mu_out_dev, double* b_alpha_out_dev, double* b_rho_out_dev_or_null)
{
    const std::string who = "mi_thermo_calculate_boundary";
    if (!a || !b) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(boundary_matches(who, a, b));
    MICHK(th_model_check(who, model));
    if (rho_form < 0 || rho_form > 2) return fail(MI_ERR_ARG, who + ": unknown rho_form");
    const int32_t nP = (int32_t)b->patchSizes.size();
    if (nP > 0 && !patch_kind) return fail(MI_ERR_ARG, who + ": patch_kind is missing");
    // the runs: consecutive patches of one kind with faces, kind 0 left out
    std::vector<int32_t> face0, count, kind;
    {
        int32_t off = 0;
        for (int32_t p = 0; p < nP; ++p) {
            const int32_t k = patch_kind[p], sz = b->patchSizes[p];
            if (k < 0 || k > 2) return fail(MI_ERR_ARG, who + ": unknown patch kind on patch " + std::to_string(p));
            if (k != 0 && sz > 0) {
                if (!kind.empty() && kind.back() == k && face0.back() + count.back() == off) count.back() += sz;
                else { face0.push_back(off); count.push_back(sz); kind.push_back(k); }
            }
            off += sz;
        }
    }
    if (kind.empty()) return MI_OK;
    if (rho_form != 0 && !b_rho_out_dev_or_null) return fail(MI_ERR_ARG, who + ": rho_form asks for rho: the rho array is missing");
    const double* in[3] = {b_he_inout_dev, b_p_dev, b_t_dev};
    double* out[6] = {b_he_inout_dev, b_t_out_dev, b_psi_out_dev, b_mu_out_dev, b_alpha_out_dev, b_rho_out_dev_or_null};
    const int nOut = rho_form ? 6 : 5;
    if (!in[0] || !in[1] || !in[2]) return fail(MI_ERR_ARG, who + ": the boundary has faces on a patch of kind 1 or 2: boundary arrays needed");
    for (int o = 0; o < nOut; ++o) if (!out[o]) return fail(MI_ERR_ARG, who + ": the boundary has faces on a patch of kind 1 or 2: boundary arrays needed");
    MICHK(arrays_aligned8(who, (const void* const*)in, 3));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    const size_t bytes = (size_t)b->nFaces * sizeof(double);
    {   // he is read and written; the others: the temperature over b_t or over b_he, nothing else shared.  b_he as the kind-1 OUTPUT is
        // kept clear of psi, mu, alpha and rho by the second call, which tests them against b_he as an input
        const void* ins[2] = {b_p_dev, b_t_dev};
        const void* heOut[1] = {b_he_inout_dev};
        MICHK(th_outputs_clear(who, ins, 2, bytes, heOut, &bytes, 1, nullptr, nullptr, nullptr));
        const void* outs[5] = {b_t_out_dev, b_psi_out_dev, b_mu_out_dev, b_alpha_out_dev, b_rho_out_dev_or_null};
        const size_t outBytes[5] = {bytes, bytes, bytes, bytes, bytes};
        MICHK(th_outputs_clear(who, (const void* const*)in, 3, bytes, outs, outBytes, nOut - 1, b_t_out_dev, b_t_dev, b_he_inout_dev));
    }
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    const auto k = th_kernels(model).boundary;
    for (size_t r0 = 0; r0 < kind.size(); r0 += mi::TH_RUNS) {
        mi::ThBoundary q{};
        q.he = b_he_inout_dev; q.p = b_p_dev; q.t = b_t_dev; q.tOut = b_t_out_dev; q.psi = b_psi_out_dev; q.mu = b_mu_out_dev; q.alpha = b_alpha_out_dev;
        q.rho = rho_form ? b_rho_out_dev_or_null : nullptr; q.rhoForm = rho_form; q.m = *model;
        q.nRuns = (int)std::min<size_t>(mi::TH_RUNS, kind.size() - r0);
        int32_t total = 0;
        for (int r = 0; r < q.nRuns; ++r) { q.first[r] = total; q.face0[r] = face0[r0 + r]; q.kind[r] = kind[r0 + r]; total += count[r0 + r]; }
        q.total = total;
        k<<<grid_for(c, total), 256, 0, c->stream>>>(q);
        HIPCHK(hipGetLastError());
    }
    return MI_OK;
}

extern "C" int mi_thermo_he(mi_ctx_t c, const mi_thermo_model* model, int64_t n, const double* p_dev, const double* t_dev, double* he_out_dev)
{
    return th_map_pass("mi_thermo_he", c, model, 0, n, p_dev, t_dev, he_out_dev, true);
}

extern "C" int mi_thermo_property(mi_ctx_t c, const mi_thermo_model* model, int kind, int64_t n, const double* p_dev, const double* t_dev, double* out_dev)
{
    return th_map_pass("mi_thermo_property", c, model, kind, n, p_dev, t_dev, out_dev, false);
}
