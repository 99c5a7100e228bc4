// turbulence.inc -- incompressible::RASModels::kEpsilon with the epsilonWallFunction, nutkWallFunction and kqRWallFunction patches
// (turbulenceModels/incompressible/RAS/kEpsilon/kEpsilon.C:132-136, :229-280; epsilonWallFunctionFvPatchScalarField.C:116-396, :540-589;
// nutkWallFunctionFvPatchScalarField.C:60-77; cfdTools/general/bound/bound.C:32-60; fvc/fvcAverage.C:71-74; included by engine.hip after
// interface.inc; DESIGN 3.5o).
//
//   G          kEpsilon.C:238  (nut*2)*magSqr(symm(gradU)) in one cell pass over the nine arrays of a vector gradient
//   wall cells :241  epsilon.boundaryField().updateCoeffs() for ALL wall patches in one launch: one thread per unique wall cell walks its
//              wall faces in (patch, face) order -- the order in which the reference's per-patch matrixPatchOperation passes meet them --
//              from 0.0, writes G, epsilon and the zero-gradient boundary values; no atomics
//   sources    :250-251, :269 and DepsilonEff / DkEff (kEpsilon.H:123-137), one cell pass per equation
//   bound      bound.C:45-54 in one row pass that writes no face field: linearInterpolate(max(vsf, lb)) recomputed on both sides of a face
//   nut        :278 and nutkWallFunction::calcNut on every wall face in one launch
// A cell meets its faces in the order of 3.5k: own faces ascending, neighbour-side faces in losort order, boundary faces by patch then by
// face.  max is (a > b) ? a : b, pos(x) is (x >= 0) ? 1 : 0.  Everything is rounded operation by operation (-ffp-contract=off); every fma
// below is written.  Restated in tests/turbulence_support.py, not pinned by a compiled reference.
namespace mi {

struct KeCell {
    const double* in[10];
    double* out[3];
    int64_t n;
    int vec;
    double c1, c2, c3, nu;
};
// a streaming cell pass under the context's launch-grid cap over the first NIN inputs and NOUT outputs of a: f(x, o) sees one cell, as
// cell_map's; a thread takes two cells with 16-byte accesses when every array allows it (a.vec), the odd last cell and every cell of a
// not-so-aligned call one by one.  Every load of a cell precedes its stores, so a stream updated in place stands in both lists.
template <int NIN, int NOUT, class F>
__device__ __forceinline__ void ke_map(const KeCell& a, F f)
{
    const int64_t n = a.n, np = a.vec ? n >> 1 : 0, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = t; q < np; q += stride) {
        const int64_t i = 2 * q;
        double x[NIN], y[NIN], ox[NOUT], oy[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; ++k) { const double2 v = ld2(a.in[k], i); x[k] = v.x; y[k] = v.y; }
        f(x, ox); f(y, oy);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) st2(a.out[k], i, make_double2(ox[k], oy[k]));
    }
    for (int64_t i = 2 * np + t; i < n; i += stride) {
        double x[NIN], o[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; ++k) x[k] = a.in[k][i];
        f(x, o);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) a.out[k][i] = o[k];
    }
}

// G = (nut*2)*magSqr(symm(gradU)).  symm: 0.5*(a + b) off the diagonal.  magSqr: xx^2 + 2*xy^2 + 2*xz^2 + yy^2 + 2*yz^2 + zz^2 left to right
// with the three squares of the diagonal contracted into the running sum and the doubled squares rounded before they are added (2*q is
// exact, so fma(2, q, s) is s + 2*q): what LLVM's contraction makes of SymmTensorI.H:276-284 (an ASSUMPTION, DESIGN 3.5o)
__device__ __forceinline__ double ke_magsqr_symm(const double* g)   // g[3*j + k] = d(U_j)/dx_k
{
    const double xy = 0.5 * (g[1] + g[3]), xz = 0.5 * (g[2] + g[6]), yz = 0.5 * (g[5] + g[7]);
    const double qxy = xy * xy, qxz = xz * xz, qyz = yz * yz;
    double s = fma(g[0], g[0], 2.0 * qxy);
    s = fma(2.0, qxz, s);
    s = fma(g[4], g[4], s);
    s = fma(2.0, qyz, s);
    s = fma(g[8], g[8], s);
    return s;
}
__global__ __launch_bounds__(256) void k_ke_production(const KeCell a)
{
    ke_map<10, 1>(a, [](const double (&x)[10], double (&o)[1]) { o[0] = (x[0] * 2.0) * ke_magsqr_symm(x + 1); });
}
// su = ((C1*G)*eps)/k, sp = (C2*eps)/k, deps = nut/sigmaEps + nu   (c1 = C1, c2 = C2, c3 = sigmaEps)
template <bool NUF>
__global__ __launch_bounds__(256) void k_ke_epsilon_terms(const KeCell a)
{
    constexpr int NIN = NUF ? 5 : 4;
    const double C1 = a.c1, C2 = a.c2, sigmaEps = a.c3, nu0 = a.nu;
    ke_map<NIN, 3>(a, [=](const double (&x)[NIN], double (&o)[3]) {
        const double G = x[0], eps = x[1], k = x[2], nut = x[3], nu = NUF ? x[NIN - 1] : nu0;
        o[0] = ((C1 * G) * eps) / k;
        o[1] = (C2 * eps) / k;
        o[2] = nut / sigmaEps + nu;
    });
}
// sp = eps/k, dk = nut + nu
template <bool NUF>
__global__ __launch_bounds__(256) void k_ke_k_terms(const KeCell a)
{
    constexpr int NIN = NUF ? 4 : 3;
    const double nu0 = a.nu;
    ke_map<NIN, 2>(a, [=](const double (&x)[NIN], double (&o)[2]) {
        o[0] = x[0] / x[1];
        o[1] = x[2] + (NUF ? x[NIN - 1] : nu0);
    });
}
// nut = (Cmu*(k*k))/eps
__global__ __launch_bounds__(256) void k_ke_nut(const KeCell a)
{
    const double Cmu = a.c1;
    ke_map<2, 1>(a, [=](const double (&x)[2], double (&o)[1]) { o[0] = (Cmu * (x[0] * x[0])) / x[1]; });
}
// out = max(x, value); out may be x
__global__ __launch_bounds__(256) void k_vec_max_value(const KeCell a)
{
    const double v = a.c1;
    ke_map<1, 1>(a, [=](const double (&x)[1], double (&o)[1]) { o[0] = (x[0] > v) ? x[0] : v; });
}

// the smallest and the largest value: per-block partials, then one block over them
__device__ __forceinline__ void ke_block_min_max(double& lo, double& hi, double (*red)[4])
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double l = __shfl_xor(lo, m, 64), h = __shfl_xor(hi, m, 64);
        lo = (l < lo) ? l : lo; hi = (h > hi) ? h : hi;
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) { lo = (red[0][w] < lo) ? red[0][w] : lo; hi = (red[1][w] > hi) ? red[1][w] : hi; }
}
__global__ __launch_bounds__(256) void k_min_max(const double* __restrict__ x, int64_t n, int vec, double* __restrict__ pmin, double* __restrict__ pmax)
{
    __shared__ double red[2][4];
    double lo = INFINITY, hi = -INFINITY;
    const int64_t np = vec ? n >> 1 : 0, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    auto take = [&](double v) { lo = (v < lo) ? v : lo; hi = (v > hi) ? v : hi; };
    for (int64_t q = t; q < np; q += stride) { const double2 v = ld2(x, 2 * q); take(v.x); take(v.y); }
    for (int64_t i = 2 * np + t; i < n; i += stride) take(x[i]);
    ke_block_min_max(lo, hi, red);
    if (threadIdx.x == 0) { pmin[blockIdx.x] = lo; pmax[blockIdx.x] = hi; }
}
__global__ __launch_bounds__(256) void k_min_max_final(const double* __restrict__ pmin, const double* __restrict__ pmax, int g, double* __restrict__ out)
{
    __shared__ double red[2][4];
    double lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < g; i += 256) { lo = (pmin[i] < lo) ? pmin[i] : lo; hi = (pmax[i] > hi) ? pmax[i] : hi; }
    ke_block_min_max(lo, hi, red);
    if (threadIdx.x == 0) { out[0] = lo; out[1] = hi; }
}

// ---- fvc::average and bound: row passes on mu_rows (the walk of k_mules_solve / k_interface_curvature) ------------------------------------
struct AvArgs {
    RowTables r;
    const double *magSf, *bMagSf;                     // the weights, internal and boundary faces
    const double *x, *bx;                             // fvc_average: the face field; bound: lambda and the boundary face values
    const double *sum, *v;                            // surfaceSum(magSf) of the handle; bound: the cell field
    double lb;
    double* out;
};
// surfaceSum(magSf), kept by the handle
template <int BS>
__global__ __launch_bounds__(BS) void k_average_sum(const AvArgs a)
{
    const double* const src[1] = {a.magSf};
    double s = 0.0;
    mu_rows<BS, 1>(a.r, src, [](int) {},
        [&](int, int, const double (&v)[1]) { s = s + v[0]; },
        [&](int, int, const double (&v)[1]) { s = s + v[0]; },
        [&](int, int bf) { s = s + a.bMagSf[bf]; },
        [&](int c) { a.out[c] = s; });
}
// surfaceSum(magSf*ssf)/surfaceSum(magSf): each product rounded, then added
template <int BS>
__global__ __launch_bounds__(BS) void k_fvc_average(const AvArgs a)
{
    const double* const src[2] = {a.magSf, a.x};
    double s = 0.0;
    auto add = [&](int, int, const double (&v)[2]) { const double p = v[0] * v[1]; s = s + p; };
    mu_rows<BS, 2>(a.r, src, [](int) {}, add, add,
        [&](int, int bf) { const double p = a.bMagSf[bf] * a.bx[bf]; s = s + p; },
        [&](int c) { a.out[c] = s / a.sum[c]; });
}
// bound.C:45-54: the face value i = fma(lambda, mP - mN, mN) of m = max(vsf, lb) is formed on both sides of a face from the same operands,
// hence with the same bits; a cell reads its neighbours' values of the INPUT field, so out is another array (the handle's)
template <int BS>
__global__ __launch_bounds__(BS) void k_bound(const AvArgs a)
{
    const double* const src[2] = {a.magSf, a.x};
    const double lb = a.lb;
    double s = 0.0, vc = 0.0, mc = 0.0;
    mu_rows<BS, 2>(a.r, src,
        [&](int c) { vc = a.v[c]; mc = mu_max(vc, lb); },
        [&](int, int f, const double (&v)[2]) { const double mN = mu_max(a.v[a.r.up[f]], lb), i = fma(v[1], mc - mN, mN), p = v[0] * i; s = s + p; },
        [&](int, int f, const double (&v)[2]) { const double mP = mu_max(a.v[a.r.lo[f]], lb), i = fma(v[1], mP - mc, mc), p = v[0] * i; s = s + p; },
        [&](int, int bf) { const double p = a.bMagSf[bf] * a.bx[bf]; s = s + p; },
        [&](int c) {
            const double avg = s / a.sum[c], pos = (-vc >= 0) ? 1.0 : 0.0, t = avg * pos;
            a.out[c] = mu_max(mu_max(vc, t), lb);
        });
}

// ---- the wall functions ------------------------------------------------------------------------------------------------------------------------
struct KeWallArgs {
    const int32_t *cells, *start, *faces, *faceCell;  // the unique wall cells (ascending), the CSR of their wall faces in (patch, face) order
    const double* weight;                             // cornerWeight per unique wall cell
    const double *k, *u[3], *buw[3], *bdc, *by, *bnuw, *bnutw;
    double *G, *eps, *beps, *bpow, *bnut, *blog;
    double Cmu25, Cmu75, kappa, E, yPlusLam;
    int nCells, nFaces;
};
// epsilonWallFunction::updateCoeffs for every wall patch at once: one thread per unique wall cell.  pow and sqrt of k[c] are the same for
// every face of the cell and are evaluated once.
__global__ __launch_bounds__(256) void k_ke_wall_cells(const KeWallArgs a)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nCells; i += gridDim.x * blockDim.x) {
        const int c = a.cells[i], j0 = a.start[i], j1 = a.start[i + 1];
        const double w = a.weight[i], kc = a.k[c], p15 = pow(kc, 1.5), sq = sqrt(kc), wc = w * a.Cmu75;
        const double uc[3] = {a.u[0][c], a.u[1][c], a.u[2][c]};
        double Gc = 0.0, ec = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int bf = a.faces[j];
            const double dc = a.bdc[bf];
            double sn[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) sn[d] = dc * (a.buw[d][bf] - uc[d]);
            const double mgu = if_mag(sn), den = a.kappa * a.by[bf];
            const double e = (wc * p15) / den;
            const double g = ((((w * (a.bnutw[bf] + a.bnuw[bf])) * mgu) * a.Cmu25) * sq) / den;
            ec = ec + e; Gc = Gc + g;
        }
        a.G[c] = Gc; a.eps[c] = ec;
        for (int j = j0; j < j1; ++j) {
            const int bf = a.faces[j];
            a.beps[bf] = ec;
            if (a.bpow) a.bpow[bf] = p15;
        }
    }
}
// nutkWallFunction::calcNut on every wall face: one thread per face
__global__ __launch_bounds__(256) void k_ke_nut_wall(const KeWallArgs a)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < a.nFaces; j += gridDim.x * blockDim.x) {
        const int bf = a.faces[j], c = a.faceCell[j];
        const double nuw = a.bnuw[bf];
        const double yPlus = ((a.Cmu25 * a.by[bf]) * sqrt(a.k[c])) / nuw;
        double r = 0.0;
        if (yPlus > a.yPlusLam) {
            const double lg = log(a.E * yPlus);
            if (a.blog) a.blog[bf] = lg;
            r = nuw * (((yPlus * a.kappa) / lg) - 1.0);
        }
        a.bnut[bf] = r;
    }
}
__global__ __launch_bounds__(256) void k_ke_wall_values(const int32_t* __restrict__ cells, const double* __restrict__ x, double* __restrict__ out, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = x[cells[i]];
}

} // namespace mi

// fvc::average on one mesh: the row tables of the addressing, the boundary's per-cell face lists and surfaceSum(magSf); scratch is what
// mi_bound writes before it copies back
struct mi_average_s : RowHandle {
    DevBuf<double> sum, scratch;
};
// the wall cells of one mesh
struct mi_ke_s : RowHandle {
    int32_t nWallCells = 0, nWallFaces = 0;
    DevBuf<int32_t> cells, start, faces, faceCell;
    DevBuf<double> weight;
};

namespace {
bool ke_positive(double x) { return std::isfinite(x) && x > 0; }
int ke_coeffs_check(const std::string& who, const mi_ke_coeffs* k)
{
    if (!k) return fail(MI_ERR_ARG, who + ": the coefficients are missing");
    const double v[9] = {k->Cmu, k->C1, k->C2, k->sigmaEps, k->kappa, k->E, k->Cmu25, k->Cmu75, k->yPlusLam};
    for (double x : v) if (!ke_positive(x)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_ke_coeffs_init)");
    return MI_OK;
}
// the checks of a cell pass (missing, aliased, not aligned for a double), then the launch under the face-grid cap
template <class K>
int ke_cell_pass(const std::string& who, mi_ctx_s* c, int64_t n, K kernel, mi::KeCell& q, const double* const* in, int nIn, double* const* out, int nOut,
                 bool inPlace = false)
{
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n > INT32_MAX) return fail(MI_ERR_ARG, who + ": too many cells");
    if (n == 0) return MI_OK;
    if (inPlace) { if (!in[0] || !out[0]) return fail(MI_ERR_ARG, who + ": arrays missing"); }
    else { MICHK(arrays_present(who, in, nIn)); MICHK(outputs_distinct(who, in, nIn, out, nOut)); }
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    for (int i = 0; i < nIn; ++i) q.in[i] = in[i];
    for (int i = 0; i < nOut; ++i) q.out[i] = out[i];
    q.n = n; q.vec = all_aligned16(in, nIn, out, nOut) ? 1 : 0;
    HIPCHK(hipSetDevice(c->device));
    kernel<<<grid_for(c, (int)((n + 1) / 2)), 256, 0, c->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace

extern "C" int mi_ke_coeffs_init(double Cmu, double C1, double C2, double sigmaEps, double kappa, double E, mi_ke_coeffs* out)
{
    const std::string who = "mi_ke_coeffs_init";
    if (!out) return fail(MI_ERR_ARG, who + ": bad argument");
    const double v[6] = {Cmu, C1, C2, sigmaEps, kappa, E};
    for (double x : v) if (!ke_positive(x)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    mi_ke_coeffs k{};
    k.Cmu = Cmu; k.C1 = C1; k.C2 = C2; k.sigmaEps = sigmaEps; k.kappa = kappa; k.E = E;
    k.Cmu25 = std::sqrt(std::sqrt(Cmu));              // pow025 (Scalar.H:207-210)
    k.Cmu75 = std::pow(Cmu, 0.75);
    double ypl = 11.0;                                // nutWallFunctionFvPatchScalarField::yPlusLam (:154-167)
    for (int i = 0; i < 10; ++i) { const double t = E * ypl; ypl = std::log(t > 1.0 ? t : 1.0) / kappa; }
    k.yPlusLam = ypl;
    MICHK(ke_coeffs_check(who, &k));
    *out = k;
    return MI_OK;
}

extern "C" int mi_min_max(mi_ctx_t c, int64_t n, const double* x_dev, double* min_out_host, double* max_out_host)
{
    const std::string who = "mi_min_max";
    if (!c || n < 0 || (n > 0 && !x_dev)) return fail(MI_ERR_ARG, who + ": bad argument");
    if (!al8(x_dev)) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
    double lo = INFINITY, hi = -INFINITY;
    if (n > 0) {
        if (c->session) return fail(MI_ERR_STATE, who + ": a PCG session (mi_pcg_begin) is active on this context and owns its reduction scratch; call mi_pcg_end first");
        HIPCHK(hipSetDevice(c->device));
        const int64_t pairs = (n + 1) / 2;
        int g = grid_for(c, pairs > INT32_MAX ? INT32_MAX : (int)pairs);
        if (g > RG) g = RG;
        k_min_max<<<g, 256, 0, c->stream>>>(x_dev, n, al16(x_dev) ? 1 : 0, c->partial.p, c->partial.p + RG);
        k_min_max_final<<<1, 256, 0, c->stream>>>(c->partial.p, c->partial.p + RG, g, c->scalars.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->hostScal, c->scalars.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        lo = c->hostScal[0]; hi = c->hostScal[1];
    }
    if (min_out_host) *min_out_host = lo;
    if (max_out_host) *max_out_host = hi;
    return MI_OK;
}

extern "C" int mi_vec_max_value(mi_ctx_t c, int64_t n, const double* x_dev, double value, double* out_dev)
{
    KeCell q{};
    q.c1 = value;
    const double* in[1] = {x_dev};
    double* out[1] = {out_dev};
    return ke_cell_pass("mi_vec_max_value", c, n, k_vec_max_value, q, in, 1, out, 1, true);
}

extern "C" int mi_average_create(mi_addr_t a, mi_grad_boundary_t b, const double* mag_sf_dev, const double* b_mag_sf_dev, mi_average_t* out)
{
    const std::string who = "mi_average_create";
    std::unique_ptr<mi_average_s> h(new mi_average_s());
    MICHK(row_handle_open(who, a, b, out, *h));
    const int32_t nb = h->nBFaces;
    if (a->L.nCells > 0 && a->L.nFaces > 0 && !mag_sf_dev) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (a->L.nCells > 0 && nb > 0 && !b_mag_sf_dev) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary face areas needed");
    if (!al8(mag_sf_dev) || !al8(b_mag_sf_dev)) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    MICHK(h->sum.alloc((size_t)h->nCells));
    MICHK(h->scratch.alloc((size_t)h->nCells));
    if (h->nCells > 0) {
        AvArgs q{};
        q.r = row_tables(a, b);
        q.magSf = mag_sf_dev; q.bMagSf = b_mag_sf_dev; q.out = h->sum.p;
        MICHK(row_launch_bs(a, 1, ROW_BS(k_average_sum), q));
        HIPCHK(hipStreamSynchronize(a->ctx->stream));
    }
    *out = h.release();
    return MI_OK;
}
extern "C" int mi_average_destroy(mi_average_t h) { delete h; return MI_OK; }

extern "C" int mi_fvc_average(mi_average_t h, const double* mag_sf_dev, const double* b_mag_sf_dev, const double* ssf_dev, const double* b_ssf_dev,
                              double* out_dev)
{
    const std::string who = "mi_fvc_average";
    MICHK(row_handle_check(who, h));
    if (h->nCells == 0) return MI_OK;
    if (h->nFaces > 0 && (!mag_sf_dev || !ssf_dev)) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (h->nBFaces > 0 && (!b_mag_sf_dev || !b_ssf_dev)) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary arrays needed");
    const double* in[4];                              // an empty array may be NULL and is never read
    int nIn = 0;
    if (h->nFaces > 0) { in[nIn++] = mag_sf_dev; in[nIn++] = ssf_dev; }
    if (h->nBFaces > 0) { in[nIn++] = b_mag_sf_dev; in[nIn++] = b_ssf_dev; }
    double* out[1] = {out_dev};
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out, 1));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, 1));
    mi_addr_s* a = h->addr;
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    AvArgs q{};
    q.r = row_tables(a, h->boundary);
    q.magSf = mag_sf_dev; q.bMagSf = b_mag_sf_dev; q.x = ssf_dev; q.bx = b_ssf_dev; q.sum = h->sum.p; q.out = out_dev;
    return row_launch_bs(a, 2, ROW_BS(k_fvc_average), q);
}

extern "C" int mi_bound(mi_average_t h, double lower_bound, const double* lambda_dev, const double* mag_sf_dev, const double* b_mag_sf_dev,
                        const double* b_face_dev, double* vsf_inout_dev)
{
    const std::string who = "mi_bound";
    MICHK(row_handle_check(who, h));
    if (std::isnan(lower_bound)) return fail(MI_ERR_ARG, who + ": lower_bound is not a number");
    if (h->nCells == 0) return MI_OK;
    if (h->nFaces > 0 && (!mag_sf_dev || !lambda_dev)) return fail(MI_ERR_ARG, who + ": an input array is missing");
    if (h->nBFaces > 0 && (!b_mag_sf_dev || !b_face_dev)) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary arrays needed");
    const double* in[4];
    int nIn = 0;
    if (h->nFaces > 0) { in[nIn++] = mag_sf_dev; in[nIn++] = lambda_dev; }
    if (h->nBFaces > 0) { in[nIn++] = b_mag_sf_dev; in[nIn++] = b_face_dev; }
    double* out[1] = {vsf_inout_dev};
    MICHK(arrays_present(who, in, nIn));
    MICHK(outputs_distinct(who, in, nIn, out, 1));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)out, 1));
    mi_addr_s* a = h->addr;
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    AvArgs q{};
    q.r = row_tables(a, h->boundary);
    q.magSf = mag_sf_dev; q.bMagSf = b_mag_sf_dev; q.x = lambda_dev; q.bx = b_face_dev; q.sum = h->sum.p; q.v = vsf_inout_dev; q.lb = lower_bound;
    q.out = h->scratch.p;
    MICHK(row_launch_bs(a, 2, ROW_BS(k_bound), q));
    HIPCHK(hipMemcpyAsync(vsf_inout_dev, h->scratch.p, (size_t)h->nCells * sizeof(double), hipMemcpyDeviceToDevice, a->ctx->stream));
    return MI_OK;
}

extern "C" int mi_ke_production(mi_ctx_t c, int64_t n, const double* nut_dev, const double* const* grad_dev, double* g_out_dev)
{
    const std::string who = "mi_ke_production";
    if (n > 0 && !grad_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    KeCell q{};
    const double* in[10] = {nut_dev};
    if (grad_dev) for (int i = 0; i < 9; ++i) in[1 + i] = grad_dev[i];
    double* out[1] = {g_out_dev};
    return ke_cell_pass(who, c, n, k_ke_production, q, in, 10, out, 1);
}

extern "C" int mi_ke_epsilon_terms(mi_ctx_t c, int64_t n, const mi_ke_coeffs* coeffs, const double* g_dev, const double* eps_dev, const double* k_dev,
                                   const double* nut_dev, const double* nu_dev_or_null, double nu_value, double* su_out_dev, double* sp_out_dev,
                                   double* deps_out_dev)
{
    const std::string who = "mi_ke_epsilon_terms";
    MICHK(ke_coeffs_check(who, coeffs));
    KeCell q{};
    q.c1 = coeffs->C1; q.c2 = coeffs->C2; q.c3 = coeffs->sigmaEps; q.nu = nu_value;
    const double* in[5] = {g_dev, eps_dev, k_dev, nut_dev, nu_dev_or_null};
    double* out[3] = {su_out_dev, sp_out_dev, deps_out_dev};
    if (nu_dev_or_null) return ke_cell_pass(who, c, n, k_ke_epsilon_terms<true>, q, in, 5, out, 3);
    return ke_cell_pass(who, c, n, k_ke_epsilon_terms<false>, q, in, 4, out, 3);
}

extern "C" int mi_ke_k_terms(mi_ctx_t c, int64_t n, const double* eps_dev, const double* k_dev, const double* nut_dev, const double* nu_dev_or_null,
                             double nu_value, double* sp_out_dev, double* dk_out_dev)
{
    const std::string who = "mi_ke_k_terms";
    KeCell q{};
    q.nu = nu_value;
    const double* in[4] = {eps_dev, k_dev, nut_dev, nu_dev_or_null};
    double* out[2] = {sp_out_dev, dk_out_dev};
    if (nu_dev_or_null) return ke_cell_pass(who, c, n, k_ke_k_terms<true>, q, in, 4, out, 2);
    return ke_cell_pass(who, c, n, k_ke_k_terms<false>, q, in, 3, out, 2);
}

extern "C" int mi_ke_nut(mi_ctx_t c, int64_t n, double Cmu, const double* k_dev, const double* eps_dev, double* nut_out_dev)
{
    const std::string who = "mi_ke_nut";
    if (!ke_positive(Cmu)) return fail(MI_ERR_ARG, who + ": Cmu must be a finite number above zero");
    KeCell q{};
    q.c1 = Cmu;
    const double* in[2] = {k_dev, eps_dev};
    double* out[1] = {nut_out_dev};
    return ke_cell_pass(who, c, n, k_ke_nut, q, in, 2, out, 1);
}

extern "C" int mi_ke_create(mi_addr_t a, mi_grad_boundary_t b, const int32_t* patch_is_wall, mi_ke_t* out)
{
    const std::string who = "mi_ke_create";
    if (!b) return fail(MI_ERR_ARG, who + ": bad argument");   // the wall cells are the boundary's
    std::unique_ptr<mi_ke_s> h(new mi_ke_s());
    MICHK(row_handle_open(who, a, b, out, *h));
    const int32_t nP = (int32_t)b->patchSizes.size(), n = b->nCells, nb = b->nFaces;
    if (nP > 0 && !patch_is_wall) return fail(MI_ERR_ARG, who + ": patch_is_wall is missing");
    std::vector<uint8_t> wall((size_t)nb, 0);         // per boundary face: on a wall patch
    {
        int32_t off = 0;
        for (int32_t p = 0; p < nP; ++p) {
            if (patch_is_wall[p] && b->patchKinds[p] == MI_GRAD_PATCH_COUPLED) return fail(MI_ERR_ARG, who + ": patch " + std::to_string(p) + " is a coupled patch, not a wall");
            if (patch_is_wall[p]) std::fill(wall.begin() + off, wall.begin() + off + b->patchSizes[p], (uint8_t)1);
            off += b->patchSizes[p];
        }
    }
    HIPCHK(hipSetDevice(a->ctx->device));               // no caller-order tables: the wall kernels walk the handle's own lists
    // the boundary's per-cell face lists hold every cell's boundary faces by patch, then by face: the wall faces among them, in that order
    std::vector<int32_t> allStart((size_t)n + 1, 0), all((size_t)nb);
    if (nb > 0) {
        HIPCHK(hipMemcpy(allStart.data(), b->allStart.p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(all.data(), b->all.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    Table<int32_t> cells, start, faces, faceCell;
    Table<double> weight;
    for (int32_t c = 0; c < n; ++c) {
        const size_t before = faces.size();
        for (int32_t j = allStart[c]; j < allStart[(size_t)c + 1]; ++j) if (wall[(size_t)all[j]]) { faces.push_back(all[j]); faceCell.push_back(c); }
        if (faces.size() > before) {
            cells.push_back(c); start.push_back((int32_t)before);
            weight.push_back(1.0 / (double)(faces.size() - before));      // cornerWeights (:146-200): 1.0/(wall faces of the cell)
        }
    }
    start.push_back((int32_t)faces.size());
    h->nWallCells = (int32_t)cells.size(); h->nWallFaces = (int32_t)faces.size();
    hipStream_t s = a->ctx->stream;
    MICHK(h->cells.upload(cells, s)); MICHK(h->start.upload(start, s)); MICHK(h->faces.upload(faces, s)); MICHK(h->faceCell.upload(faceCell, s));
    MICHK(h->weight.upload(weight, s));
    HIPCHK(hipStreamSynchronize(s));
    *out = h.release();
    return MI_OK;
}
extern "C" int mi_ke_destroy(mi_ke_t h) { delete h; return MI_OK; }

namespace {
void ke_wall_tables(const mi_ke_s* h, const mi_ke_coeffs* k, KeWallArgs& q)
{
    q.cells = h->cells.p; q.start = h->start.p; q.faces = h->faces.p; q.faceCell = h->faceCell.p; q.weight = h->weight.p;
    q.Cmu25 = k->Cmu25; q.Cmu75 = k->Cmu75; q.kappa = k->kappa; q.E = k->E; q.yPlusLam = k->yPlusLam;
    q.nCells = h->nWallCells; q.nFaces = h->nWallFaces;
}
} // namespace

extern "C" int mi_ke_wall_cells(mi_ke_t h, const mi_ke_coeffs* coeffs, const mi_ke_wall* x)
{
    const std::string who = "mi_ke_wall_cells";
    MICHK(row_handle_check(who, h));
    MICHK(ke_coeffs_check(who, coeffs));
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    if (h->nWallFaces == 0) return MI_OK;
    const double* in[12] = {x->k_dev, x->u_dev[0], x->u_dev[1], x->u_dev[2], x->b_uw_dev[0], x->b_uw_dev[1], x->b_uw_dev[2],
                            x->b_delta_coeffs_dev, x->b_y_dev, x->b_nuw_dev, x->b_nutw_dev};
    double* out[4] = {x->g_inout_dev, x->eps_inout_dev, x->b_eps_out_dev, x->b_pow_out_dev};
    const int nOut = x->b_pow_out_dev ? 4 : 3;
    MICHK(arrays_present(who, in, 11));
    MICHK(outputs_distinct(who, in, 11, out, nOut));
    MICHK(arrays_aligned8(who, (const void* const*)in, 11));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    HIPCHK(hipSetDevice(h->ctx->device));
    KeWallArgs q{};
    ke_wall_tables(h, coeffs, q);
    q.k = x->k_dev; q.bdc = x->b_delta_coeffs_dev; q.by = x->b_y_dev; q.bnuw = x->b_nuw_dev; q.bnutw = x->b_nutw_dev;
    for (int d = 0; d < 3; ++d) { q.u[d] = x->u_dev[d]; q.buw[d] = x->b_uw_dev[d]; }
    q.G = x->g_inout_dev; q.eps = x->eps_inout_dev; q.beps = x->b_eps_out_dev; q.bpow = x->b_pow_out_dev;
    k_ke_wall_cells<<<grid_for(h->ctx, h->nWallCells), 256, 0, h->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_ke_nut_wall(mi_ke_t h, const mi_ke_coeffs* coeffs, const double* k_dev, const double* b_y_dev, const double* b_nuw_dev,
                              double* b_nutw_out_dev, double* b_log_out_dev_or_null)
{
    const std::string who = "mi_ke_nut_wall";
    MICHK(row_handle_check(who, h));
    MICHK(ke_coeffs_check(who, coeffs));
    if (h->nWallFaces == 0) return MI_OK;
    const double* in[3] = {k_dev, b_y_dev, b_nuw_dev};
    double* out[2] = {b_nutw_out_dev, b_log_out_dev_or_null};
    const int nOut = b_log_out_dev_or_null ? 2 : 1;
    MICHK(arrays_present(who, in, 3));
    MICHK(outputs_distinct(who, in, 3, out, nOut));
    MICHK(arrays_aligned8(who, (const void* const*)in, 3));
    MICHK(arrays_aligned8(who, (const void* const*)out, nOut));
    HIPCHK(hipSetDevice(h->ctx->device));
    KeWallArgs q{};
    ke_wall_tables(h, coeffs, q);
    q.k = k_dev; q.by = b_y_dev; q.bnuw = b_nuw_dev; q.bnut = b_nutw_out_dev; q.blog = b_log_out_dev_or_null;
    k_ke_nut_wall<<<grid_for(h->ctx, h->nWallFaces), 256, 0, h->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_ke_wall_cell_labels(mi_ke_t h, int32_t* n_out, const int32_t** labels_dev_out)
{
    MICHK(row_handle_check("mi_ke_wall_cell_labels", h));
    if (!n_out || !labels_dev_out) return fail(MI_ERR_ARG, "mi_ke_wall_cell_labels: bad argument");
    *n_out = h->nWallCells;
    *labels_dev_out = h->cells.p;
    return MI_OK;
}

extern "C" int mi_ke_wall_values(mi_ke_t h, const double* eps_dev, double* values_out_dev)
{
    const std::string who = "mi_ke_wall_values";
    MICHK(row_handle_check(who, h));
    if (h->nWallCells == 0) return MI_OK;
    const double* in[1] = {eps_dev};
    double* out[1] = {values_out_dev};
    MICHK(arrays_present(who, in, 1));
    MICHK(outputs_distinct(who, in, 1, out, 1));
    MICHK(arrays_aligned8(who, (const void* const*)in, 1));
    MICHK(arrays_aligned8(who, (const void* const*)out, 1));
    HIPCHK(hipSetDevice(h->ctx->device));
    k_ke_wall_values<<<grid_for(h->ctx, h->nWallCells), 256, 0, h->ctx->stream>>>(h->cells.p, eps_dev, values_out_dev, h->nWallCells);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// ==== incompressible::RASModels::kOmegaSST (turbulenceModels/incompressible/RAS/kOmegaSST/kOmegaSST.C:47-111, :284-296, :398-468, kOmegaSST.H:164-243;
// omegaWallFunctionFvPatchScalarField.C:209-239, :241-394, :548-596; fvMatrix.C:2208-2216, :2759-2814; fvmSup.C:100-214; DESIGN 3.5p) ==========
//
//   production  :412-413  S2 = 2*magSqr(symm(gradU)), G = nut*S2 (and mag(symm(gradU)) for the constructor's nut) in one cell pass
//   wall cells  :416      omega.boundaryField().updateCoeffs() for ALL wall patches in one launch on the mi_ke_t handle, as k_ke_wall_cells
//   blend       :418-439  CDkOmega, F1, F23, the four blends, the omega equation's su / sp / susp and both diffusivities in one cell pass
//   sources     :432-439  su - fvm::Sp - fvm::SuSp as the reference groups it: the matrix of the right-hand side formed, then subtracted
//   k terms     :456-457  min(G, (c1*betaStar)*k*omega) and betaStar*omega
//   nut         :466, :287-295  a1*k/max(a1*omega, (b1*F23)*sqrt(S2)) with F23 recomputed in the pass
// y, the wall distance of every cell, is the caller's array.  min(a, b) = (a < b) ? a : b.  tanh is the device library's: F1 and F23 are not
// the reference's bits, everything before them and everything formed from them is.  Restated in tests/komegasst_support.py.
namespace mi {

struct SstCell {
    const double* in[12];
    double* out[10];
    uint32_t n;                                       // the entries refuse more than INT32_MAX cells
    int vec, ctor;
    uint32_t want;                                    // bit k: output k is written (an optional output that is not wanted is NULL)
    double nu;
    mi_sst_coeffs K;
};
// The argument block as the kernel finds it in its argument segment (the one by-value argument, at offset 0).  mi_sst_blend has 22 array
// bases and 16 coefficients: held in scalar registers across the loop together they do not fit and the compiler spills them to vector lanes.
// The empty asm makes the pointer opaque, so the bases are read where the loads and where the stores need them (scalar loads that hit the
// scalar cache) and are not live across the cell's arithmetic.
typedef const SstCell __attribute__((address_space(4)))* SstArgs;
__device__ __forceinline__ SstArgs sst_args()
{
    SstArgs p = (SstArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// ke_map for the wider passes of this model: the same walk; outputs from NREQ on are written only when wanted (the same for every thread).
// 32-bit counters: 2*q < n <= INT32_MAX and q + stride < 2^32.
template <int NIN, int NOUT, int NREQ, class F>
__device__ __forceinline__ void sst_map(const SstCell& a, F f)
{
    const uint32_t n = a.n, np = a.vec ? n >> 1 : 0, t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x, want = a.want;
    for (uint32_t q = t; q < np; q += stride) {
        const uint32_t i = 2 * q;
        double x[NIN], y[NIN], ox[NOUT], oy[NOUT];
        SstArgs p = sst_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) { const double2 v = ld2(p->in[k], i); x[k] = v.x; y[k] = v.y; }
        f(x, ox); f(y, oy);
        p = sst_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (want >> k & 1u)) st2(p->out[k], i, make_double2(ox[k], oy[k]));
    }
    for (uint32_t i = 2 * np + t; i < n; i += stride) {
        double x[NIN], o[NOUT];
        SstArgs p = sst_args();
#pragma unroll
        for (int k = 0; k < NIN; ++k) x[k] = p->in[k][i];
        f(x, o);
        p = sst_args();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) if (k < NREQ || (want >> k & 1u)) p->out[k][i] = o[k];
    }
}
__device__ __forceinline__ double sst_min(double a, double b) { return (a < b) ? a : b; }
__device__ __forceinline__ double sst_pow4(double s) { const double q = s * s; return q * q; }   // Scalar.H:189 sqr(sqr(s))
// F23() :73-111 -> F2, or F2*F3 under the F3 switch; t3 = tanh(pow4(arg3)) (0 without the switch)
template <bool F3>
__device__ __forceinline__ double sst_f23(const mi_sst_coeffs& K, double k, double omega, double y, double nu, double& t3)
{
    const double y2 = y * y;
    const double far = (500.0 * nu) / (y2 * omega);
    const double arg2 = sst_min(mu_max((K.twoInvBetaStar * sqrt(k)) / (omega * y), far), 100.0);
    double f = tanh(arg2 * arg2);
    t3 = 0.0;
    if (F3) {
        const double arg3 = sst_min((150.0 * nu) / (omega * y2), 10.0);
        t3 = tanh(sst_pow4(arg3));
        f = f * (1.0 - t3);
    }
    return f;
}
__device__ __forceinline__ double sst_blend(double F1, double d, double psi2) { return F1 * d + psi2; }   // kOmegaSST.H:164-172, d = psi1 - psi2

// in: nut, gradU[9]; out: S2, G, mag(symm(gradU)) (optional)
__global__ __launch_bounds__(256) void k_sst_production(const SstCell a)
{
    sst_map<10, 3, 2>(a, [](const double (&x)[10], double (&o)[3]) {
        const double m = ke_magsqr_symm(x + 1);
        o[0] = 2.0 * m;
        o[1] = x[0] * o[0];
        o[2] = sqrt(m);
    });
}
// in: gradK[3], gradOmega[3], k, omega, y, nut, S2, [nu]; out: F1, su, sp, susp, DomegaEff, DkEff, then optional CDkOmega, arg1, F23, tanh(pow4(arg3))
template <bool NUF, bool F3>
__global__ __launch_bounds__(256) void k_sst_blend(const SstCell a)
{
    constexpr int NIN = NUF ? 12 : 11;
    const mi_sst_coeffs K = a.K;
    const double nu0 = a.nu;
    // the eight values of the blends live in vector registers (there is room at this occupancy, there is none among the scalar ones)
    double dGamma = K.dGamma, gamma2 = K.gamma2, dBeta = K.dBeta, beta2 = K.beta2, dAO = K.dAlphaOmega, aO2 = K.alphaOmega2, dAK = K.dAlphaK, aK2 = K.alphaK2;
    asm volatile("" : "+v"(dGamma), "+v"(gamma2), "+v"(dBeta), "+v"(beta2), "+v"(dAO), "+v"(aO2), "+v"(dAK), "+v"(aK2));
    sst_map<NIN, 10, 6>(a, [=](const double (&x)[NIN], double (&o)[10]) {
        const double k = x[6], omega = x[7], y = x[8], nut = x[9], S2 = x[10], nu = NUF ? x[NIN - 1] : nu0;
        const double CD = (K.twoAlphaOmega2 * lu_dot(x[0], x[1], x[2], x[3], x[4], x[5])) / omega;
        const double CDplus = mu_max(CD, 1.0e-10);
        const double y2 = y * y, sk = sqrt(k);
        const double arg1 = sst_min(sst_min(mu_max((K.invBetaStar * sk) / (omega * y), (500.0 * nu) / (y2 * omega)), (K.fourAlphaOmega2 * k) / (CDplus * y2)), 10.0);
        const double F1 = tanh(sst_pow4(arg1));
        double t3;
        const double F23 = sst_f23<F3>(K, k, omega, y, nu, t3);
        o[0] = F1;
        o[1] = sst_blend(F1, dGamma, gamma2) * sst_min(S2, (K.c1a1BetaStar * omega) * mu_max(K.a1 * omega, (K.b1 * F23) * sqrt(S2)));
        o[2] = sst_blend(F1, dBeta, beta2) * omega;
        o[3] = ((F1 - 1.0) * CD) / omega;
        o[4] = sst_blend(F1, dAO, aO2) * nut + nu;
        o[5] = sst_blend(F1, dAK, aK2) * nut + nu;
        o[6] = CD; o[7] = arg1; o[8] = F23; o[9] = t3;
    });
}
// in: V, su, sp, susp, omega, diag, source; out: diag, source (in place)
__global__ __launch_bounds__(256) void k_sst_omega_sources(const SstCell a)
{
    sst_map<7, 2, 2>(a, [](const double (&x)[7], double (&o)[2]) {
        const double V = x[0], su = x[1], sp = x[2], susp = x[3], omega = x[4];
        const double rd = (-(V * sp)) - V * mu_max(susp, 0.0);
        const double rs = (-(V * su)) - (0.0 - (V * sst_min(susp, 0.0)) * omega);
        o[0] = x[5] - rd;
        o[1] = x[6] - rs;
    });
}
// in: G, k, omega; out: su, sp
__global__ __launch_bounds__(256) void k_sst_k_terms(const SstCell a)
{
    const double cbk = a.K.c1BetaStar, betaStar = a.K.betaStar;
    sst_map<3, 2, 2>(a, [=](const double (&x)[3], double (&o)[2]) {
        o[0] = sst_min(x[0], (cbk * x[1]) * x[2]);
        o[1] = betaStar * x[2];
    });
}
// in: k, omega, y, S2 (the constructor's form: mag(symm(gradU))), [nu]; out: nut, optional F23
template <bool NUF, bool F3>
__global__ __launch_bounds__(256) void k_sst_nut(const SstCell a)
{
    constexpr int NIN = NUF ? 5 : 4;
    const mi_sst_coeffs K = a.K;
    const int ctor = a.ctor;
    const double nu0 = a.nu;
    sst_map<NIN, 2, 1>(a, [=](const double (&x)[NIN], double (&o)[2]) {
        double t3;
        const double F23 = sst_f23<F3>(K, x[0], x[1], x[2], NUF ? x[NIN - 1] : nu0, t3);
        const double bF = K.b1 * F23;
        const double strain = ctor ? (bF * sqrt(2.0)) * x[3] : bF * sqrt(x[3]);
        o[0] = (K.a1 * x[0]) / mu_max(K.a1 * x[1], strain);
        o[1] = F23;
    });
}

struct SstWallArgs {
    const int32_t *cells, *start, *faces;
    const double* weight;
    const double *k, *u[3], *buw[3], *bdc, *by, *bnuw, *bnutw;
    double *G, *omega, *bomega;
    double Cmu25, kappa, beta1;
    int nCells;
};
// omegaWallFunction::updateCoeffs for every wall patch at once, as k_ke_wall_cells.  OmegaCalculateOmegaFunctor (:270-279):
// w*sqrt(sqr(omegaVis) + sqr(omegaLog)) with the first square contracted into the sum (an ASSUMPTION, DESIGN 3.5p)
__global__ __launch_bounds__(256) void k_sst_wall_cells(const SstWallArgs a)
{
    const double ck = a.Cmu25 * a.kappa;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nCells; i += gridDim.x * blockDim.x) {
        const int c = a.cells[i], j0 = a.start[i], j1 = a.start[i + 1];
        const double w = a.weight[i], sq = sqrt(a.k[c]);
        const double uc[3] = {a.u[0][c], a.u[1][c], a.u[2][c]};
        double Gc = 0.0, oc = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int bf = a.faces[j];
            const double dc = a.bdc[bf], y = a.by[bf], nuw = a.bnuw[bf];
            double sn[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) sn[d] = dc * (a.buw[d][bf] - uc[d]);
            const double mgu = if_mag(sn);
            const double omegaVis = (6.0 * nuw) / (a.beta1 * (y * y));
            const double omegaLog = sq / (ck * y);
            const double o = w * sqrt(fma(omegaVis, omegaVis, omegaLog * omegaLog));
            const double g = ((((w * (a.bnutw[bf] + nuw)) * mgu) * a.Cmu25) * sq) / (a.kappa * y);
            oc = oc + o; Gc = Gc + g;
        }
        a.G[c] = Gc; a.omega[c] = oc;
        for (int j = j0; j < j1; ++j) a.bomega[a.faces[j]] = oc;
    }
}

} // namespace mi

namespace {
int sst_coeffs_check(const std::string& who, const mi_sst_coeffs* k)
{
    if (!k) return fail(MI_ERR_ARG, who + ": the coefficients are missing");
    const double pos[23] = {k->alphaK1, k->alphaK2, k->alphaOmega1, k->alphaOmega2, k->gamma1, k->gamma2, k->beta1, k->beta2, k->betaStar, k->a1, k->b1, k->c1,
                            k->Cmu, k->kappa, k->E, k->wallBeta1, k->twoAlphaOmega2, k->fourAlphaOmega2, k->invBetaStar, k->twoInvBetaStar, k->c1a1BetaStar,
                            k->c1BetaStar, k->Cmu25};
    for (double x : pos) if (!ke_positive(x)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_sst_coeffs_init)");
    if (!ke_positive(k->yPlusLam)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_sst_coeffs_init)");
    const double any[4] = {k->dAlphaK, k->dAlphaOmega, k->dBeta, k->dGamma};
    for (double x : any) if (!std::isfinite(x)) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero (mi_sst_coeffs_init)");
    return MI_OK;
}
// the checks of ke_cell_pass for an SstCell: nOpt trailing outputs may be NULL; nInOut leading outputs are also the LAST nInOut inputs
template <class K>
int sst_cell_pass(const std::string& who, mi_ctx_s* c, int64_t n, K kernel, mi::SstCell& q, const double* const* in, int nIn, double* const* out, int nOut,
                  int nOpt = 0, int nInOut = 0)
{
    if (!c || n < 0) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n > INT32_MAX) return fail(MI_ERR_ARG, who + ": too many cells");
    if (n == 0) return MI_OK;
    MICHK(arrays_present(who, in, nIn));
    const double* inAll[12];
    double* given[10];
    int nGiven = 0;
    q.want = 0;
    for (int i = 0; i < nOut; ++i) {
        if (!out[i] && i >= nOut - nOpt) continue;
        given[nGiven++] = out[i];
        q.want |= 1u << i;
    }
    for (int i = 0; i < nIn - nInOut; ++i) inAll[i] = in[i];
    MICHK(outputs_distinct(who, inAll, nIn - nInOut, given, nGiven));
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
} // namespace

extern "C" int mi_sst_coeffs_init(const double* model_or_null, const double* wall_or_null, mi_sst_coeffs* out)
{
    const std::string who = "mi_sst_coeffs_init";
    if (!out) return fail(MI_ERR_ARG, who + ": bad argument");
    const double model0[12] = {0.85, 1.0, 0.5, 0.856, 5.0 / 9.0, 0.44, 0.075, 0.0828, 0.09, 0.31, 1.0, 10.0};   // kOmegaSST.C:127-243
    const double wall0[4] = {0.09, 0.41, 9.8, 0.075};                                                           // omegaWallFunction :406-409
    const double* m = model_or_null ? model_or_null : model0;
    const double* w = wall_or_null ? wall_or_null : wall0;
    for (int i = 0; i < 12; ++i) if (!ke_positive(m[i])) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    for (int i = 0; i < 4; ++i) if (!ke_positive(w[i])) return fail(MI_ERR_ARG, who + ": every coefficient must be a finite number above zero");
    mi_sst_coeffs k{};
    k.alphaK1 = m[0]; k.alphaK2 = m[1]; k.alphaOmega1 = m[2]; k.alphaOmega2 = m[3]; k.gamma1 = m[4]; k.gamma2 = m[5];
    k.beta1 = m[6]; k.beta2 = m[7]; k.betaStar = m[8]; k.a1 = m[9]; k.b1 = m[10]; k.c1 = m[11];
    k.Cmu = w[0]; k.kappa = w[1]; k.E = w[2]; k.wallBeta1 = w[3];
    // the products of dimensionedScalars, formed once in the reference's order
    k.twoAlphaOmega2 = 2 * k.alphaOmega2;             // :420
    k.fourAlphaOmega2 = 4 * k.alphaOmega2;            // :64
    k.invBetaStar = 1.0 / k.betaStar;                 // :61
    k.twoInvBetaStar = 2.0 / k.betaStar;              // :80
    k.c1a1BetaStar = (k.c1 / k.a1) * k.betaStar;      // :433
    k.c1BetaStar = k.c1 * k.betaStar;                 // :456
    k.dAlphaK = k.alphaK1 - k.alphaK2; k.dAlphaOmega = k.alphaOmega1 - k.alphaOmega2; k.dBeta = k.beta1 - k.beta2; k.dGamma = k.gamma1 - k.gamma2;
    k.Cmu25 = std::sqrt(std::sqrt(k.Cmu));
    double ypl = 11.0;
    for (int i = 0; i < 10; ++i) { const double t = k.E * ypl; ypl = std::log(t > 1.0 ? t : 1.0) / k.kappa; }
    k.yPlusLam = ypl;
    MICHK(sst_coeffs_check(who, &k));
    *out = k;
    return MI_OK;
}

extern "C" int mi_sst_production(mi_ctx_t c, int64_t n, const double* nut_dev, const double* const* grad_dev, double* s2_out_dev, double* g_out_dev,
                                 double* mag_out_dev_or_null)
{
    const std::string who = "mi_sst_production";
    if (n > 0 && !grad_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    SstCell q{};
    const double* in[10] = {nut_dev};
    if (grad_dev) for (int i = 0; i < 9; ++i) in[1 + i] = grad_dev[i];
    double* out[3] = {s2_out_dev, g_out_dev, mag_out_dev_or_null};
    return sst_cell_pass(who, c, n, k_sst_production, q, in, 10, out, 3, 1);
}

extern "C" int mi_sst_blend(mi_ctx_t c, int64_t n, const mi_sst_coeffs* coeffs, int f3, const mi_sst_blend_arrays* x)
{
    const std::string who = "mi_sst_blend";
    MICHK(sst_coeffs_check(who, coeffs));
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    if (!x->nu_dev_or_null && !ke_positive(x->nu_value)) return fail(MI_ERR_ARG, who + ": nu must be a finite number above zero");
    SstCell q{};
    q.K = *coeffs; q.nu = x->nu_value;
    const double* in[12] = {x->grad_k_dev[0], x->grad_k_dev[1], x->grad_k_dev[2], x->grad_omega_dev[0], x->grad_omega_dev[1], x->grad_omega_dev[2],
                            x->k_dev, x->omega_dev, x->y_dev, x->nut_dev, x->s2_dev, x->nu_dev_or_null};
    double* out[10] = {x->f1_out_dev, x->su_out_dev, x->sp_out_dev, x->susp_out_dev, x->domega_out_dev, x->dk_out_dev,
                       x->cdkomega_out_dev_or_null, x->arg1_out_dev_or_null, x->f23_out_dev_or_null, x->tanh3_out_dev_or_null};
    auto kernel = x->nu_dev_or_null ? (f3 ? k_sst_blend<true, true> : k_sst_blend<true, false>) : (f3 ? k_sst_blend<false, true> : k_sst_blend<false, false>);
    return sst_cell_pass(who, c, n, kernel, q, in, x->nu_dev_or_null ? 12 : 11, out, 10, 4);
}

extern "C" int mi_sst_omega_sources(mi_ctx_t c, int64_t n, const double* vol_dev, const double* su_dev, const double* sp_dev, const double* susp_dev,
                                    const double* omega_dev, double* diag_inout_dev, double* source_inout_dev)
{
    SstCell q{};
    const double* in[7] = {vol_dev, su_dev, sp_dev, susp_dev, omega_dev, diag_inout_dev, source_inout_dev};
    double* out[2] = {diag_inout_dev, source_inout_dev};
    if (n > 0 && (!diag_inout_dev || !source_inout_dev)) return fail(MI_ERR_ARG, "mi_sst_omega_sources: output arrays missing");
    return sst_cell_pass("mi_sst_omega_sources", c, n, k_sst_omega_sources, q, in, 7, out, 2, 0, 2);
}

extern "C" int mi_sst_k_terms(mi_ctx_t c, int64_t n, const mi_sst_coeffs* coeffs, const double* g_dev, const double* k_dev, const double* omega_dev,
                              double* su_out_dev, double* sp_out_dev)
{
    const std::string who = "mi_sst_k_terms";
    MICHK(sst_coeffs_check(who, coeffs));
    SstCell q{};
    q.K = *coeffs;
    const double* in[3] = {g_dev, k_dev, omega_dev};
    double* out[2] = {su_out_dev, sp_out_dev};
    return sst_cell_pass(who, c, n, k_sst_k_terms, q, in, 3, out, 2);
}

extern "C" int mi_sst_nut(mi_ctx_t c, int64_t n, const mi_sst_coeffs* coeffs, int f3, int constructor_form, const double* k_dev, const double* omega_dev,
                          const double* y_dev, const double* s_dev, const double* nu_dev_or_null, double nu_value, double* nut_out_dev,
                          double* f23_out_dev_or_null)
{
    const std::string who = "mi_sst_nut";
    MICHK(sst_coeffs_check(who, coeffs));
    if (!nu_dev_or_null && !ke_positive(nu_value)) return fail(MI_ERR_ARG, who + ": nu must be a finite number above zero");
    SstCell q{};
    q.K = *coeffs; q.ctor = constructor_form ? 1 : 0; q.nu = nu_value;
    const double* in[5] = {k_dev, omega_dev, y_dev, s_dev, nu_dev_or_null};
    double* out[2] = {nut_out_dev, f23_out_dev_or_null};
    auto kernel = nu_dev_or_null ? (f3 ? k_sst_nut<true, true> : k_sst_nut<true, false>) : (f3 ? k_sst_nut<false, true> : k_sst_nut<false, false>);
    return sst_cell_pass(who, c, n, kernel, q, in, nu_dev_or_null ? 5 : 4, out, 2, 1);
}

extern "C" int mi_sst_wall_cells(mi_ke_t h, const mi_sst_coeffs* coeffs, const mi_sst_wall* x)
{
    const std::string who = "mi_sst_wall_cells";
    MICHK(row_handle_check(who, h));
    MICHK(sst_coeffs_check(who, coeffs));
    if (!x) return fail(MI_ERR_ARG, who + ": the arrays are missing");
    if (h->nWallFaces == 0) return MI_OK;
    const double* in[11] = {x->k_dev, x->u_dev[0], x->u_dev[1], x->u_dev[2], x->b_uw_dev[0], x->b_uw_dev[1], x->b_uw_dev[2],
                            x->b_delta_coeffs_dev, x->b_y_dev, x->b_nuw_dev, x->b_nutw_dev};
    double* out[3] = {x->g_inout_dev, x->omega_inout_dev, x->b_omega_out_dev};
    MICHK(arrays_present(who, in, 11));
    MICHK(outputs_distinct(who, in, 11, out, 3));
    MICHK(arrays_aligned8(who, (const void* const*)in, 11));
    MICHK(arrays_aligned8(who, (const void* const*)out, 3));
    HIPCHK(hipSetDevice(h->ctx->device));
    SstWallArgs q{};
    q.cells = h->cells.p; q.start = h->start.p; q.faces = h->faces.p; q.weight = h->weight.p; q.nCells = h->nWallCells;
    q.Cmu25 = coeffs->Cmu25; q.kappa = coeffs->kappa; q.beta1 = coeffs->wallBeta1;
    q.k = x->k_dev; q.bdc = x->b_delta_coeffs_dev; q.by = x->b_y_dev; q.bnuw = x->b_nuw_dev; q.bnutw = x->b_nutw_dev;
    for (int d = 0; d < 3; ++d) { q.u[d] = x->u_dev[d]; q.buw[d] = x->b_uw_dev[d]; }
    q.G = x->g_inout_dev; q.omega = x->omega_inout_dev; q.bomega = x->b_omega_out_dev;
    k_sst_wall_cells<<<grid_for(h->ctx, h->nWallCells), 256, 0, h->ctx->stream>>>(q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
