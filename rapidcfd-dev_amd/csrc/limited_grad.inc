// limited_grad.inc -- the limited gradient schemes cellLimited / cellMDLimited / faceLimited / faceMDLimited (included by engine.hip after
// row_entry.inc).
//
// The reference limits `Gauss linear` gradients with host loops over owner / neighbour that scatter to both cells of every face
// (finiteVolume/gradSchemes/limitedGradSchemes/*/*Grads.C).  Here it is ONE row pass on the skeleton of k_gauss_grad: a thread owns a
// cell, walks its faces in the order the reference visits them for that cell -- neighbour side (losort: ascending faces, whose owners are
// lower), own faces ascending, boundary faces by patch then face -- and reads and writes its own cell's gradient only.  The pass works in
// place, with no atomics and no scratch.  Rounding: these loops are host code in the reference, every expression is rounded operation by
// operation as written (DESIGN 3.5c), which the engine's -ffp-contract=off gives plain expressions.
namespace mi {

enum { LG_CELL = 0, LG_CELL_MD = 1, LG_FACE = 2, LG_FACE_MD = 3 };   // MI_GRAD_CELL_LIMITED ... MI_GRAD_FACE_MD_LIMITED
struct LGradArgs {
    RowTables r;                                      // the boundary lists: all faces for the cell kinds, the limited ones for the face kinds
    const double *cf[3], *cc[3], *bcf[3], *vf[3], *bv[3];
    double *g[9], *limOut[3];                         // g[3*j + k] = d(vf_j)/dx_k, in place
    double rk;                                        // 1.0/k - 1.0
    int expand;                                       // k < 1: the cell kinds' and faceMDLimited's expansion of the bounds
};
// Foam::max / Foam::min (the first argument wins a tie: signed zeros keep the reference's order)
__device__ __forceinline__ double lg_max(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double lg_min(double a, double b) { return a < b ? a : b; }
// Vector & Vector as the host compiles it: (ax*bx + ay*by) + az*bz, three products and two sums each rounded
__device__ __forceinline__ double lg_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
// cellLimitedGrad<scalar>::limitFace (cellLimitedGrad.H:136-171) = faceLimitedGrad::limitFace (faceLimitedGrad.H:140-156); VSMALL = 1e-300
__device__ __forceinline__ void lg_limit(double& lim, double maxD, double minD, double e)
{
    if (e > maxD + 1.0e-300) lim = lg_min(lim, maxD / e);
    else if (e < minD - 1.0e-300) lim = lg_min(lim, minD / e);
}
// cellMDLimitedGrad<scalar>::limitFace (cellMDLimitedGrad.H:136-154) on the gradient gi of one component: g = g + dcf*(maxD - e)/magSqr(dcf)
__device__ __forceinline__ void lg_md(double* gi, double maxD, double minD, double dx, double dy, double dz)
{
    const double e = lg_dot(dx, dy, dz, gi[0], gi[1], gi[2]);
    double t;
    if (e > maxD) t = maxD - e;
    else if (e < minD) t = minD - e;
    else return;
    const double m = lg_dot(dx, dy, dz, dx, dy, dz);
    gi[0] = gi[0] + dx * t / m; gi[1] = gi[1] + dy * t / m; gi[2] = gi[2] + dz * t / m;
}

template <int KIND, int NC, int BS>
__global__ __launch_bounds__(BS) void k_limited_grad(const LGradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    double *sx = rp_smem, *sy = sx + a.r.cap, *sz = sy + a.r.cap;
    const int lb = a.r.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.r.blockStart) { c0 = a.r.blockStart[lb]; cEnd = a.r.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.r.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.r.os[c0], nf = a.r.os[cEnd] - f0;
    const bool staged = nf <= a.r.cap;
    if (staged) { stage_dma8<BS>(a.cf[0] + f0, sx, nf, tid); stage_dma8<BS>(a.cf[1] + f0, sy, nf, tid); stage_dma8<BS>(a.cf[2] + f0, sz, nf, tid); }
    int nb = 0, ne = 0;
    if (live) { nb = a.r.ls[c]; ne = a.r.ls[c + 1]; }
    const int cnt = ne - nb;
    // the first four neighbour-side faces, their owners and -- when they are not in the block's staged range -- their centres
    int nfk[4], nok[4]; double nx[4], ny[4], nz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nfk[k] = (k < cnt) ? a.r.losort[nb + k] : 0;
        nok[k] = (k < cnt) ? a.r.lo[nfk[k]] : 0;
        if (k < cnt && (!staged || nfk[k] < f0)) { const int f = nfk[k]; nx[k] = a.cf[0][f]; ny[k] = a.cf[1][f]; nz[k] = a.cf[2][f]; }
        else { nx[k] = ny[k] = nz[k] = 0.0; }
    }
    __syncthreads();
    if (!live) return;
    const double cx = a.cc[0][c], cy = a.cc[1][c], cz = a.cc[2][c];
    double v[NC], g[3 * NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = a.vf[j][c];
#pragma unroll
    for (int i = 0; i < 3 * NC; ++i) g[i] = a.g[i][c];
    const int ob = a.r.os[c], oe = a.r.os[c + 1];
    const int bb = a.r.bStart ? a.r.bStart[c] : 0, be = a.r.bStart ? a.r.bStart[c + 1] : 0;
    // every face of the cell in the reference's order: fn(dcf = Cf - C[c] per component, the value across the face is o[j][i], c owns the face)
    auto walk = [&](auto&& fn) {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < cnt) {
            double fx = nx[k], fy = ny[k], fz = nz[k];
            if (staged && nfk[k] >= f0) { const int j = nfk[k] - f0; fx = sx[j]; fy = sy[j]; fz = sz[j]; }
            fn(fx - cx, fy - cy, fz - cz, a.vf, nok[k], false);
        }
        for (int j = nb + 4; j < ne; ++j) {
            const int f = a.r.losort[j];
            double fx, fy, fz;
            if (staged && f >= f0) { fx = sx[f - f0]; fy = sy[f - f0]; fz = sz[f - f0]; }
            else { fx = a.cf[0][f]; fy = a.cf[1][f]; fz = a.cf[2][f]; }
            fn(fx - cx, fy - cy, fz - cz, a.vf, a.r.lo[f], false);
        }
        for (int f = ob; f < oe; ++f) {
            double fx, fy, fz;
            if (staged) { fx = sx[f - f0]; fy = sy[f - f0]; fz = sz[f - f0]; }
            else { fx = a.cf[0][f]; fy = a.cf[1][f]; fz = a.cf[2][f]; }
            fn(fx - cx, fy - cy, fz - cz, a.vf, a.r.up[f], true);
        }
        for (int j = bb; j < be; ++j) {
            const int bf = a.r.bFace[j];
            fn(a.bcf[0][bf] - cx, a.bcf[1][bf] - cy, a.bcf[2][bf] - cz, a.bv, bf, true);
        }
    };
    if (KIND == LG_CELL || KIND == LG_CELL_MD) {
        // cellLimitedGrads.C:71-139: the cell's bounds over every neighbour value, made relative, expanded by (1/k - 1)*(max - min) when k < 1
        double mx[NC], mn[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) mx[j] = mn[j] = v[j];
        walk([&](double, double, double, const double* const* o, int i, bool) {
#pragma unroll
            for (int j = 0; j < NC; ++j) { const double w = o[j][i]; mx[j] = lg_max(mx[j], w); mn[j] = lg_min(mn[j], w); }
        });
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            mx[j] = mx[j] - v[j]; mn[j] = mn[j] - v[j];
            if (a.expand) { const double t = a.rk * (mx[j] - mn[j]); mx[j] = mx[j] + t; mn[j] = mn[j] - t; }
        }
        if (KIND == LG_CELL) {
            // cellLimitedGrads.C:141-190: a limiter per component, extrapolate = (Cf - C) & g; then g *= limiter (vector: cmptMultiply per row)
            double lim[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) lim[j] = 1.0;
            walk([&](double dx, double dy, double dz, const double* const*, int, bool) {
#pragma unroll
                for (int j = 0; j < NC; ++j) lg_limit(lim[j], mx[j], mn[j], lg_dot(dx, dy, dz, g[3 * j], g[3 * j + 1], g[3 * j + 2]));
            });
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                g[3 * j] = g[3 * j] * lim[j]; g[3 * j + 1] = g[3 * j + 1] * lim[j]; g[3 * j + 2] = g[3 * j + 2] * lim[j];
                if (a.limOut[0]) a.limOut[j][c] = lim[j];
            }
        } else {
            // cellMDLimitedGrads.C:137-183: every face moves g directly, one component's gradient at a time
            walk([&](double dx, double dy, double dz, const double* const*, int, bool) {
#pragma unroll
                for (int j = 0; j < NC; ++j) lg_md(g + 3 * j, mx[j], mn[j], dx, dy, dz);
            });
        }
    } else {
        // faceLimitedGrads.C / faceMDLimitedGrads.C: bounds per face from the face's (owner, neighbour) values, one loop
        double lim = 1.0;
        walk([&](double dx, double dy, double dz, const double* const* o, int i, bool own) {
            if (KIND == LG_FACE && NC == 3) {
                // faceLimitedGrads.C:216-254: gradf = dcf & g, vsfOwn / vsfNei = gradf & (owner / neighbour value), extrapolate magSqr(gradf);
                // on the neighbour side of an internal face the bounds are not expanded
                const double gf0 = lg_dot(dx, dy, dz, g[0], g[1], g[2]), gf1 = lg_dot(dx, dy, dz, g[3], g[4], g[5]), gf2 = lg_dot(dx, dy, dz, g[6], g[7], g[8]);
                const double sc = lg_dot(gf0, gf1, gf2, v[0], v[1], v[2]), so = lg_dot(gf0, gf1, gf2, o[0][i], o[1][i], o[2][i]);
                const double sOwn = own ? sc : so, sNei = own ? so : sc;
                double mxF = lg_max(sOwn, sNei), mnF = lg_min(sOwn, sNei);
                if (own) { const double t = a.rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t; }
                lg_limit(lim, mxF - sc, mnF - sc, lg_dot(gf0, gf1, gf2, gf0, gf1, gf2));
            } else {
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const double w = o[j][i];
                    const double pOwn = own ? v[j] : w, pNei = own ? w : v[j];
                    double mxF = lg_max(pOwn, pNei), mnF = lg_min(pOwn, pNei);
                    if (KIND == LG_FACE || a.expand) { const double t = a.rk * (mxF - mnF); mxF = mxF + t; mnF = mnF - t; }
                    if (KIND == LG_FACE) lg_limit(lim, mxF - v[j], mnF - v[j], lg_dot(dx, dy, dz, g[3 * j], g[3 * j + 1], g[3 * j + 2]));
                    else lg_md(g + 3 * j, mxF - v[j], mnF - v[j], dx, dy, dz);
                }
            }
        });
        if (KIND == LG_FACE) {
#pragma unroll
            for (int i = 0; i < 3 * NC; ++i) g[i] = g[i] * lim;
            if (a.limOut[0]) a.limOut[0][c] = lim;
        }
    }
#pragma unroll
    for (int i = 0; i < 3 * NC; ++i) a.g[i][c] = g[i];
}

} // namespace mi

namespace {
template <int KIND, int NC>
int lg_launch(mi_addr_s* a, LGradArgs& q)
{
    return row_launch_bs(a, 3, k_limited_grad<KIND, NC, 256>, k_limited_grad<KIND, NC, 512>, k_limited_grad<KIND, NC, 1024>, q);
}
template <int KIND>
int lg_launch_kind(mi_addr_s* a, LGradArgs& q, int nc) { return nc == 1 ? lg_launch<KIND, 1>(a, q) : lg_launch<KIND, 3>(a, q); }
const char* const kGradLimNames[] = {"cellLimited", "cellMDLimited", "faceLimited", "faceMDLimited"};
// the constructors' check (cellLimitedGrad.H:94-107 and its siblings) on a caller-filled mi_grad_limiter
int grad_lim_check(const char* who, const mi_grad_limiter* l)
{
    if (!l || l->kind < MI_GRAD_CELL_LIMITED || l->kind > MI_GRAD_FACE_MD_LIMITED) return fail(MI_ERR_ARG, std::string(who) + ": invalid mi_grad_limiter");
    if (!(l->k >= 0 && l->k <= 1)) return fail(MI_ERR_ARG, std::string(who) + ": coefficient k should be >= 0 and <= 1");
    if (l->identity != (l->k < 1.0e-15 ? 1 : 0)) return fail(MI_ERR_ARG, std::string(who) + ": identity must be k < SMALL");
    return MI_OK;
}
int grad_lim_kind(const std::string& s) { for (int k = 0; k < 4; ++k) if (s == kGradLimNames[k]) return k; return -1; }
// the coefficient token of a limited scheme (readScalar, then the constructors' range check)
int grad_lim_fill(const char* who, int kind, const std::string& ktok, mi_grad_limiter* out)
{
    double k = 0;
    if (!scheme_number(ktok, k)) return fail(MI_ERR_ARG, std::string(who) + ": '" + ktok + "' is not a number");
    mi_grad_limiter l{};
    l.kind = kind; l.k = k; l.identity = k < 1.0e-15 ? 1 : 0;
    MICHK(grad_lim_check(who, &l));
    *out = l;
    return MI_OK;
}
} // namespace

extern "C" int mi_grad_limiter_parse(const char* scheme, mi_grad_limiter* out)
{
    const char* who = "mi_grad_limiter_parse";
    if (!scheme || !out) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, std::string(who) + ": empty scheme");
    auto kind_of = grad_lim_kind;
    const int kind = kind_of(tok[0]);
    if (kind < 0) return fail(MI_ERR_ARG, std::string(who) + ": unknown limited gradient scheme '" + tok[0] + "'");
    if (tok.size() < 2) return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[0] + "' needs a base gradient scheme and a coefficient");
    if (kind_of(tok[1]) >= 0) return fail(MI_ERR_ARG, std::string(who) + ": a limited scheme over a limited scheme ('" + tok[1] + "') is not supported");
    if (tok[1] != "Gauss") return fail(MI_ERR_ARG, std::string(who) + ": base gradient scheme '" + tok[1] + "' is not supported (only Gauss)");
    if (tok.size() < 3) return fail(MI_ERR_ARG, std::string(who) + ": Gauss needs an interpolation scheme");
    if (tok[2] != "linear") return fail(MI_ERR_ARG, std::string(who) + ": interpolation scheme '" + tok[2] + "' is not supported (only linear)");
    if (tok.size() < 4) return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[0] + "' needs the coefficient k");
    if (tok.size() > 4) return fail(MI_ERR_ARG, std::string(who) + ": extra '" + tok[4] + "'");
    return grad_lim_fill(who, kind, tok[3], out);
}

extern "C" int mi_grad_boundary_create(mi_addr_t a, int32_t n_patches, const int32_t* patch_sizes, const int32_t* const* face_cells_host,
                                       const int32_t* patch_kinds, mi_grad_boundary_t* out)
{
    const char* who = "mi_grad_boundary_create";
    if (!a || !out || n_patches < 0 || (n_patches > 0 && (!patch_sizes || !face_cells_host || !patch_kinds))) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const int32_t n = a->L.nCells;
    Table<int32_t> allStart((size_t)n + 1, 0), limStart((size_t)n + 1, 0);
    int64_t total = 0;
    for (int32_t p = 0; p < n_patches; ++p) {
        const int32_t m = patch_sizes[p], kind = patch_kinds[p];
        if (m < 0 || (m > 0 && !face_cells_host[p])) return fail(MI_ERR_ARG, std::string(who) + ": bad patch " + std::to_string(p));
        if (kind != MI_GRAD_PATCH_OTHER && kind != MI_GRAD_PATCH_COUPLED && kind != MI_GRAD_PATCH_FIXES_VALUE)
            return fail(MI_ERR_ARG, std::string(who) + ": bad kind of patch " + std::to_string(p));
        for (int32_t i = 0; i < m; ++i) {
            const int32_t c = face_cells_host[p][i];
            if (c < 0 || c >= n) return fail(MI_ERR_ARG, std::string(who) + ": faceCells out of range in patch " + std::to_string(p));
            ++allStart[(size_t)c + 1];
            if (kind != MI_GRAD_PATCH_OTHER) ++limStart[(size_t)c + 1];
        }
        total += m;
    }
    if (total > INT32_MAX) return fail(MI_ERR_ARG, std::string(who) + ": too many boundary faces");
    for (int32_t c = 0; c < n; ++c) { allStart[(size_t)c + 1] += allStart[c]; limStart[(size_t)c + 1] += limStart[c]; }
    Table<int32_t> all((size_t)allStart[n]), lim((size_t)limStart[n]);
    {
        Table<int32_t> ca(allStart.begin(), allStart.end() - 1), cl(limStart.begin(), limStart.end() - 1);
        int32_t off = 0;                                  // each cell's entries in patch order, faces in patch order
        for (int32_t p = 0; p < n_patches; ++p) {
            for (int32_t i = 0; i < patch_sizes[p]; ++i) {
                const int32_t c = face_cells_host[p][i];
                all[(size_t)ca[c]++] = off + i;
                if (patch_kinds[p] != MI_GRAD_PATCH_OTHER) lim[(size_t)cl[c]++] = off + i;
            }
            off += patch_sizes[p];
        }
    }
    HIPCHK(hipSetDevice(a->ctx->device));
    mi_grad_boundary_s* b = new mi_grad_boundary_s();
    b->ctx = a->ctx; b->addr = a; b->nCells = n; b->nFaces = (int32_t)total; b->nLimited = limStart[n];
    if (n_patches > 0) { b->patchSizes.assign(patch_sizes, patch_sizes + n_patches); b->patchKinds.assign(patch_kinds, patch_kinds + n_patches); }
    hipStream_t s = a->ctx->stream;
    int r = MI_OK;
    if (b->nFaces > 0) { r = b->allStart.upload(allStart, s); if (r == MI_OK) r = b->all.upload(all, s); }
    if (r == MI_OK && b->nLimited > 0) { r = b->limStart.upload(limStart, s); if (r == MI_OK) r = b->lim.upload(lim, s); }
    if (r != MI_OK) { delete b; return r; }
    if (hipStreamSynchronize(s) != hipSuccess) { delete b; return fail(MI_ERR_DEVICE, std::string(who) + ": upload failed"); }
    *out = b;
    return MI_OK;
}
extern "C" int mi_grad_boundary_destroy(mi_grad_boundary_t b) { delete b; return MI_OK; }

extern "C" int mi_limited_grad(mi_addr_t a, const mi_grad_limiter* lim, mi_grad_boundary_t b, int32_t n_comp, const double* const* vf_dev,
                               const double* const* c_dev, const double* const* cf_dev, const double* const* bvalue_dev, const double* const* bcf_dev,
                               double* const* grad_inout_dev, double* const* limiter_out_dev_or_null)
{
    const char* who = "mi_limited_grad";
    if (!a) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    MICHK(grad_lim_check(who, lim));
    if (n_comp != 1 && n_comp != 3) return fail(MI_ERR_ARG, std::string(who) + ": n_comp must be 1 or 3");
    const bool md = lim->kind == MI_GRAD_CELL_MD_LIMITED || lim->kind == MI_GRAD_FACE_MD_LIMITED;
    if (md && limiter_out_dev_or_null) return fail(MI_ERR_ARG, std::string(who) + ": the MD kinds have no limiter field: limiter_out must be NULL");
    MICHK(boundary_matches(who, a, b));
    if (!vf_dev || !c_dev || !cf_dev || !grad_inout_dev) return fail(MI_ERR_ARG, std::string(who) + ": input arrays missing");
    const bool hasB = b && b->nFaces > 0;
    if (hasB && (!bvalue_dev || !bcf_dev)) return fail(MI_ERR_ARG, std::string(who) + ": the boundary has faces: boundary values and face centres needed");
    const int nLim = md ? 0 : (lim->kind == MI_GRAD_CELL_LIMITED ? n_comp : 1);
    const double* in[14];
    int m = 0;
    for (int j = 0; j < n_comp; ++j) in[m++] = vf_dev[j];
    for (int d = 0; d < 3; ++d) { in[m++] = c_dev[d]; if (a->L.nFaces > 0) in[m++] = cf_dev[d]; }   // no faces: the face centres are empty arrays (one_cell, tests/test_degenerate_meshes.py)
    if (hasB) { for (int j = 0; j < n_comp; ++j) in[m++] = bvalue_dev[j]; for (int d = 0; d < 3; ++d) in[m++] = bcf_dev[d]; }
    double* outs[12];
    int no = 0;
    for (int i = 0; i < 3 * n_comp; ++i) outs[no++] = grad_inout_dev[i];
    for (int j = 0; j < nLim && limiter_out_dev_or_null; ++j) outs[no++] = limiter_out_dev_or_null[j];
    MICHK(arrays_present(who, in, m));
    MICHK(outputs_distinct(who, in, m, outs, no));
    if (lim->identity) return MI_OK;                      // k < SMALL: the basic scheme's gradient unchanged (cellLimitedGrads.C:59-62)
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nCells == 0) return MI_OK;
    LGradArgs q{};
    const bool faceKind = lim->kind == MI_GRAD_FACE_LIMITED || lim->kind == MI_GRAD_FACE_MD_LIMITED;
    q.r = faceKind ? row_tables(a, b ? b->limStart.p : nullptr, b ? b->lim.p : nullptr) : row_tables(a, b);   // no limited face: no list
    for (int d = 0; d < 3; ++d) { q.cc[d] = c_dev[d]; q.cf[d] = cf_dev[d]; if (hasB) q.bcf[d] = bcf_dev[d]; }
    for (int j = 0; j < n_comp; ++j) { q.vf[j] = vf_dev[j]; if (hasB) q.bv[j] = bvalue_dev[j]; }
    for (int i = 0; i < 3 * n_comp; ++i) q.g[i] = grad_inout_dev[i];
    for (int j = 0; j < nLim && limiter_out_dev_or_null; ++j) q.limOut[j] = limiter_out_dev_or_null[j];
    q.rk = 1.0 / lim->k - 1.0;
    q.expand = lim->k < 1.0 ? 1 : 0;
    switch (lim->kind) {
    case MI_GRAD_CELL_LIMITED: return lg_launch_kind<LG_CELL>(a, q, n_comp);
    case MI_GRAD_CELL_MD_LIMITED: return lg_launch_kind<LG_CELL_MD>(a, q, n_comp);
    case MI_GRAD_FACE_LIMITED: return lg_launch_kind<LG_FACE>(a, q, n_comp);
    default: return lg_launch_kind<LG_FACE_MD>(a, q, n_comp);
    }
}
