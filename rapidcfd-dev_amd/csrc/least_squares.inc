// least_squares.inc -- the leastSquares gradient scheme (finiteVolume/gradSchemes/leastSquaresGrad; included by engine.hip after
// limited_grad.inc): the least-squares vectors, built once per mesh on the device, and the gradient, one row pass per evaluation.
//
// The reference's device code for this scheme cannot be the definition (DESIGN 3.5i, SURVEY Appendix B): its gradient writes through a
// permutation iterator whose indices repeat, its vectors file does not compile.  What those files keep of the upstream algorithm is:
//   vectors   leastSquaresVectors.C:123-225, host loops: dd summed over the internal faces in face order (owner and neighbour side), then
//             the patches in patch order; inv(dd) in the host Field<symmTensor> form (symmTensorField.C:50-105: caller cell 0 alone decides
//             removeCmpts); then every face's vectors.  Every expression is rounded operation by operation as written (DESIGN 3.5c), which
//             -ffp-contract=off gives plain expressions.
//   gradient  the loop kept in the comment of leastSquaresGrad.C:109-118, then the patches (:139-189), with the arithmetic of the device
//             functor leastSquaresCalcGradFunctor (:39-53) contracted as DESIGN 3.5a contracts every device functor: delta = a - b
//             rounded once, then one fma per gradient component.
// Both are restated, not pinned by a compiled reference (tests/test_least_squares_grad.py holds the restatement).
// A cell sees its faces in the order those loops reach it on owner-sorted addressing: neighbour side (losort, ascending), own faces
// ascending, boundary faces by patch then face -- the order of k_limited_grad.
namespace mi {

// sqr(d) scaled by s (SymmTensorI.H:546-554, then scalar*SymmTensor per component): xx xy xz yy yz zz
__device__ __forceinline__ void ls_wdd(double s, double dx, double dy, double dz, double* t)
{
    t[0] = s * (dx * dx); t[1] = s * (dx * dy); t[2] = s * (dx * dz); t[3] = s * (dy * dy); t[4] = s * (dy * dz); t[5] = s * (dz * dz);
}
// magSqr(Vector) (VectorSpaceI.H:336-344): (x*x + y*y) + z*z
__device__ __forceinline__ double ls_magsqr(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

struct LsBuildArgs {
    RowTables r;
    const uint8_t* bCoupled;                          // per boundary face: 1 on a coupled patch
    const double *cc[3], *w, *magSf, *bw, *bMagSf, *bd[3];
    double* dd[6];                                    // xx xy xz yy yz zz; inverted in place by k_ls_invert
    double* dd0;                                      // caller cell 0's dd, six values (the read-back for removeCmpts)
    double *p[3], *nv[3], *bp[3];
    double add[6];                                    // removeCmpts as the tensor added before and subtracted after the inversion
    int removes;
    int nf;
};

// dd per cell (leastSquaresVectors.C:123-170): a thread owns a cell and adds its faces' terms in the loops' order
__global__ __launch_bounds__(256) void k_ls_dd(const LsBuildArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.r.n) return;
    const double cx = a.cc[0][c], cy = a.cc[1][c], cz = a.cc[2][c];
    double dd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6];
    for (int j = a.r.ls[c]; j < a.r.ls[c + 1]; ++j) {              // c is the neighbour: d = C[c] - C[own], dd[nei] += w*wdd
        const int f = a.r.losort[j], o = a.r.lo[f];
        const double dx = cx - a.cc[0][o], dy = cy - a.cc[1][o], dz = cz - a.cc[2][o];
        ls_wdd(a.magSf[f] / ls_magsqr(dx, dy, dz), dx, dy, dz, t);
        const double w = a.w[f];
#pragma unroll
        for (int i = 0; i < 6; ++i) dd[i] = dd[i] + w * t[i];
    }
    for (int f = a.r.os[c]; f < a.r.os[c + 1]; ++f) {              // c is the owner: d = C[nei] - C[c], dd[own] += (1 - w)*wdd
        const int u = a.r.up[f];
        const double dx = a.cc[0][u] - cx, dy = a.cc[1][u] - cy, dz = a.cc[2][u] - cz;
        ls_wdd(a.magSf[f] / ls_magsqr(dx, dy, dz), dx, dy, dz, t);
        const double w1 = 1.0 - a.w[f];
#pragma unroll
        for (int i = 0; i < 6; ++i) dd[i] = dd[i] + w1 * t[i];
    }
    if (a.r.bStart) for (int j = a.r.bStart[c]; j < a.r.bStart[c + 1]; ++j) {
        const int bf = a.r.bFace[j];
        const double dx = a.bd[0][bf], dy = a.bd[1][bf], dz = a.bd[2][bf];
        const double m = ls_magsqr(dx, dy, dz);
        // coupled: ((1 - pw)*pMagSf/magSqr(d))*sqr(d) (:156-157); the others: (pMagSf/magSqr(d))*sqr(d) (:166-167)
        const double s = a.bCoupled[bf] ? (1.0 - a.bw[bf]) * a.bMagSf[bf] / m : a.bMagSf[bf] / m;
        ls_wdd(s, dx, dy, dz, t);
#pragma unroll
        for (int i = 0; i < 6; ++i) dd[i] = dd[i] + t[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) a.dd[i][c] = dd[i];
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.dd0[i] = dd[i];
    }
}

// inv(dd) per cell, in place (symmTensorField.C:65-104 around SymmTensorI.H:344-399): det, the cofactors, / detst; a removed component
// gets +1 before and -1 after, for every cell.  A cell without faces has dd = 0 and a non-finite inverse that no face reads.
__global__ __launch_bounds__(256) void k_ls_invert(const LsBuildArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.r.n) return;
    double xx = a.dd[0][c], xy = a.dd[1][c], xz = a.dd[2][c], yy = a.dd[3][c], yz = a.dd[4][c], zz = a.dd[5][c];
    if (a.removes) { xx = xx + a.add[0]; xy = xy + a.add[1]; xz = xz + a.add[2]; yy = yy + a.add[3]; yz = yz + a.add[4]; zz = zz + a.add[5]; }
    const double det = xx * yy * zz + xy * yz * xz + xz * xy * yz - xx * yz * yz - xy * xy * zz - xz * yy * xz;
    double r[6];
    r[0] = (yy * zz - yz * yz) / det; r[1] = (xz * yz - xy * zz) / det; r[2] = (xy * yz - xz * yy) / det;
    r[3] = (xx * zz - xz * xz) / det; r[4] = (xy * xz - xx * yz) / det; r[5] = (xx * yy - xy * xy) / det;
#pragma unroll
    for (int i = 0; i < 6; ++i) a.dd[i][c] = a.removes ? r[i] - a.add[i] : r[i];
}

// SymmTensor & Vector (SymmTensorI.H:248-256) of cell c's inverse
__device__ __forceinline__ void ls_inv_dot(const LsBuildArgs& a, int c, double dx, double dy, double dz, double* v)
{
    const double xx = a.dd[0][c], xy = a.dd[1][c], xz = a.dd[2][c], yy = a.dd[3][c], yz = a.dd[4][c], zz = a.dd[5][c];
    v[0] = xx * dx + xy * dy + xz * dz; v[1] = xy * dx + yy * dy + yz * dz; v[2] = xz * dx + yz * dy + zz * dz;
}
// pVectors / nVectors of the internal faces (leastSquaresVectors.C:178-188), one thread a face
__global__ __launch_bounds__(256) void k_ls_face_vectors(const LsBuildArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.nf) return;
    const int o = a.r.lo[f], u = a.r.up[f];
    const double dx = a.cc[0][u] - a.cc[0][o], dy = a.cc[1][u] - a.cc[1][o], dz = a.cc[2][u] - a.cc[2][o];
    const double m = a.magSf[f] / ls_magsqr(dx, dy, dz), w = a.w[f];
    const double sp = (1.0 - w) * m, sn = -w * m;
    double v[3];
    ls_inv_dot(a, o, dx, dy, dz, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.p[k][f] = sp * v[k];
    ls_inv_dot(a, u, dx, dy, dz, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.nv[k][f] = sn * v[k];
}
// the boundary pVectors (leastSquaresVectors.C:190-225) through the per-cell lists: every boundary face belongs to one cell
__global__ __launch_bounds__(256) void k_ls_boundary_vectors(const LsBuildArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.r.n) return;
    for (int j = a.r.bStart[c]; j < a.r.bStart[c + 1]; ++j) {
        const int bf = a.r.bFace[j];
        const double dx = a.bd[0][bf], dy = a.bd[1][bf], dz = a.bd[2][bf];
        const double m = ls_magsqr(dx, dy, dz);
        const double s = a.bCoupled[bf] ? (1.0 - a.bw[bf]) * a.bMagSf[bf] / m : a.bMagSf[bf] * (1.0 / m);
        double v[3];
        ls_inv_dot(a, c, dx, dy, dz, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.bp[k][bf] = s * v[k];
    }
}

struct LsGradArgs {
    RowTables r;
    const double *p[3], *nv[3], *bp[3], *vf[3], *bv[3];
    double* g[9];                                     // g[3*j + k] = d(vf_j)/dx_k
};
// the gradient: k_gauss_grad's skeleton with the block's own-face pVectors staged, nVectors and the owner's vf gathered for the
// neighbour-side faces (the first four before the barrier), the boundary faces through the per-cell lists
template <int NC, int BS>
__global__ __launch_bounds__(BS) void k_ls_grad(const LsGradArgs a)
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
    if (staged) { stage_dma8<BS>(a.p[0] + f0, sx, nf, tid); stage_dma8<BS>(a.p[1] + f0, sy, nf, tid); stage_dma8<BS>(a.p[2] + f0, sz, nf, tid); }
    int nb = 0, ne = 0;
    if (live) { nb = a.r.ls[c]; ne = a.r.ls[c + 1]; }
    const int cnt = ne - nb;
    double nx[4], ny[4], nz[4], no[4][NC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
            const int f = a.r.losort[nb + k], o = a.r.lo[f];
            nx[k] = a.nv[0][f]; ny[k] = a.nv[1][f]; nz[k] = a.nv[2][f];
#pragma unroll
            for (int j = 0; j < NC; ++j) no[k][j] = a.vf[j][o];
        } else {
            nx[k] = ny[k] = nz[k] = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) no[k][j] = 0.0;
        }
    }
    __syncthreads();
    if (!live) return;
    double v[NC], g[3 * NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = a.vf[j][c];
#pragma unroll
    for (int i = 0; i < 3 * NC; ++i) g[i] = 0.0;
    // lsGrad[nei] -= neiLs*(vsf[nei] - vsf[own])
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double d = v[j] - no[k][j];
            g[3 * j] = fma(-nx[k], d, g[3 * j]); g[3 * j + 1] = fma(-ny[k], d, g[3 * j + 1]); g[3 * j + 2] = fma(-nz[k], d, g[3 * j + 2]);
        }
    }
    for (int i = nb + 4; i < ne; ++i) {
        const int f = a.r.losort[i], o = a.r.lo[f];
        const double lx = a.nv[0][f], ly = a.nv[1][f], lz = a.nv[2][f];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double d = v[j] - a.vf[j][o];
            g[3 * j] = fma(-lx, d, g[3 * j]); g[3 * j + 1] = fma(-ly, d, g[3 * j + 1]); g[3 * j + 2] = fma(-lz, d, g[3 * j + 2]);
        }
    }
    // lsGrad[own] += ownLs*(vsf[nei] - vsf[own])
    const int ob = a.r.os[c], oe = a.r.os[c + 1];
    for (int f = ob; f < oe; ++f) {
        double lx, ly, lz;
        if (staged) { lx = sx[f - f0]; ly = sy[f - f0]; lz = sz[f - f0]; }
        else { lx = a.p[0][f]; ly = a.p[1][f]; lz = a.p[2][f]; }
        const int u = a.r.up[f];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double d = a.vf[j][u] - v[j];
            g[3 * j] = fma(lx, d, g[3 * j]); g[3 * j + 1] = fma(ly, d, g[3 * j + 1]); g[3 * j + 2] = fma(lz, d, g[3 * j + 2]);
        }
    }
    // the patches: lsGrad[faceCells] += patchOwnLs*(neiVsf | patchVsf - vsf[faceCells])
    if (a.r.bStart) for (int i = a.r.bStart[c]; i < a.r.bStart[c + 1]; ++i) {
        const int bf = a.r.bFace[i];
        const double lx = a.bp[0][bf], ly = a.bp[1][bf], lz = a.bp[2][bf];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double d = a.bv[j][bf] - v[j];
            g[3 * j] = fma(lx, d, g[3 * j]); g[3 * j + 1] = fma(ly, d, g[3 * j + 1]); g[3 * j + 2] = fma(lz, d, g[3 * j + 2]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3 * NC; ++i) a.g[i][c] = g[i];
}

} // namespace mi

// the least-squares vectors of one mesh: pVectors / nVectors on the internal faces, pVectors on the boundary faces, caller's face order
struct mi_ls_vectors_s : RowHandle {
    DevBuf<double> p[3], nv[3], bp[3];
};

extern "C" int mi_grad_scheme_parse(const char* scheme, mi_grad_scheme* out)
{
    const char* who = "mi_grad_scheme_parse";
    if (!scheme || !out) return fail(MI_ERR_ARG, std::string(who) + ": bad argument");
    const std::vector<std::string> tok = scheme_words(scheme);
    if (tok.empty()) return fail(MI_ERR_ARG, std::string(who) + ": empty scheme");
    mi_grad_scheme g{};
    const int kind = grad_lim_kind(tok[0]);
    const size_t b = kind >= 0 ? 1 : 0;               // where the base scheme starts
    if (kind >= 0) {
        if (tok.size() < 2) return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[0] + "' needs a base gradient scheme and a coefficient");
        if (grad_lim_kind(tok[1]) >= 0) return fail(MI_ERR_ARG, std::string(who) + ": a limited scheme over a limited scheme ('" + tok[1] + "') is not supported");
    }
    size_t next;                                      // the first token after the base scheme
    if (tok[b] == "Gauss") {
        if (tok.size() < b + 2) return fail(MI_ERR_ARG, std::string(who) + ": Gauss needs an interpolation scheme");
        if (tok[b + 1] != "linear") return fail(MI_ERR_ARG, std::string(who) + ": interpolation scheme '" + tok[b + 1] + "' is not supported (only linear)");
        g.base = MI_GRAD_BASE_GAUSS_LINEAR; next = b + 2;
    } else if (tok[b] == "leastSquares") {
        g.base = MI_GRAD_BASE_LEAST_SQUARES; next = b + 1;
    } else {
        return fail(MI_ERR_ARG, std::string(who) + ": " + (kind >= 0 ? "base " : "") + "gradient scheme '" + tok[b] + "' is not supported (only Gauss linear and leastSquares)");
    }
    if (kind < 0) {
        if (tok.size() > next) return fail(MI_ERR_ARG, std::string(who) + ": extra '" + tok[next] + "'");
        *out = g;
        return MI_OK;
    }
    if (tok.size() < next + 1) return fail(MI_ERR_ARG, std::string(who) + ": '" + tok[0] + "' needs the coefficient k");
    if (tok.size() > next + 1) return fail(MI_ERR_ARG, std::string(who) + ": extra '" + tok[next + 1] + "'");
    g.limited = 1;
    MICHK(grad_lim_fill(who, kind, tok[next], &g.limiter));
    *out = g;
    return MI_OK;
}

namespace {
template <int NC>
int ls_grad_launch(mi_addr_s* a, LsGradArgs& q) { return row_launch_bs(a, 3, k_ls_grad<NC, 256>, k_ls_grad<NC, 512>, k_ls_grad<NC, 1024>, q); }
} // namespace

extern "C" int mi_ls_vectors_create(mi_addr_t a, mi_grad_boundary_t b, const double* const* c_dev, const double* weights_dev, const double* mag_sf_dev,
                                    const double* b_weights_dev, const double* b_mag_sf_dev, const double* const* b_delta_dev, mi_ls_vectors_t* out)
{
    const std::string who = "mi_ls_vectors_create";
    std::unique_ptr<mi_ls_vectors_s> v(new mi_ls_vectors_s());
    MICHK(row_handle_open(who, a, b, out, *v));
    const int32_t n = v->nCells, nf = v->nFaces, nb = v->nBFaces;
    if (n > 0 && (!c_dev || !c_dev[0] || !c_dev[1] || !c_dev[2])) return fail(MI_ERR_ARG, who + ": the cell centres are missing");
    if (nf > 0 && (!weights_dev || !mag_sf_dev)) return fail(MI_ERR_ARG, who + ": the face weights and magSf are missing");
    int64_t nCoupled = 0;
    if (b) for (size_t p = 0; p < b->patchSizes.size(); ++p) if (b->patchKinds[p] == MI_GRAD_PATCH_COUPLED) nCoupled += b->patchSizes[p];
    if (nb > 0 && (!b_mag_sf_dev || !b_delta_dev || !b_delta_dev[0] || !b_delta_dev[1] || !b_delta_dev[2] || (nCoupled > 0 && !b_weights_dev)))
        return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary weights, magSf and delta needed");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    hipStream_t s = a->ctx->stream;
    for (int k = 0; k < 3; ++k) {
        if (nf > 0) { MICHK(v->p[k].alloc((size_t)nf)); MICHK(v->nv[k].alloc((size_t)nf)); }
        if (nb > 0) MICHK(v->bp[k].alloc((size_t)nb));
    }
    if (n == 0) { *out = v.release(); return MI_OK; }
    DevBuf<double> dd;                                // six cell arrays and caller cell 0's six values
    DevBuf<uint8_t> coupled;
    MICHK(dd.alloc((size_t)6 * n + 6));
    LsBuildArgs q{};
    q.r = row_tables(a, b);
    if (nb > 0) {
        MICHK(coupled.alloc((size_t)nb));
        HIPCHK(hipMemsetAsync(coupled.p, 0, (size_t)nb, s));
        size_t off = 0;
        for (size_t p = 0; p < b->patchSizes.size(); ++p) {
            if (b->patchKinds[p] == MI_GRAD_PATCH_COUPLED && b->patchSizes[p] > 0) HIPCHK(hipMemsetAsync(coupled.p + off, 1, (size_t)b->patchSizes[p], s));
            off += (size_t)b->patchSizes[p];
        }
        q.bCoupled = coupled.p;
        q.bw = b_weights_dev; q.bMagSf = b_mag_sf_dev;
        for (int k = 0; k < 3; ++k) { q.bd[k] = b_delta_dev[k]; q.bp[k] = v->bp[k].p; }
    }
    q.w = weights_dev; q.magSf = mag_sf_dev;
    for (int k = 0; k < 3; ++k) { q.cc[k] = c_dev[k]; q.p[k] = v->p[k].p; q.nv[k] = v->nv[k].p; }
    for (int i = 0; i < 6; ++i) q.dd[i] = dd.p + (size_t)i * n;
    q.dd0 = dd.p + (size_t)6 * n;
    q.nf = nf;
    const int cellBlocks = (n + 255) / 256;
    k_ls_dd<<<cellBlocks, 256, 0, s>>>(q);
    HIPCHK(hipGetLastError());
    // removeCmpts from caller cell 0 alone (symmTensorField.C:57-63; magSqr(SymmTensor) SymmTensorI.H:276-284; SMALL = 1e-15)
    double t[6];
    HIPCHK(hipMemcpyAsync(t, q.dd0, sizeof t, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double scale = t[0] * t[0] + 2 * (t[1] * t[1]) + 2 * (t[2] * t[2]) + t[3] * t[3] + 2 * (t[4] * t[4]) + t[5] * t[5];
    const bool rm[3] = {t[0] * t[0] / scale < 1.0e-15, t[3] * t[3] / scale < 1.0e-15, t[5] * t[5] / scale < 1.0e-15};
    const int diag[3] = {0, 3, 5};
    for (int d = 0; d < 3; ++d) if (rm[d]) { q.removes = 1; q.add[diag[d]] = 1.0; }
    k_ls_invert<<<cellBlocks, 256, 0, s>>>(q);
    HIPCHK(hipGetLastError());
    if (nf > 0) { k_ls_face_vectors<<<(nf + 255) / 256, 256, 0, s>>>(q); HIPCHK(hipGetLastError()); }
    if (nb > 0) { k_ls_boundary_vectors<<<cellBlocks, 256, 0, s>>>(q); HIPCHK(hipGetLastError()); }
    HIPCHK(hipStreamSynchronize(s));                  // dd and the coupled marks are released here
    *out = v.release();
    return MI_OK;
}
extern "C" int mi_ls_vectors_destroy(mi_ls_vectors_t v) { delete v; return MI_OK; }

extern "C" int mi_ls_vectors_fields(mi_ls_vectors_t v, double* const* p_out_dev, double* const* n_out_dev, double* const* bp_out_dev_or_null)
{
    const std::string who = "mi_ls_vectors_fields";
    if (!v) return fail(MI_ERR_ARG, who + ": bad argument");
    if (!p_out_dev || !n_out_dev) return fail(MI_ERR_ARG, who + ": output arrays missing");
    if (v->nBFaces > 0 && !bp_out_dev_or_null) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary output arrays needed");
    const double* in[9];
    double* outs[9];
    int nIn = 0, nOut = 0;
    for (int k = 0; k < 3; ++k) {
        if (v->nFaces > 0) { in[nIn++] = v->p[k].p; in[nIn++] = v->nv[k].p; }
        if (v->nBFaces > 0) in[nIn++] = v->bp[k].p;
    }
    if (v->nFaces > 0) for (int k = 0; k < 3; ++k) { outs[nOut++] = p_out_dev[k]; outs[nOut++] = n_out_dev[k]; }
    if (v->nBFaces > 0) for (int k = 0; k < 3; ++k) outs[nOut++] = bp_out_dev_or_null[k];
    MICHK(outputs_distinct(who, in, nIn, outs, nOut));
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    for (int k = 0; k < 3; ++k) {
        if (v->nFaces > 0) {
            HIPCHK(hipMemcpyAsync(p_out_dev[k], v->p[k].p, (size_t)v->nFaces * sizeof(double), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(n_out_dev[k], v->nv[k].p, (size_t)v->nFaces * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        if (v->nBFaces > 0) HIPCHK(hipMemcpyAsync(bp_out_dev_or_null[k], v->bp[k].p, (size_t)v->nBFaces * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    return MI_OK;
}

extern "C" int mi_ls_grad(mi_ls_vectors_t v, int32_t n_comp, const double* const* vf_dev, const double* const* bvalue_dev_or_null, double* const* grad_out_dev)
{
    const std::string who = "mi_ls_grad";
    if (!v) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n_comp != 1 && n_comp != 3) return fail(MI_ERR_ARG, who + ": n_comp must be 1 or 3");
    mi_addr_s* a = v->addr;
    MICHK(row_handle_check(who, v, "the vectors were"));
    if (!vf_dev || !grad_out_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    const bool hasB = v->nBFaces > 0;
    if (hasB && !bvalue_dev_or_null) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary values needed");
    const double* in[15];
    int nIn = 0;
    for (int j = 0; j < n_comp; ++j) { in[nIn++] = vf_dev[j]; if (hasB) in[nIn++] = bvalue_dev_or_null[j]; }
    MICHK(arrays_present(who, in, nIn));
    for (int k = 0; k < 3; ++k) {
        if (v->nFaces > 0) { in[nIn++] = v->p[k].p; in[nIn++] = v->nv[k].p; }
        if (hasB) in[nIn++] = v->bp[k].p;
    }
    MICHK(outputs_distinct(who, in, nIn, grad_out_dev, 3 * n_comp));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    if (a->L.nCells == 0) return MI_OK;
    LsGradArgs q{};
    q.r = row_tables(a, v->boundary);
    for (int k = 0; k < 3; ++k) { q.p[k] = v->p[k].p; q.nv[k] = v->nv[k].p; q.bp[k] = v->bp[k].p; }
    for (int j = 0; j < n_comp; ++j) { q.vf[j] = vf_dev[j]; if (hasB) q.bv[j] = bvalue_dev_or_null[j]; }
    for (int i = 0; i < 3 * n_comp; ++i) q.g[i] = grad_out_dev[i];
    return n_comp == 1 ? ls_grad_launch<1>(a, q) : ls_grad_launch<3>(a, q);
}
