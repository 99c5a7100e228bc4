// reconstruct.inc -- fvc::reconstruct of a surfaceScalarField and fvc::surfaceSum (included by engine.hip after least_squares.inc; DESIGN 3.5k).
//
//   reconstruct   fvcReconstruct.C:45-84: inv(surfaceSum(SfHat*Sf)) & surfaceSum(SfHat*ssf), SfHat = Sf/magSf (one division per component).
//                 The geometric tensor and its inverse are constants of a static mesh: they are built ONCE per mesh
//                 (mi_reconstruct_create) and the handle keeps the nine inverse components and SfHat; an evaluation is one row pass.
//   surfaceSum    fvcSurfaceIntegrate.C:262-360 with surfaceIntegrateFunctor<Type, false> (:40-132): every face term is ADDED, on the owner
//                 and on the neighbour side.  A cell meets its faces from +0.0: own faces ascending, neighbour-side faces in losort
//                 order, boundary faces by patch then by face within the patch.
//   inverse       tensorField.C:226-305: caller cell 0 alone decides removeCmpts (T.cc/magSqr(T) < SMALL, the nine squares summed left to
//                 right); a removed component adds the whole tensor (1,0,0, 0,0,0, 0,0,0) ... to every cell before the inversion and
//                 subtracts it after; det TensorI.H:552-560 and the nine cofactor expressions / det of :588-604, uncontracted (an
//                 ASSUMPTION: the reference's functor is device code whose contraction cannot be pinned).
//   T & s         TensorI.H:409-420, contracted as every device dot product here is (DESIGN 3.5a / 3.5f; the same standing assumption):
//                 out_a = fma(R_az, s_z, fma(R_ax, s_x, R_ay*s_y)).
// Every other expression is rounded operation by operation (-ffp-contract=off): a product SfHat_a*Sf_b or SfHat_k*ssf is a stored field
// in the reference, rounded before it is added.  Restated in tests/reconstruct_support.py, not pinned by a compiled reference.
namespace mi {

struct RcBuildArgs {
    RowTables r;
    const double *sf[3], *magSf, *bsf[3], *bMagSf;
    double *hat[3], *bhat[3];                         // SfHat, internal and boundary faces
    double* T[9];                                     // xx xy xz yx yy yz zx zy zz; inverted in place by k_rc_invert
    double* T0;                                       // caller cell 0's tensor, nine values (the read-back for removeCmpts)
    double add[9];                                    // removeCmpts as the tensor added before and subtracted after the inversion
    int removes;
    int nf, nb;
};

// SfHat = Sf/magSf on the internal faces [0, nf) and the boundary faces [nf, nf + nb), one thread a face
__global__ __launch_bounds__(256) void k_rc_hat(const RcBuildArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nf) {
        const double m = a.magSf[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.hat[k][i] = a.sf[k][i] / m;
    } else if (i < (int64_t)a.nf + a.nb) {
        const int64_t j = i - a.nf;
        const double m = a.bMagSf[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.bhat[k][j] = a.bsf[k][j] / m;
    }
}

// T[c] = surfaceSum(SfHat*Sf): a thread owns a cell and adds its faces' outer products (TensorI.H:437-448, each product rounded) in
// surfaceSum's order
__global__ __launch_bounds__(256) void k_rc_tensor(const RcBuildArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.r.n) return;
    double T[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto add = [&](const double* const* hat, const double* const* sf, int f) {
        const double h[3] = {hat[0][f], hat[1][f], hat[2][f]}, s[3] = {sf[0][f], sf[1][f], sf[2][f]};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { const double p = h[i] * s[j]; T[3 * i + j] = T[3 * i + j] + p; }
    };
    for (int f = a.r.os[c]; f < a.r.os[c + 1]; ++f) add(a.hat, a.sf, f);
    for (int j = a.r.ls[c]; j < a.r.ls[c + 1]; ++j) add(a.hat, a.sf, a.r.losort[j]);
    if (a.r.bStart) for (int j = a.r.bStart[c]; j < a.r.bStart[c + 1]; ++j) add(a.bhat, a.bsf, a.r.bFace[j]);
#pragma unroll
    for (int i = 0; i < 9; ++i) a.T[i][c] = T[i];
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.T0[i] = T[i];
    }
}

// inv(T) per cell, in place (tensorField.C:253-304 around TensorI.H:552-560 and :588-604).  The added tensor's zeros are added too: a -0.0
// component becomes +0.0, as in k_ls_invert.  A cell without faces has T = 0, det = 0 and a non-finite inverse.
__global__ __launch_bounds__(256) void k_rc_invert(const RcBuildArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.r.n) return;
    double t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { t[i] = a.T[i][c]; if (a.removes) t[i] = t[i] + a.add[i]; }
    const double xx = t[0], xy = t[1], xz = t[2], yx = t[3], yy = t[4], yz = t[5], zx = t[6], zy = t[7], zz = t[8];
    const double det = xx * yy * zz + xy * yz * zx + xz * yx * zy - xx * yz * zy - xy * yx * zz - xz * yy * zx;
    double r[9];
    r[0] = (yy * zz - zy * yz) / det; r[1] = (xz * zy - xy * zz) / det; r[2] = (xy * yz - xz * yy) / det;
    r[3] = (zx * yz - yx * zz) / det; r[4] = (xx * zz - xz * zx) / det; r[5] = (yx * xz - xx * yz) / det;
    r[6] = (yx * zy - yy * zx) / det; r[7] = (xy * zx - xx * zy) / det; r[8] = (xx * yy - yx * xy) / det;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.T[i][c] = a.removes ? r[i] - a.add[i] : r[i];
}

struct RcArgs {
    RowTables r;
    const double *hat[3], *bhat[3], *ssf[4], *bssf[4], *inv[9];
    double* out[12];                                  // out[3*r + k]
    int nst;                                         // the first nst fluxes are staged beside SfHat; the others are read from global memory
};
// the evaluation: k_gauss_grad's skeleton with 3 + nst staged face arrays (SfHat and the fluxes of the block's own faces; nst = NRHS unless
// the largest block's faces do not fit the LDS budget with all of them), the first four neighbour-side faces in registers before the
// barrier, the boundary faces through the per-cell lists, and the stored inverse in the epilogue.  s_k += SfHat_k*ssf with the product
// rounded first; no division.
template <int BS, int NRHS>
__global__ __launch_bounds__(BS) void k_reconstruct(const RcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rp_smem[];
    double* sh = rp_smem;                             // sh + k*cap: SfHat_k (k < 3), flux k - 3
    const int lb = a.r.xcd ? xcd_block() : (int)blockIdx.x;
    int c0, cEnd;
    if (a.r.blockStart) { c0 = a.r.blockStart[lb]; cEnd = a.r.blockStart[lb + 1]; }
    else { c0 = lb * BS; cEnd = min(c0 + BS, a.r.n); }
    const int tid = threadIdx.x, c = c0 + tid;
    const bool live = c < cEnd;
    const int f0 = a.r.os[c0], nf = a.r.os[cEnd] - f0;
    const bool staged = nf <= a.r.cap;
    if (staged) {
#pragma unroll
        for (int k = 0; k < 3; ++k) stage_dma8<BS>(a.hat[k] + f0, sh + k * a.r.cap, nf, tid);
#pragma unroll
        for (int r = 0; r < NRHS; ++r) if (r < a.nst) stage_dma8<BS>(a.ssf[r] + f0, sh + (3 + r) * a.r.cap, nf, tid);
    }
    int nb = 0, ne = 0;
    if (live) { nb = a.r.ls[c]; ne = a.r.ls[c + 1]; }
    const int cnt = ne - nb;
    int nfk[4]; double nh[4][3], nv[4][NRHS];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                     // before the barrier: what LDS will not hold -- cut faces, and the fluxes past nst
        nfk[k] = (k < cnt) ? a.r.losort[nb + k] : 0;
        const int f = nfk[k];
        const bool cut = k < cnt && (!staged || f < f0);
#pragma unroll
        for (int d = 0; d < 3; ++d) nh[k][d] = cut ? a.hat[d][f] : 0.0;
#pragma unroll
        for (int r = 0; r < NRHS; ++r) nv[k][r] = (cut || (k < cnt && r >= a.nst)) ? a.ssf[r][f] : 0.0;
    }
    __syncthreads();
    if (!live) return;
    double s[3 * NRHS];
#pragma unroll
    for (int i = 0; i < 3 * NRHS; ++i) s[i] = 0.0;
    auto term = [&](const double (&h)[3], const double (&v)[NRHS]) {
#pragma unroll
        for (int r = 0; r < NRHS; ++r)
#pragma unroll
            for (int d = 0; d < 3; ++d) { const double p = h[d] * v[r]; s[3 * r + d] = s[3 * r + d] + p; }
    };
    auto face = [&](int f) {                          // an internal face: from LDS when the block owns it
        double h[3], v[NRHS];
        if (staged && f >= f0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) h[d] = sh[d * a.r.cap + (f - f0)];
#pragma unroll
            for (int r = 0; r < NRHS; ++r) v[r] = r < a.nst ? sh[(3 + r) * a.r.cap + (f - f0)] : a.ssf[r][f];
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) h[d] = a.hat[d][f];
#pragma unroll
            for (int r = 0; r < NRHS; ++r) v[r] = a.ssf[r][f];
        }
        term(h, v);
    };
    const int ob = a.r.os[c], oe = a.r.os[c + 1];
    for (int f = ob; f < oe; ++f) face(f);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < cnt) {
        if (staged && nfk[k] >= f0) {
            const int j = nfk[k] - f0;
#pragma unroll
            for (int d = 0; d < 3; ++d) nh[k][d] = sh[d * a.r.cap + j];
#pragma unroll
            for (int r = 0; r < NRHS; ++r) if (r < a.nst) nv[k][r] = sh[(3 + r) * a.r.cap + j];
        }
        term(nh[k], nv[k]);
    }
    for (int j = nb + 4; j < ne; ++j) face(a.r.losort[j]);
    if (a.r.bStart) for (int j = a.r.bStart[c]; j < a.r.bStart[c + 1]; ++j) {
        const int bf = a.r.bFace[j];
        double h[3], v[NRHS];
#pragma unroll
        for (int d = 0; d < 3; ++d) h[d] = a.bhat[d][bf];
#pragma unroll
        for (int r = 0; r < NRHS; ++r) v[r] = a.bssf[r][bf];
        term(h, v);
    }
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = a.inv[i][c];
#pragma unroll
    for (int r = 0; r < NRHS; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d)
            a.out[3 * r + d][c] = fma(R[3 * d + 2], s[3 * r + 2], fma(R[3 * d], s[3 * r], R[3 * d + 1] * s[3 * r + 1]));
}

} // namespace mi

// the reconstruction data of one mesh: inv(surfaceSum(SfHat*Sf)) per cell and SfHat per internal and boundary face, caller's order
struct mi_reconstruct_s : RowHandle {
    int32_t removed[3] = {0, 0, 0};
    DevBuf<double> hat[3], bhat[3], inv[9];
};

extern "C" int mi_surface_sum(mi_addr_t a, int32_t mode, const double* ssf_dev, double* out_dev)
{
    const std::string who = "mi_surface_sum";
    if (!a) return fail(MI_ERR_ARG, who + ": bad argument");
    if (mode != MI_SURFACE_SUM && mode != MI_SURFACE_SUM_MAG) return fail(MI_ERR_ARG, who + ": mode must be MI_SURFACE_SUM or MI_SURFACE_SUM_MAG");
    if (a->L.nCells == 0) return MI_OK;
    if (!out_dev || (!ssf_dev && !faceless(a))) return fail(MI_ERR_ARG, who + ": an array is missing");
    const void* p[2] = {ssf_dev, out_dev};
    MICHK(arrays_aligned8(who, p, 2));
    if (out_dev == ssf_dev) return fail(MI_ERR_ARG, who + ": the output must not alias the input");
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    // the row pass of mi_row_face_op (kind 0 / kind 2 with one face array) started from +0.0: own faces ascending, then losort order
    if (mode == MI_SURFACE_SUM) return row_sum<M_PLUS, M_PLUS>(a, ssf_dev, ssf_dev, nullptr, nullptr, out_dev);
    return row_sum<M_MAG, M_MAG>(a, ssf_dev, ssf_dev, nullptr, nullptr, out_dev);
}

extern "C" int mi_reconstruct_create(mi_addr_t a, mi_grad_boundary_t b, const double* const* sf_dev, const double* mag_sf_dev,
                                     const double* const* b_sf_dev, const double* b_mag_sf_dev, mi_reconstruct_t* out)
{
    const std::string who = "mi_reconstruct_create";
    std::unique_ptr<mi_reconstruct_s> v(new mi_reconstruct_s());
    MICHK(row_handle_open(who, a, b, out, *v));
    const int32_t n = v->nCells, nf = v->nFaces, nb = v->nBFaces;
    const void* in[8];
    int nIn = 0;
    if (nf > 0) {
        if (!sf_dev || !sf_dev[0] || !sf_dev[1] || !sf_dev[2] || !mag_sf_dev) return fail(MI_ERR_ARG, who + ": the face area vectors and magSf are missing");
        for (int k = 0; k < 3; ++k) in[nIn++] = sf_dev[k];
        in[nIn++] = mag_sf_dev;
    }
    if (nb > 0) {
        if (!b_sf_dev || !b_sf_dev[0] || !b_sf_dev[1] || !b_sf_dev[2] || !b_mag_sf_dev)
            return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary Sf and magSf needed");
        for (int k = 0; k < 3; ++k) in[nIn++] = b_sf_dev[k];
        in[nIn++] = b_mag_sf_dev;
    }
    MICHK(arrays_aligned8(who, in, nIn));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    hipStream_t s = a->ctx->stream;
    if (n == 0) { *out = v.release(); return MI_OK; }
    for (int k = 0; k < 3; ++k) {
        if (nf > 0) MICHK(v->hat[k].alloc((size_t)nf));
        if (nb > 0) MICHK(v->bhat[k].alloc((size_t)nb));
    }
    for (int i = 0; i < 9; ++i) MICHK(v->inv[i].alloc((size_t)n));
    DevBuf<double> t0;                                // caller cell 0's nine values
    MICHK(t0.alloc(9));
    RcBuildArgs q{};
    q.r = row_tables(a, b);
    if (nf > 0) { for (int k = 0; k < 3; ++k) { q.sf[k] = sf_dev[k]; q.hat[k] = v->hat[k].p; } q.magSf = mag_sf_dev; }
    if (nb > 0) {
        q.bMagSf = b_mag_sf_dev;
        for (int k = 0; k < 3; ++k) { q.bsf[k] = b_sf_dev[k]; q.bhat[k] = v->bhat[k].p; }
    }
    for (int i = 0; i < 9; ++i) q.T[i] = v->inv[i].p;
    q.T0 = t0.p;
    q.nf = nf; q.nb = nb;
    const int cellBlocks = (n + 255) / 256;
    const int64_t faces = (int64_t)nf + nb;
    if (faces > 0) { k_rc_hat<<<(unsigned)((faces + 255) / 256), 256, 0, s>>>(q); HIPCHK(hipGetLastError()); }
    k_rc_tensor<<<cellBlocks, 256, 0, s>>>(q);
    HIPCHK(hipGetLastError());
    // removeCmpts from caller cell 0 alone (tensorField.C:233-251; magSqr(Tensor): the nine squares left to right; SMALL = 1e-15).  A cell
    // 0 without faces gives 0/0: the comparisons are false and nothing is removed
    double t[9];
    HIPCHK(hipMemcpyAsync(t, q.T0, sizeof t, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double scale = t[0] * t[0];
    for (int i = 1; i < 9; ++i) scale = scale + t[i] * t[i];
    for (int d = 0; d < 3; ++d)
        if (t[4 * d] / scale < 1.0e-15) { q.removes = 1; q.add[4 * d] = 1.0; v->removed[d] = 1; }
    k_rc_invert<<<cellBlocks, 256, 0, s>>>(q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));                  // the caller's geometry arrays and t0 are free from here
    *out = v.release();
    return MI_OK;
}
extern "C" int mi_reconstruct_destroy(mi_reconstruct_t rc) { delete rc; return MI_OK; }

extern "C" int mi_reconstruct_fields(mi_reconstruct_t rc, double* const* inv_out_dev, int32_t* removed_out_host)
{
    const std::string who = "mi_reconstruct_fields";
    if (!rc) return fail(MI_ERR_ARG, who + ": bad argument");
    if (rc->nCells > 0) {
        if (!inv_out_dev) return fail(MI_ERR_ARG, who + ": output arrays missing");
        const double* in[9];
        for (int i = 0; i < 9; ++i) in[i] = rc->inv[i].p;
        MICHK(outputs_distinct(who, in, 9, inv_out_dev, 9));
        MICHK(arrays_aligned8(who, (const void* const*)inv_out_dev, 9));
        HIPCHK(hipSetDevice(rc->ctx->device));
        for (int i = 0; i < 9; ++i)
            HIPCHK(hipMemcpyAsync(inv_out_dev[i], rc->inv[i].p, (size_t)rc->nCells * sizeof(double), hipMemcpyDeviceToDevice, rc->ctx->stream));
    }
    if (removed_out_host) for (int d = 0; d < 3; ++d) removed_out_host[d] = rc->removed[d];
    return MI_OK;
}

extern "C" int mi_fvc_reconstruct(mi_reconstruct_t rc, int32_t n_rhs, const double* const* ssf_dev, const double* const* b_ssf_dev_or_null,
                                  double* const* out_dev)
{
    const std::string who = "mi_fvc_reconstruct";
    if (!rc) return fail(MI_ERR_ARG, who + ": bad argument");
    if (n_rhs < 1 || n_rhs > 4) return fail(MI_ERR_ARG, who + ": n_rhs must be 1 to 4");
    mi_addr_s* a = rc->addr;
    MICHK(row_handle_check(who, rc));
    if (rc->nCells == 0) return MI_OK;
    if (!out_dev) return fail(MI_ERR_ARG, who + ": output arrays missing");
    const bool hasF = rc->nFaces > 0, hasB = rc->nBFaces > 0;
    if (hasF && !ssf_dev) return fail(MI_ERR_ARG, who + ": input arrays missing");
    if (hasB && !b_ssf_dev_or_null) return fail(MI_ERR_ARG, who + ": the boundary has faces: boundary fluxes needed");
    const double* in[23];
    int nIn = 0;
    for (int r = 0; r < n_rhs; ++r) { if (hasF) in[nIn++] = ssf_dev[r]; if (hasB) in[nIn++] = b_ssf_dev_or_null[r]; }
    MICHK(arrays_present(who, in, nIn));
    MICHK(arrays_aligned8(who, (const void* const*)in, nIn));
    for (int k = 0; k < 3; ++k) { if (hasF) in[nIn++] = rc->hat[k].p; if (hasB) in[nIn++] = rc->bhat[k].p; }
    for (int i = 0; i < 9; ++i) in[nIn++] = rc->inv[i].p;
    MICHK(outputs_distinct(who, in, nIn, out_dev, 3 * n_rhs));
    MICHK(arrays_aligned8(who, (const void* const*)out_dev, 3 * n_rhs));
    HIPCHK(hipSetDevice(a->ctx->device));
    MICHK(ensure_caller_tables(a));
    RcArgs q{};
    const mi_addr_s::RowPlan& rp = a->rowPlan[1];     // the gradient's plan
    q.r = row_tables(a, rc->boundary);
    for (int k = 0; k < 3; ++k) { q.hat[k] = rc->hat[k].p; q.bhat[k] = rc->bhat[k].p; }
    for (int r = 0; r < n_rhs; ++r) { if (hasF) q.ssf[r] = ssf_dev[r]; if (hasB) q.bssf[r] = b_ssf_dev_or_null[r]; }
    for (int i = 0; i < 9; ++i) q.inv[i] = rc->inv[i].p;
    for (int i = 0; i < 3 * n_rhs; ++i) q.out[i] = out_dev[i];
    // 3 + n_rhs staged arrays within row_cap's budget; where the largest block does not fit with all the fluxes, as many as do fit are
    // staged (SfHat first: every flux reads it) rather than sending every block down the unstaged path
    int nst = n_rhs;
    if (rp.capForced <= 0) {
        const int want = (rp.maxFaces + 1) & ~1;
        while (nst > 0 && row_cap(rp, 3 + nst) < want) --nst;
        if (row_cap(rp, 3 + nst) < want) nst = n_rhs;  // not even SfHat alone: the blocks that fit stage everything, the others nothing
    }
    q.nst = nst;
    switch (n_rhs) {
    case 1: return row_launch_bs(a, 3 + nst, ROW_BS(k_reconstruct, 1), q);
    case 2: return row_launch_bs(a, 3 + nst, ROW_BS(k_reconstruct, 2), q);
    case 3: return row_launch_bs(a, 3 + nst, ROW_BS(k_reconstruct, 3), q);
    default: return row_launch_bs(a, 3 + nst, ROW_BS(k_reconstruct, 4), q);
    }
}
