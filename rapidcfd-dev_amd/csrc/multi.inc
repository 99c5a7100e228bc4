// multi.inc -- several right-hand sides against ONE matrix in one solve (included by engine.hip).
//
// fvMatrix<vector>::solveSegregated (src/finiteVolume/fvMatrices/fvMatrix/fvMatrixSolve.C:103-225) solves the components of a
// vector equation one after the other with the same lduMatrix: three solver constructions, three prologues and, per
// iteration, three passes over the same upper / lower / addressing for A p and three for A^T p (PBiCG.C:67-246).  The
// MI355X-first form keeps each component's arithmetic -- its own scalars, its own convergence test, the same fma chains and
// reduction trees as a single solve, so each history equals the single-component solve bit for bit -- and shares what does
// not depend on the component: tile_kernel_multi stages a tile's coefficients ONCE for the 2 x nrhs operand vectors of a
// step (A p_c and A^T pT_c, or the DILU pair precondition / preconditionT), sumA and 1/diag are computed once per binding,
// and the host polls all components with one copy.
namespace {

struct MultiDiag { const double* diag[3]; const double* rD[3]; };   // engine order, per component (all equal: shared)
// operands / results of component c: x[2c] (plain) and x[2c+1] (through the transpose), y / y2 likewise; dotPartial[c]: nTiles
// doubles receiving the per-tile partials of y[2c] . x[2c+1] (or nullptr); b[c], y2: the prologue's  y2 = b - y
struct MultiIO {
    const double* x[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double* y[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double* y2[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const double* b[3] = {nullptr, nullptr, nullptr};
    double* dotPartial[3] = {nullptr, nullptr, nullptr};
    double* sumA[3] = {nullptr, nullptr, nullptr};   // OP_PROLOGUE: sumA with component c's diagonal, out of the same pass (or nullptr)
    const int32_t* done[3] = {nullptr, nullptr, nullptr};
    bool storeTransposed = true;   // false: the fused pass does not store y[2c+1] (the prologue only needs y2 = b - y of it); the fall-back always does
};

template <int OP, int NRHS, bool SRD>
int launch_tile_multi_n(mi_matrix_s* m, const MultiIO& io, const MultiDiag& dg, const int* comp)
{
    mi_addr_s* a = m->addr;
    mi_ctx_s* cx = a->ctx;
    const TileLayout& L = a->L;
    TileArgs t;
    t.tileCellStart = a->tileCellStart.p; t.tileSlotStart = a->tileSlotStart.p; t.tileIfaceSlot0 = a->tileIfaceSlot0.p; t.tileHaloStart = a->tileHaloStart.p;
    t.haloCell = a->haloCell.p; t.tileSliceStart = a->tileSliceStart.p; t.sliceEntryStart = a->sliceEntryStart.p;
    t.entries = a->entries.p; t.entries16 = nullptr; t.sliceEntryStart16 = nullptr; t.slotBase = nullptr; t.tileSbStart = nullptr;
    t.diag = nullptr; t.up = m->upE.p; t.low = m->asym ? m->lowE.p : m->upE.p;
    t.x = nullptr; t.b = nullptr; t.rD = nullptr; t.y = nullptr; t.omega = 0.0; t.dotPartial = nullptr; t.dotPartial2 = nullptr; t.flags = cx->tileFlags;
    t.tileList = nullptr; t.nPos = L.nTiles; t.done = nullptr;
    const int32_t slots = (L.maxSlots + 3) & ~1;
    const int32_t xlen = (((L.maxCells + 63) & ~63) + L.maxHalo + 2 + 1) & ~1;
    const int nOperands = OP == OP_SUMA ? 0 : 2 * NRHS, nRD = OP == OP_AINV ? (SRD ? 1 : NRHS) : 0;
    t.offLow = slots; t.offX = 2 * slots; t.offRD = 2 * slots + nOperands * xlen; t.offSB = xlen;
    const size_t lds = sizeof(double) * ((size_t)t.offRD + (size_t)nRD * (size_t)xlen);
    if (sw::get(SW_DEBUG_MULTI)) fprintf(stderr, "[multi] OP %d NRHS %d SRD %d: slots %d xlen %d (maxCells %d maxHalo %d) lds %zu\n", OP, NRHS, (int)SRD, slots, xlen, L.maxCells, L.maxHalo, lds);
    if (lds > 159 * 1024) return MI_ERR_LIMIT;     // (no message: the caller falls back to fewer operands per pass)
    MultiVec<NRHS> V;
    for (int k = 0; k < NRHS; ++k) {
        const int c = comp[k];
        V.x[k] = io.x[2 * c]; V.x[NRHS + k] = io.x[2 * c + 1];
        V.y[k] = io.y[2 * c]; V.y[NRHS + k] = io.storeTransposed ? io.y[2 * c + 1] : nullptr;
        V.y2[k] = io.y2[2 * c]; V.y2[NRHS + k] = io.y2[2 * c + 1];
        V.b[k] = io.b[c]; V.dotPartial[k] = io.dotPartial[c];
        V.done[k] = io.done[c]; V.diag[k] = dg.diag[c]; V.rD[k] = dg.rD[c]; V.sumA[k] = io.sumA[c];
    }
    if constexpr ((OP == OP_AMUL || OP == OP_AINV) && SRD) {
        // the passes of the Krylov iterations (no fused b - y): one resident workgroup per CU that prefetches its next tile into
        // registers while it walks the current one (multi_pipe.inc); same bits, same per-tile partials
        bool anyY2 = false;
        for (int v = 0; v < 2 * NRHS; ++v) anyY2 = anyY2 || V.y2[v] != nullptr;
        if (cx->multiPipe && !anyY2 && L.maxCells <= 1024 && slots <= 4096 && L.nTiles > 0) {
            const int G = std::min(L.nTiles, std::max(8, (cx->nCU / 8) * 8));
            const void* pf = (const void*)tile_kernel_multi_pipe<OP, NRHS>;
            if (!cx->ldsAttrSet.count(pf)) { HIPCHK(hipFuncSetAttribute(pf, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024)); cx->ldsAttrSet.insert(pf); }
            tile_kernel_multi_pipe<OP, NRHS><<<G, 1024, lds, cx->stream>>>(t, V, L.nTiles);
            HIPCHK(hipGetLastError());
            return MI_OK;
        }
    }
    const void* fn = (const void*)tile_kernel_multi<OP, NRHS, SRD, 1024>;
    if (!cx->ldsAttrSet.count(fn)) { HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024)); cx->ldsAttrSet.insert(fn); }
    if (L.nTiles > 0) tile_kernel_multi<OP, NRHS, SRD, 1024><<<L.nTiles, 1024, lds, cx->stream>>>(t, V);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
template <int OP>
int launch_tile_multi_group(mi_matrix_s* m, int n, const int* comp, const MultiIO& io, const MultiDiag& dg)
{
    bool shared = true;
    for (int k = 1; k < n; ++k) if (dg.rD[comp[k]] != dg.rD[comp[0]]) shared = false;
    if (OP != OP_AINV) shared = true;   // (only the AINV pass stages rD)
    if (n == 3) return shared ? launch_tile_multi_n<OP, 3, true>(m, io, dg, comp) : launch_tile_multi_n<OP, 3, false>(m, io, dg, comp);
    if (n == 2) return shared ? launch_tile_multi_n<OP, 2, true>(m, io, dg, comp) : launch_tile_multi_n<OP, 2, false>(m, io, dg, comp);
    return launch_tile_multi_n<OP, 1, true>(m, io, dg, comp);
}

// As few passes over the coefficients as the LDS allows: all components at once, else two and one, else one by one, else the
// single-vector kernels (*fused = false then: no dot partials, no y2 -- the caller runs its separate passes).
template <int OP>
int tile_multi(mi_matrix_s* m, int nrhs, const MultiIO& io, const MultiDiag& dg, bool* fused)
{
    mi_addr_s* a = m->addr;
    if (!m->bound) return fail(MI_ERR_STATE, "matrix coefficients not bound (mi_matrix_set_coeffs)");
    if ((OP == OP_AMUL || OP == OP_PROLOGUE) && !a->ami.empty()) for (int v = 0; v < 2 * nrhs; ++v) MICHK(ami_fill(m, io.x[v]));
    *fused = true;
    if (!a->compact && sw::get(SW_MULTI_TILE)) {
        static const int all[3] = {0, 1, 2};
        int rc = launch_tile_multi_group<OP>(m, nrhs, all, io, dg);
        if (rc == MI_ERR_LIMIT && nrhs == 3) {       // two components and one
            static const int one[1] = {2};
            rc = launch_tile_multi_group<OP>(m, 2, all, io, dg);
            if (rc == MI_OK) rc = launch_tile_multi_group<OP>(m, 1, one, io, dg);
        }
        if (rc == MI_ERR_LIMIT && nrhs > 1) {
            rc = MI_OK;
            for (int c = 0; c < nrhs && rc == MI_OK; ++c) { const int one[1] = {c}; rc = launch_tile_multi_group<OP>(m, 1, one, io, dg); }
        }
        if (rc != MI_ERR_LIMIT) return rc;
    }
    *fused = false;
    if (sw::get(SW_DEBUG_MULTI)) fprintf(stderr, "[multi] OP %d: single-vector fall-back (compact %d)\n", OP, (int)a->compact);
    if (OP == OP_PROLOGUE) return MI_OK;   // (the caller runs the separate prologue passes)
    if (OP == OP_SUMA || dg.diag[0] != m->diagE.p) return fail(MI_ERR_LIMIT, "multi-vector tile pass: the tile image does not fit the LDS (per-component diagonals have no single-vector path)");
    for (int c = 0; c < nrhs; ++c) {   // (a finished component's single-vector passes are not gated: they only cost time)
        MICHK(launch_tile<OP>(m, false, io.x[2 * c], nullptr, m->rD.p, io.y[2 * c], 0.0, 0));
        MICHK(launch_tile<OP>(m, true, io.x[2 * c + 1], nullptr, m->rD.p, io.y[2 * c + 1], 0.0, 0));
    }
    return MI_OK;
}

// ONE halo exchange for the operand vectors of a multi-vector pass (engine order, ext region behind the owned cells) on a
// matrix with communicators attached -- round 4: the reference exchanges per operand and per component
// (lduMatrixUpdateMatrixInterfaces.C:30-276 inside every Amul / Tmul of every solveSegregated component), round 3 therefore
// solved the components of a decomposed momentum equation one after the other.  Over peer windows: one k_halo_push with all
// operands (a window holds HALO_NV of them per parity) and one k_halo_pull; over the communicator's own send / recv: one
// grouped call per operand.
int multi_exchange(mi_matrix_s* m, int nv, double* const* xs)
{
    if (!comm_remote(m)) return MI_OK;
    double* u[HALO_NV]; const double* cu[HALO_NV];
    int nu = 0;
    for (int v = 0; v < nv; ++v) {
        bool seen = false;
        for (int k = 0; k < nu; ++k) if (u[k] == xs[v]) seen = true;
        if (seen) continue;
        if (nu == HALO_NV) return fail(MI_ERR_LIMIT, "multi-vector halo exchange: too many operands");
        u[nu] = xs[v]; cu[nu] = xs[v]; ++nu;
    }
    if (peer_halo_ready(m)) {
        MICHK(peer_exchange_push_n(m, nu, cu));
        return peer_exchange_pull_n(m, nu, u);
    }
    mi_addr_s* a = m->addr;
    if (m->sendBuf.n < (size_t)a->L.nExt) MICHK(m->sendBuf.alloc((size_t)a->L.nExt));
    for (int v = 0; v < nu; ++v) {
        MICHK(mi_halo_pack_engine(a, u[v], m->sendBuf.p));
        MICHK(comm_exchange_start(m, m->sendBuf.p, u[v]));
        MICHK(comm_exchange_wait(m));       // (also: the send buffer is free again before the next operand is packed)
        MICHK(scale_received(m, u[v]));
    }
    return MI_OK;
}

// the sums of up to three components that are due at the same point of their loops become GLOBAL sums in one all-reduce
// (what globalize does for one solve): final reductions (block k: P[k]), all-reduce of n doubles, spread back as {sum, 0, ...}
struct Ptr6 { double* p[6]; };
__global__ __launch_bounds__(RB) void k_reduce_final_n(const Ptr6 P, double* __restrict__ out)
{
    __shared__ double red[RB / 64];
    const double t = sum_partials(P.p[blockIdx.x], red);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}
__global__ __launch_bounds__(RB) void k_spread_n(const double* __restrict__ sums, const Ptr6 P)
{
    double* q = P.p[blockIdx.x];
    const double v = sums[blockIdx.x];
    for (int i = threadIdx.x; i < RG; i += RB) q[i] = (i == 0) ? v : 0.0;
}
int globalize_n(mi_matrix_s* m, int n, double* const* P)
{
    if (!comm_attached(m) || n <= 0) return MI_OK;
    mi_ctx_s* c = m->addr->ctx;
    hipStream_t s = c->stream;
    if (n > 6) return fail(MI_ERR_LIMIT, "globalize_n: at most six sums");
    if (peer_reduce_ready(m)) return peer_globalize(m, n, P);
    Ptr6 q;
    for (int k = 0; k < 6; ++k) q.p[k] = P[k < n ? k : 0];
    double* sc = c->scalars.p + 10;
    k_reduce_final_n<<<n, RB, 0, s>>>(q, sc);
    MICHK(comm_allreduce(m, sc, (size_t)n));
    k_spread_n<<<n, RB, 0, s>>>(sc, q);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

int tile_pair(mi_matrix_s* m, bool ainv, const double* x0, const double* x1, double* y0, double* y1, const int32_t* gate, double* dotPartial, bool* fused)
{
    MultiIO io;
    io.x[0] = x0; io.x[1] = x1; io.y[0] = y0; io.y[1] = y1; io.done[0] = gate; io.dotPartial[0] = dotPartial;
    MultiDiag dg; for (int k = 0; k < 3; ++k) { dg.diag[k] = m->diagE.p; dg.rD[k] = m->rD.p; }
    return ainv ? tile_multi<OP_AINV>(m, 1, io, dg, fused) : tile_multi<OP_AMUL>(m, 1, io, dg, fused);
}

} // namespace

namespace {
// mi_pbicg_solve takes the multi-vector solver's route for its one right-hand side exactly when mi_pbicg_solve_multi would not hand it back
bool pbicg_single_via_multi(const mi_matrix_s* m)
{
    if (sw::get(SW_PBICG_MULTI) == 0 || m->addr->compact || !m->addr->ami.empty()) return false;
    return !(comm_attached(m) && (comm_any_ami(m) || comm_any_compact(m)));
}
}
extern "C" int mi_pbicg_solve_multi(mi_matrix_t m, int32_t nrhs, const double* const* diag_dev, double* const* psi_io, const double* const* source,
                                    const mi_solver_controls* ctl, int precond, mi_solver_perf* perf, double* hist_host, int32_t hist_len)
{
    if (!m || nrhs < 1 || nrhs > 3 || !psi_io || !source || !ctl) return fail(MI_ERR_ARG, "mi_pbicg_solve_multi: bad argument (1 <= nrhs <= 3)");
    for (int c = 0; c < nrhs; ++c) if (!psi_io[c] || !source[c] || (diag_dev && !diag_dev[c])) return fail(MI_ERR_ARG, "mi_pbicg_solve_multi: NULL component");
    MICHK(solver_entry("mi_pbicg_solve_multi", m, true));
    if (precond != MI_PRECOND_NONE && precond != MI_PRECOND_DIAGONAL && precond != MI_PRECOND_AINV) return fail(MI_ERR_ARG, "unknown preconditioner kind");
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    const bool att = comm_attached(m);
    if ((att && (comm_any_ami(m) || comm_any_compact(m))) || sw::get(SW_PBICG_MULTI) == 0) {
        // component by component, as the reference (a decomposed matrix with cyclicAMI patches interpolates per operand inside
        // its tile operators; MI_PBICG_MULTI=0: A/B hook)
        if (diag_dev) return fail(MI_ERR_UNSUPPORTED, "mi_pbicg_solve_multi: per-component diagonals with MI_PBICG_MULTI=0 (or on an attached matrix with cyclicAMI patches): bind each diagonal and call mi_pbicg_solve");
        for (int k = 0; k < nrhs; ++k) {
            if (c->pbicgHostStepped == 0) MICHK(pbicg_solve_device(m, psi_io[k], source[k], ctl, precond, perf ? perf + k : nullptr, hist_host ? hist_host + (size_t)k * (size_t)hist_len : nullptr, hist_len));
            else MICHK(mi_pbicg_solve(m, psi_io[k], source[k], ctl, precond, perf ? perf + k : nullptr, hist_host ? hist_host + (size_t)k * (size_t)hist_len : nullptr, hist_len));
        }
        return MI_OK;
    }
    hipStream_t s = c->stream;
    const int64_t n = a->L.nCells;
    const int histLen = ctl->maxIter + 2;
    c->stats[6] += 1;   // mi_ctx_stat(6): solves through the multi-vector loop below
    // per component: 8 engine-order vectors (+ diagonal, 1/diagonal, sumA when the diagonals differ), a device state, 4 RG partial slots, a history
    double *psi[3], *src[3], *pA[3], *wA[3], *rA[3], *pT[3], *wT[3], *rT[3], *dgE[3] = {nullptr, nullptr, nullptr}, *rDc[3] = {nullptr, nullptr, nullptr}, *sumAc[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < nrhs; ++k) {
        double** vs[8] = {&psi[k], &src[k], &pA[k], &wA[k], &rA[k], &pT[k], &wT[k], &rT[k]};
        const size_t v0 = WV_MULTI + WV_MULTI_STRIDE * (size_t)k;
        for (size_t j = 0; j < 8; ++j) MICHK(m->vec(v0 + j, vs[j]));
        if (diag_dev) MICHK(m->vecs({{v0 + 8, &dgE[k]}, {v0 + 9, &rDc[k]}, {v0 + 10, &sumAc[k]}}));
    }
    if (m->mstate.n < 3) MICHK(m->mstate.alloc(3));
    if (m->mpartial.n < (size_t)3 * 4 * RG) MICHK(m->mpartial.alloc((size_t)3 * 4 * RG));
    if (m->mhist.n < (size_t)3 * (size_t)histLen) MICHK(m->mhist.alloc((size_t)3 * (size_t)histLen));
    if (!m->mhostState) HIPCHK(hipHostMalloc((void**)&m->mhostState, 3 * sizeof(PcgState)));
    MICHK(ensure_rD(m));
    MultiDiag dg;
    for (int k = 0; k < 3; ++k) { dg.diag[k] = m->diagE.p; dg.rD[k] = m->rD.p; }
    PcgState* st[3]; double *P1[3], *P2[3], *P3[3], *hist[3]; const int32_t* done[3];
    for (int k = 0; k < nrhs; ++k) {
        st[k] = m->mstate.p + k; P1[k] = m->mpartial.p + (size_t)k * 4 * RG; P2[k] = P1[k] + RG; P3[k] = P1[k] + 2 * RG;
        hist[k] = m->mhist.p + (size_t)k * (size_t)histLen; done[k] = &st[k]->done;
        PcgState h; memset(&h, 0, sizeof(h));
        h.tolerance = ctl->tolerance; h.relTol = ctl->relTol; h.maxIter = ctl->maxIter; h.minIter = ctl->minIter;
        m->mhostState[k] = h;
        k_gather_perm<<<RG, RB, 0, s>>>(psi_io[k], a->perm(), psi[k], a->L.nCells);
        k_gather_perm<<<RG, RB, 0, s>>>(source[k], a->perm(), src[k], a->L.nCells);
        if (diag_dev) { // component k's diagonal (addBoundaryDiag(diag, cmpt)) and its reciprocal, engine order
            k_gather_perm<<<RG, RB, 0, s>>>(diag_dev[k], a->perm(), dgE[k], a->L.nCells);
            k_recip<<<RG, RB, 0, s>>>(rDc[k], dgE[k], n);
            dg.diag[k] = dgE[k]; dg.rD[k] = rDc[k];
        }
    }
    HIPCHK(hipMemcpyAsync(m->mstate.p, m->mhostState, sizeof(PcgState) * (size_t)nrhs, hipMemcpyHostToDevice, s));
    // ---- prologue (PBiCG.C:91-131 for every component) in ONE pass over the coefficients: wA = A psi (normFactor needs it),
    //      rA = source - wA, rT = source - A^T psi
    if (m->mtilePartial.n < (size_t)3 * (size_t)a->L.nTiles) MICHK(m->mtilePartial.alloc((size_t)3 * (size_t)a->L.nTiles));   // (its own buffer: GAMG relies on the zero tail of tilePartial)
    bool fused = false;
    const double* sumA[3];
    bool sumADone = false;
    {
        MultiIO io;
        for (int k = 0; k < nrhs; ++k) { io.x[2 * k] = psi[k]; io.x[2 * k + 1] = psi[k]; io.y[2 * k] = wA[k]; io.y[2 * k + 1] = wT[k]; io.storeTransposed = false; io.y2[2 * k] = rA[k]; io.y2[2 * k + 1] = rT[k]; io.b[k] = src[k]; }
        if (att) MICHK(multi_exchange(m, nrhs, psi));   // neighbour-rank values of every component's psi in one exchange
        if (c->fusePrologue && (diag_dev || !m->sumAValid)) {
            // ... and sumA (lduMatrix::sumA starts from the diagonal: per component when the diagonals differ) out of the SAME pass
            if (!diag_dev && m->sumAE.n != (size_t)n) MICHK(m->sumAE.alloc((size_t)n));
            for (int k = 0; k < nrhs; ++k) { io.sumA[k] = diag_dev ? sumAc[k] : (k == 0 ? m->sumAE.p : nullptr); sumA[k] = diag_dev ? sumAc[k] : m->sumAE.p; }
            MICHK((tile_multi<OP_PROLOGUE>(m, nrhs, io, dg, &fused)));
            if (fused) { sumADone = true; if (!diag_dev) m->sumAValid = true; }
            else { for (int k = 0; k < nrhs; ++k) io.sumA[k] = nullptr; }
        }
        if (!fused) MICHK((tile_multi<OP_AMUL>(m, nrhs, io, dg, &fused)));
        if (!fused) for (int k = 0; k < nrhs; ++k) { k_sub<<<RG, RB, 0, s>>>(rA[k], src[k], wA[k], n); k_sub<<<RG, RB, 0, s>>>(rT[k], src[k], wT[k], n); }
    }
    if (sumADone) { // (out of the prologue pass)
    } else if (diag_dev) { // lduMatrix::sumA starts from the diagonal: one pass gives every component's
        MultiIO io; bool f = false;
        for (int k = 0; k < nrhs; ++k) { io.y[2 * k] = sumAc[k]; sumA[k] = sumAc[k]; }
        MICHK((tile_multi<OP_SUMA>(m, nrhs, io, dg, &f)));
    } else {
        if (!m->sumAValid) { // sumA depends on the coefficients only: once per binding, shared by the components
            if (m->sumAE.n != (size_t)n) MICHK(m->sumAE.alloc((size_t)n));
            MICHK(launch_tile<OP_SUMA>(m, false, nullptr, nullptr, nullptr, m->sumAE.p, 0.0, 0));
            m->sumAValid = true;
        }
        for (int k = 0; k < nrhs; ++k) sumA[k] = m->sumAE.p;
    }
    if (c->fusePrologue) {
        // the components' sums in ONE launch each: sum psi; normFactor + sum|rA| (rA formed again from source - wA: the same rounding), with
        // gAverage(psi) on the device; the first convergence tests.  Partials per component: P1 normFactor, P2 sum|rA|, P3 sum psi
        Sum3 S3; NormMag3 N3; Init3 I3;
        for (int k = 0; k < 3; ++k) {
            const int j = k < nrhs ? k : 0;
            S3.a[k] = psi[j]; S3.partial[k] = P3[j];
            N3.Apsi[k] = wA[j]; N3.src[k] = src[j]; N3.sumA[k] = sumA[j]; N3.sumPsi[k] = P3[j]; N3.partialNF[k] = P1[j]; N3.partialMag[k] = P2[j];
            I3.st[k] = st[j]; I3.partialNF[k] = P1[j]; I3.partialR[k] = P2[j]; I3.hist[k] = hist[j];
        }
        k_sum3<<<dim3(RG, nrhs), RB, 0, s>>>(S3, n);
        if (!att) {
            k_normfactor_mag3<false><<<dim3(RG, nrhs), RB, 0, s>>>(N3, (double)n, n);
            k_solve_init3<false><<<nrhs, RB, 0, s>>>(I3, histLen);
        } else {
            // decomposed case: gSum(psi), the normFactor sum and gSumMag(rA) are global (lduMatrixSolver.C:182-236): the components'
            // sums travel together -- one all-reduce of nrhs doubles, one of 2 nrhs
            Ptr6 q; for (int k = 0; k < 6; ++k) q.p[k] = P3[k < nrhs ? k : 0];
            k_reduce_final_n<<<nrhs, RB, 0, s>>>(q, c->scalars.p);
            MICHK(comm_allreduce(m, c->scalars.p, (size_t)nrhs));
            for (int k = 0; k < 3; ++k) N3.sumPsi[k] = c->scalars.p + (k < nrhs ? k : 0);
            k_normfactor_mag3<true><<<dim3(RG, nrhs), RB, 0, s>>>(N3, (double)comm_n_global(m), n);
            for (int k = 0; k < nrhs; ++k) k_reduce_final2<<<2, RB, 0, s>>>(P1[k], c->scalars.p + 4 + 2 * k, P2[k], c->scalars.p + 5 + 2 * k);
            MICHK(comm_allreduce(m, c->scalars.p + 4, (size_t)2 * (size_t)nrhs));
            for (int k = 0; k < 3; ++k) { const int j = k < nrhs ? k : 0; I3.partialNF[k] = c->scalars.p + 4 + 2 * j; I3.partialR[k] = c->scalars.p + 5 + 2 * j; }
            k_solve_init3<true><<<nrhs, RB, 0, s>>>(I3, histLen);
        }
    } else
    if (!att) {
    for (int k = 0; k < nrhs; ++k) {
        // gAverage(psi) stays on the device (sum / n in the normFactor pass: the host's division, without the host)
        k_reduce<RED_SUM><<<RG, RB, 0, s>>>(psi[k], nullptr, n, P1[k]);
        k_reduce_final<<<1, RB, 0, s>>>(P1[k], c->scalars.p + k);
        k_normfactor_dev<<<RG, RB, 0, s>>>(wA[k], src[k], sumA[k], c->scalars.p + k, (double)n, n, P1[k]);
        k_reduce<RED_MAG><<<RG, RB, 0, s>>>(rA[k], nullptr, n, P2[k]);
        k_solve_init<false><<<1, RB, 0, s>>>(st[k], P1[k], P2[k], hist[k], histLen);
    }
    } else {
        // decomposed case: gSum(psi), the normFactor sum and gSumMag(rA) are global (lduMatrixSolver.C:182-236): the components'
        // sums travel together -- one all-reduce of nrhs doubles, one of 2 nrhs
        for (int k = 0; k < nrhs; ++k) { k_reduce<RED_SUM><<<RG, RB, 0, s>>>(psi[k], nullptr, n, P1[k]); k_reduce_final<<<1, RB, 0, s>>>(P1[k], c->scalars.p + k); }
        MICHK(comm_allreduce(m, c->scalars.p, (size_t)nrhs));
        for (int k = 0; k < nrhs; ++k) {
            k_normfactor_dev<<<RG, RB, 0, s>>>(wA[k], src[k], sumA[k], c->scalars.p + k, (double)comm_n_global(m), n, P1[k]);
            k_reduce<RED_MAG><<<RG, RB, 0, s>>>(rA[k], nullptr, n, P2[k]);
            k_reduce_final2<<<2, RB, 0, s>>>(P1[k], c->scalars.p + 4 + 2 * k, P2[k], c->scalars.p + 5 + 2 * k);
        }
        MICHK(comm_allreduce(m, c->scalars.p + 4, (size_t)2 * (size_t)nrhs));
        for (int k = 0; k < nrhs; ++k) k_solve_init<true><<<1, RB, 0, s>>>(st[k], c->scalars.p + 4 + 2 * k, c->scalars.p + 5 + 2 * k, hist[k], histLen);
    }
    HIPCHK(hipGetLastError());
    auto fetch = [&]() -> int {
        HIPCHK(hipMemcpyAsync(m->mhostState, m->mstate.p, sizeof(PcgState) * (size_t)nrhs, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MI_OK;
    };
    auto all_done = [&]() { for (int k = 0; k < nrhs; ++k) if (!m->mhostState[k].done) return false; return true; };
    // (no host read before the first iteration is enqueued: a component that the prologue finds converged gates itself)
    // ---- iterations: every component runs ITS loop (its scalars, its test); what they share is the pass over the matrix
    int it = 0;
    Fold3 f1, f2;
    for (int k = 0; k < 3; ++k) { f1.in[k] = m->mtilePartial.p + (size_t)(k < nrhs ? k : 0) * (size_t)a->L.nTiles; f1.out[k] = P1[k < nrhs ? k : 0]; f2.in[k] = f1.in[k]; f2.out[k] = P2[k < nrhs ? k : 0]; }
    auto enqueue = [&](int nb) -> int {
        for (int j = 0; j < nb; ++j, ++it) {
            if (precond == MI_PRECOND_AINV) { // DILU: precondition(wA, rA), preconditionT(wT, rT) and sum wA.rT of all components in one pass
                MultiIO io;
                for (int k = 0; k < nrhs; ++k) { io.x[2 * k] = rA[k]; io.x[2 * k + 1] = rT[k]; io.y[2 * k] = wA[k]; io.y[2 * k + 1] = wT[k]; io.done[k] = done[k]; io.dotPartial[k] = const_cast<double*>(f1.in[k]); }
                MICHK((tile_multi<OP_AINV>(m, nrhs, io, dg, &fused)));
                if (fused) k_fold_partials3<<<nrhs, 1024, 0, s>>>(f1, a->L.nTiles);
                else for (int k = 0; k < nrhs; ++k) k_reduce<RED_PROD><<<RG, RB, 0, s>>>(wA[k], rT[k], n, P1[k]);
            } else {
                for (int k = 0; k < nrhs; ++k) {
                    if (precond == MI_PRECOND_DIAGONAL) k_bicg_precond_dot<true><<<RG, RB, 0, s>>>(st[k], dg.rD[k], rA[k], rT[k], wA[k], wT[k], n, P1[k]);
                    else k_bicg_precond_dot<false><<<RG, RB, 0, s>>>(st[k], nullptr, rA[k], rT[k], wA[k], wT[k], n, P1[k]);
                }
            }
            MICHK(globalize_n(m, nrhs, P1));           // decomposed case: wA.rT of every component, one all-reduce
            for (int k = 0; k < nrhs; ++k) k_bicg_update_p<<<RG, RB, 0, s>>>(st[k], it, P1[k], wA[k], wT[k], pA[k], pT[k], n);
            {
                MultiIO io;
                for (int k = 0; k < nrhs; ++k) { io.x[2 * k] = pA[k]; io.x[2 * k + 1] = pT[k]; io.y[2 * k] = wA[k]; io.y[2 * k + 1] = wT[k]; io.done[k] = done[k]; io.dotPartial[k] = const_cast<double*>(f2.in[k]); }
                if (att) { double* ops[6]; for (int k = 0; k < nrhs; ++k) { ops[2 * k] = pA[k]; ops[2 * k + 1] = pT[k]; } MICHK(multi_exchange(m, 2 * nrhs, ops)); }   // pA and pT of every component: ONE exchange
                MICHK((tile_multi<OP_AMUL>(m, nrhs, io, dg, &fused)));
                if (fused) k_fold_partials3<<<nrhs, 1024, 0, s>>>(f2, a->L.nTiles);
                else for (int k = 0; k < nrhs; ++k) k_reduce<RED_PROD><<<RG, RB, 0, s>>>(wA[k], pT[k], n, P2[k]);
            }
            MICHK(globalize_n(m, nrhs, P2));           // wA.pT
            for (int k = 0; k < nrhs; ++k) k_bicg_update_psi_r<<<RG, RB, 0, s>>>(st[k], it, P2[k], pA[k], wA[k], wT[k], psi[k], rA[k], rT[k], n, P3[k]);
            MICHK(globalize_n(m, nrhs, P3));           // sum|rA|
            for (int k = 0; k < nrhs; ++k) k_pcg_final<false><<<1, RB, 0, s>>>(st[k], it, P3[k], hist[k], histLen);
        }
        HIPCHK(hipGetLastError());
        return MI_OK;
    };
    // (batches grow 1, 2, 4 ...: the momentum predictor of a time step usually needs ONE iteration per component.  After every fetch
    //  drive_batches checks the peer windows: a window wait that ran out of polls voids the sums)
    MICHK(drive_batches(m, ctl, it, 1, enqueue, fetch, all_done));
    for (int k = 0; k < nrhs; ++k) {
        k_scatter_perm<<<RG, RB, 0, s>>>(psi[k], a->perm(), psi_io[k], a->L.nCells);
        if (perf) fill_perf(m->mhostState[k], perf + k);
        if (hist_host) MICHK(copy_hist(s, hist[k], histLen, hist_host + (size_t)k * (size_t)hist_len, hist_len, m->mhostState[k].nIterations, false));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MI_OK;
}
