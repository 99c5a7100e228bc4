// PCG on one GPU: the residual update of iteration `it` and the search-direction update of iteration `it + 1` in ONE launch (round 6).
// PCG.C:166-195 then :139-160 of the next pass through the loop:
//
//     phase 1   alpha = wArA / wApA ; rA -= alpha wA ; sum|rA| ; wArA' = sum (rD o rA).rA          (k_pcg_update_psi_r)
//     -------   one grid barrier: the two sums are global
//     phase 2   convergence test ; psi += alpha pA ; beta = wArA' / wArA ; pA = rD o rA + beta pA    (k_pcg_final, k_pcg_update_p)
//
// The three kernels it replaces read rD and rA twice (k_pcg_update_p forms the preconditioned residual rD o rA again: 16 of its 48
// bytes per cell) because a launch boundary sits where the barrier sits here.  Workgroup b owns the same chunk of cells in both
// phases, so what phase 2 needs of phase 1 -- z = rD o rA, one double per cell -- STAYS ON THE CHIP: the first FUSED_HR strides of a
// chunk in registers, the next FUSED_LP pairs in LDS (10 M cells: 80 MB, of 128 MB of vector registers + 40 MB of LDS on the device;
// what does not fit is formed again from rD and rA as before).  Per iteration at 10 M cells: 64 instead of 80 bytes per cell in these
// passes, and the launch of k_pcg_final gone.  (Folding the Amul's per-tile partials here as well, instead of k_fold_partials' launch, was
// measured: no gain -- every workgroup pays the fold's load latency that the one-workgroup kernel pays once.)
//
// Same grid as the kernels it replaces (RG x RB, chunk b = partial slot b), same per-thread order of additions, same roundings:
// every partial sum, every vector and the residual history are bit for bit those of the separate kernels
// (tests/test_pcg_fused.py; MI_PCG_FUSE_RP=0 gives the separate kernels).
//
// The barrier is persist.inc's scheme for RG workgroups of RB threads: arrival slots on separate 64-byte lines, polled by workgroup
// 0, 64 release copies polled by the others; agent-scope (write-through) stores and agent-scope loads for everything that crosses
// workgroups, so nothing is flushed or invalidated.
//
// A PLAIN launch, and no workgroup ever depends on another one being resident.  hipLaunchCooperativeKernel costs ~22 us per launch on
// this runtime (measured: 3 400 it/s with it against 3 675 without, 3 415 for the separate kernels) -- more than the fusion saves.  On
// a device the process has to itself the RG workgroups ARE co-resident (four per CU: <= 64 VGPRs, <= 40 KB of LDS; the occupancy is
// asked once per context), but nothing guarantees it (another process's kernels, a partitioned device).  So a wait is bounded
// (FUSED_WAIT_POLLS, ~10 x the normal wait) and a workgroup that runs out of patience LEAVES: it marks its chunk pending and exits,
// which frees its CU for workgroups that have not started; workgroup 0, which collects the arrivals, hands its closing duties over the
// same way.  k_pcg_fused_finish, launched behind every fused launch, normally finds nothing and returns; otherwise it runs phase 2 of the
// pending chunks with z formed again from rD and rA (the same values: the same bits) and the closing duties.  No cooperative launch, no
// deadlock, no fault path.
namespace mi {

constexpr int FUSED_HR = 5;                      // strides of a chunk whose z values stay in registers (pairs: 4 VGPRs each)
constexpr int FUSED_PF = 3;                      // strides (<= FUSED_HR) whose psi update runs between arriving at the barrier and being released
constexpr int FUSED_LP = 2544;                   // pairs of z in LDS per workgroup (40 704 B + the reduction scratch: four workgroups per CU)
constexpr int FUSED_BAR_WORDS = BAR_LINE * (RG + 64) + RG + 64;   // + pending flag of every chunk, + workgroup 0's
constexpr int FUSED_PEND_AT = BAR_LINE * (RG + 64);
constexpr long long FUSED_WAIT_POLLS = 1000;     // a poll is a memory round trip (~1 us): the normal wait is a few tens
static_assert(sw::table[SW_PCG_FUSE_POLLS].dflt == FUSED_WAIT_POLLS, "switches.hpp: the default of MI_PCG_FUSE_POLLS is FUSED_WAIT_POLLS");

struct FusedArgs {
    PcgState* st;
    int it;
    const double* partial2;      // RG partials of wA.pA (k_fold_partials)
    double *partial3, *partial1; // out: RG partials of sum|rA|, of (rD o rA).rA
    const double *wA, *rD;
    double *pA, *psi, *rA;
    int64_t n;
    double* hist; int histLen;
    unsigned int* bar; unsigned int gen;   // barrier words; generation of THIS launch (the host counts the launches)
    long long maxPolls;
    int testMode;                          // tests: 1 = every third workgroup loses patience at once, 2 = workgroup 0 does, 3 = both
};

__device__ __forceinline__ void st_agent(double* p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double* p)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// sum_partials over slots other workgroups of THIS launch wrote (same order of additions)
__device__ __forceinline__ double sum_partials_agent(const double* partial, double* red)
{
    double v = 0;
#pragma unroll
    for (int k = 0; k < RG / RB; ++k) v += ld_agent(partial + threadIdx.x + k * RB);
    return block_sum<RB>(v, red);
}

// Split barrier.  fused_arrive: this workgroup's phase-1 stores have been performed, its arrival is published.  fused_wait -- true: every
// workgroup has arrived and this one may go on; false: it ran out of patience (it must mark its chunk pending and leave).  Workgroup 0
// collects the arrivals and releases the others.  Between the two a workgroup does the part of phase 2 that needs no global sum.
__device__ __forceinline__ void fused_arrive(unsigned int* bar, unsigned int target, int* flag)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0) *flag = 1;
    __syncthreads();
    if (blockIdx.x != 0 && threadIdx.x == 0) __hip_atomic_store(&bar[blockIdx.x * BAR_LINE], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool fused_wait(unsigned int* bar, unsigned int target, long long maxPolls, int testMode, int* flag)
{
    const unsigned int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0) {
        if (testMode & 2) { if (tid == 0) *flag = 0; }
        else
        for (unsigned int w = tid; w < (unsigned int)RG; w += RB) {
            if (w == 0) continue;
            long long polls = 0;
            while (__hip_atomic_load(&bar[w * BAR_LINE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != target) {
                if (++polls > maxPolls) { *flag = 0; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        if (*flag != 0 && tid < 64) __hip_atomic_store(&bar[(RG + tid) * BAR_LINE], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if (tid == 0) {
            const unsigned int* line = &bar[(RG + (b & 63u)) * BAR_LINE];
            long long polls = 0;
            if ((testMode & 1) && b % 3u == 1u) *flag = 0;
            else
            while (__hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != target) {
                if (++polls > 2 * maxPolls) { *flag = 0; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const bool ok = *flag != 0;
    __syncthreads();
    return ok;
}

// the scalars of phase 2, from the complete partial sums (every workgroup: the same bits)
struct FusedScalars { double res, wArA, beta; bool conv, cont; };
template <bool AGENT>
__device__ __forceinline__ FusedScalars fused_scalars(const PcgState* st, int it, const double* partial3, const double* partial1, double wArAold, double* red)
{
    FusedScalars q;
    q.res = (AGENT ? sum_partials_agent(partial3, red) : sum_partials(partial3, red)) / st->normFactor;
    q.conv = sp_converged(st, q.res);                                           // SolverPerformance.C:60-92
    q.cont = (it < st->maxIter && !q.conv) || (it + 1 < st->minIter);           // PCG.C:197-204
    q.wArA = AGENT ? sum_partials_agent(partial1, red) : sum_partials(partial1, red);
    q.beta = q.wArA / wArAold;
    return q;
}
// closing duties of the launch (one thread): what k_pcg_update_psi_r's and k_pcg_final's leading threads record
__device__ __forceinline__ void fused_close(PcgState* st, int it, double alpha, double wApA, const FusedScalars& q, double* hist, int histLen)
{
    st->alpha = alpha; st->wApA = wApA;
    st->finalResidual = q.res;
    if (it + 1 < histLen) hist[it + 1] = q.res;
    st->nIterations = it + 1;
    st->it = it + 1;              // (k_pcg_final advances it too: the persistent kernel starts a later batch from it)
    st->converged = q.conv;
    if (q.cont) st->wArA[(it + 1) & 1] = q.wArA; else st->done = 1;
    st->pApplyItP1 = st->rItP1;   // psi is complete here: nothing is owed to a later pass (pcg_flush)
}

template <int PMODE>   // 1: diagonal preconditioner (z = rD o rA), 2: none (z = rA)
__global__ __launch_bounds__(RB, 8) void k_pcg_fused_r_p(FusedArgs a)
{
    extern __shared__ double2 zLds[];            // FUSED_LP pairs
    __shared__ double red[RB / 64];
    __shared__ int flag;
    PcgState* __restrict__ st = a.st;
    if (st->done) return;
    const int it = a.it;
    const unsigned int b = blockIdx.x, tid = threadIdx.x;
    const bool lead = b == 0 && tid == 0;
    // ---- phase 1: k_pcg_update_psi_r ------------------------------------------------------------------------------------------
    const double wApA = sum_partials(a.partial2, red);
    if (fabs(wApA) / st->normFactor < SP_VSMALL) { // checkSingularity, SolverPerformance.C:32-44: `break` before psi / rA move (every workgroup takes this branch)
        if (tid == 0) a.partial3[b] = -1.0;       // (the marker k_pcg_final reads: kept for a reader of the partials)
        if (lead) { st->singular = 1; st->done = 1; }
        return;
    }
    const double wArAold = st->wArA[it & 1];
    const double alpha = wArAold / wApA;
    const Chunk ck = my_chunk(a.n);
    // the chunk's own base pointers (uniform) and 32-bit indices inside it: the z values need the registers
    const double* __restrict__ wA = a.wA + ck.lo; const double* __restrict__ rD = a.rD + (PMODE == 1 ? ck.lo : 0);
    double* __restrict__ rA = a.rA + ck.lo; double* __restrict__ pA = a.pA + ck.lo; double* __restrict__ psi = a.psi + ck.lo;
    const int len = (int)(ck.hi - ck.lo), np = len >> 1;
    const bool oddTail = (len & 1) && tid == 0;
    double acc0 = 0, acc1 = 0, d0 = 0, d1 = 0;
    double2 zr[FUSED_HR];
    double zTail = 0.0;
    auto residual2 = [&](int i) -> double2 {
        const double2 w = ld2_stream(wA, i);
        double2 r = ld2(rA, i);
        r.x = fma(-alpha, w.x, r.x); r.y = fma(-alpha, w.y, r.y);
        st2(rA, i, r); acc0 += fabs(r.x); acc1 += fabs(r.y);
        double2 z = r;
        if (PMODE == 1) { const double2 d = ld2_rd(rD, i); z.x = d.x * r.x; z.y = d.y * r.y; }
        d0 = fma(z.x, r.x, d0); d1 = fma(z.y, r.y, d1);
        return z;
    };
#pragma unroll
    for (int k = 0; k < FUSED_HR; ++k) {
        const int q = (int)tid + k * RB;
        zr[k] = make_double2(0.0, 0.0);
        if (q < np) zr[k] = residual2(2 * q);
    }
    for (int q = (int)tid + FUSED_HR * RB; q < np; q += RB) {
        const double2 z = residual2(2 * q);
        const int l = q - FUSED_HR * RB;
        if (l < FUSED_LP) zLds[l] = z;
    }
    if (oddTail) {
        const int i = len - 1;
        const double r = fma(-alpha, wA[i], rA[i]); rA[i] = r; acc0 += fabs(r);
        zTail = (PMODE == 1) ? rD[i] * r : r;
        d0 = fma(zTail, r, d0);
    }
    const double t = block_sum<RB>(acc0 + acc1, red);
    const double u = block_sum<RB>(d0 + d1, red);
    if (tid == 0) { st_agent(a.partial3 + b, t); st_agent(a.partial1 + b, u); }
    fused_arrive(a.bar, a.gen, &flag);
    // in the barrier's shadow: psi += alpha pA of the first FUSED_PF strides needs no global sum; their pA values stay in registers for phase 2
    double2 pf[FUSED_PF];
#pragma unroll
    for (int k = 0; k < FUSED_PF; ++k) {
        const int q = (int)tid + k * RB;
        pf[k] = make_double2(0.0, 0.0);
        if (q < np) {
            const int i = 2 * q;
            pf[k] = ld2(pA, i);
            double2 x = ld2_stream(psi, i);
            x.x = fma(alpha, pf[k].x, x.x); x.y = fma(alpha, pf[k].y, x.y);
            st2_stream(psi, i, x);
        }
    }
    if (!fused_wait(a.bar, a.gen, a.maxPolls, a.testMode, &flag)) {
        // out of patience: (the rest of) phase 2 of this chunk and workgroup 0's closing duties are left to k_pcg_fused_finish
        if (tid == 0) __hip_atomic_store(&a.bar[FUSED_PEND_AT + b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lead) __hip_atomic_store(&a.bar[FUSED_PEND_AT + RG], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // ---- phase 2: k_pcg_final of iteration it, then k_pcg_update_p of iteration it + 1 ------------------------------------------
    const FusedScalars sc = fused_scalars<true>(st, it, a.partial3, a.partial1, wArAold, red);
    const bool cont = sc.cont;
    const double beta = sc.beta;
    auto direction2 = [&](int i, double2 z) {
        const double2 p = ld2(pA, i);
        double2 x = ld2_stream(psi, i);
        x.x = fma(alpha, p.x, x.x); x.y = fma(alpha, p.y, x.y);
        st2_stream(psi, i, x);
        if (cont) st2(pA, i, make_double2(fma(beta, p.x, z.x), fma(beta, p.y, z.y)));
    };
#pragma unroll
    for (int k = 0; k < FUSED_HR; ++k) {
        const int q = (int)tid + k * RB;
        if (q < np) {
            if (k < FUSED_PF) { if (cont) st2(pA, 2 * q, make_double2(fma(beta, pf[k].x, zr[k].x), fma(beta, pf[k].y, zr[k].y))); }
            else direction2(2 * q, zr[k]);
        }
    }
    for (int q = (int)tid + FUSED_HR * RB; q < np; q += RB) {
        const int l = q - FUSED_HR * RB, i = 2 * q;
        double2 z;
        if (l < FUSED_LP) z = zLds[l];
        else { z = ld2(rA, i); if (PMODE == 1) { const double2 d = ld2_rd(rD, i); z.x = d.x * z.x; z.y = d.y * z.y; } }   // beyond the chip: formed again (this thread's own stores)
        direction2(i, z);
    }
    if (oddTail) {
        const int i = len - 1;
        const double p = pA[i];
        psi[i] = fma(alpha, p, psi[i]);
        if (cont) pA[i] = fma(beta, p, zTail);
    }
    if (lead) fused_close(st, it, alpha, wApA, sc, a.hist, a.histLen);
}

// behind every fused launch: phase 2 of the chunks whose workgroup left the barrier early (normally none: one load and out)
template <int PMODE>
__global__ __launch_bounds__(RB) void k_pcg_fused_finish(FusedArgs a)
{
    __shared__ double red[RB / 64];
    const unsigned int b = blockIdx.x, tid = threadIdx.x;
    unsigned int* pend = a.bar + FUSED_PEND_AT;
    PcgState* __restrict__ st = a.st;
    // k_pcg_final's note, which the fused launch replaces: the k_pcg_update_p of this iteration (if one ran) has added the psi
    // term iteration it - 1 owed.  fused_close records the same when the launch completes; this covers the launches that return
    // at once (solve done, singular direction), where a deferred term added by that k_pcg_update_p would otherwise be flushed twice
    if (b == 0 && tid == 0 && st->rItP1 >= a.it) st->pApplyItP1 = a.it;
    const bool mine = pend[b] != 0u, closing = b == 0 && pend[RG] != 0u;
    if (!mine && !closing) return;
    const int it = a.it;
    const double wApA = sum_partials(a.partial2, red);
    const double wArAold = st->wArA[it & 1];
    const double alpha = wArAold / wApA;
    const FusedScalars sc = fused_scalars<false>(st, it, a.partial3, a.partial1, wArAold, red);
    if (mine) {
        const Chunk ck = my_chunk(a.n);
        const double* __restrict__ rD = a.rD + (PMODE == 1 ? ck.lo : 0); const double* __restrict__ rA = a.rA + ck.lo;
        double* __restrict__ pA = a.pA + ck.lo; double* __restrict__ psi = a.psi + ck.lo;
        const int len = (int)(ck.hi - ck.lo), np = len >> 1;
        for (int q = (int)tid; q < np; q += RB) {
            const int i = 2 * q;
            double2 z = ld2(rA, i);
            if (PMODE == 1) { const double2 d = ld2_rd(rD, i); z.x = d.x * z.x; z.y = d.y * z.y; }
            const double2 p = ld2(pA, i);
            if (q >= FUSED_PF * RB) {   // (the first strides' psi moved before the workgroup waited)
                double2 x = ld2(psi, i);
                x.x = fma(alpha, p.x, x.x); x.y = fma(alpha, p.y, x.y);
                st2(psi, i, x);
            }
            if (sc.cont) st2(pA, i, make_double2(fma(sc.beta, p.x, z.x), fma(sc.beta, p.y, z.y)));
        }
        if ((len & 1) && tid == 0) {
            const int i = len - 1;
            const double z = (PMODE == 1) ? rD[i] * rA[i] : rA[i];
            const double p = pA[i];
            psi[i] = fma(alpha, p, psi[i]);
            if (sc.cont) pA[i] = fma(sc.beta, p, z);
        }
    }
    __syncthreads();
    if (tid == 0) { pend[b] = 0u; if (closing) { fused_close(st, it, alpha, wApA, sc, a.hist, a.histLen); pend[RG] = 0u; } }
}

} // namespace mi

namespace {

bool pcg_fused_rp_usable(const mi_matrix_s* m, int precond)
{
    const mi_ctx_s* c = m->addr->ctx;
    return c->pcgFuseRP != 0 && !comm_attached(m) && (precond == MI_PRECOND_DIAGONAL || precond == MI_PRECOND_NONE) && !c->fuseFinal;
}

// residual update of iteration `it` + direction update of iteration it + 1; MI_ERR_UNSUPPORTED (nothing ran, never tried again on this
// context) when the device cannot hold the grid
int pcg_fused_rp_launch(mi_matrix_s* m, int it, int precond)
{
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    hipStream_t s = c->stream;
    const void* fn = precond == MI_PRECOND_DIAGONAL ? (const void*)k_pcg_fused_r_p<1> : (const void*)k_pcg_fused_r_p<2>;
    const size_t lds = sizeof(double2) * (size_t)FUSED_LP;
    if (c->pcgFuseRP < 0) {   // first use on this context: can RG workgroups of this kernel be resident at once? (if not, the separate kernels)
        int perCU = 0, nCU = 0;
        (void)hipDeviceGetAttribute(&nCU, hipDeviceAttributeMultiprocessorCount, c->device);
        for (const void* f : {(const void*)k_pcg_fused_r_p<1>, (const void*)k_pcg_fused_r_p<2>}) {
            int q = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, f, RB, lds) != hipSuccess) { (void)hipGetLastError(); q = 0; }
            perCU = (f == (const void*)k_pcg_fused_r_p<1>) ? q : std::min(perCU, q);
        }
        c->pcgFuseRP = ((int64_t)perCU * nCU >= RG) ? 1 : 0;
        if (!c->pcgFuseRP) return MI_ERR_UNSUPPORTED;
    }
    if (m->fusedBar.n < (size_t)FUSED_BAR_WORDS) {
        MICHK(m->fusedBar.alloc((size_t)FUSED_BAR_WORDS));
        HIPCHK(hipMemsetAsync(m->fusedBar.p, 0, sizeof(unsigned int) * (size_t)FUSED_BAR_WORDS, s));
        m->fusedGen = 0;
    }
    if (++m->fusedGen == 0u) {   // the generation wrapped: slots hold old generations that must not be mistaken for this one
        HIPCHK(hipMemsetAsync(m->fusedBar.p, 0, sizeof(unsigned int) * BAR_LINE * (size_t)(RG + 64), s));
        m->fusedGen = 1u;
    }
    FusedArgs A;
    A.st = c->state.p; A.it = it;
    A.partial1 = c->partial.p; A.partial2 = c->partial.p + RG; A.partial3 = c->partial.p + 2 * RG;
    double *psi, *pA, *wA, *rA;
    MICHK(m->vecs({{WV_PSI, &psi}, {WV_PA, &pA}, {WV_WA, &wA}, {WV_RA, &rA}}));
    A.wA = wA; A.rD = m->rD.p; A.pA = pA; A.psi = psi; A.rA = rA; A.n = a->L.nCells;
    A.hist = m->hist.p; A.histLen = m->histLen;
    A.bar = m->fusedBar.p; A.gen = m->fusedGen;
    static const long long polls = (long long)sw::get(SW_PCG_FUSE_POLLS);
    A.maxPolls = polls;
    A.testMode = c->pcgFuseTest;
    void* args[1] = {&A};
    static const int coop = sw::get(SW_PCG_FUSE_COOP);   // 1 (A/B): hipLaunchCooperativeKernel -- ~22 us per launch on this runtime
    if (coop) {
        if (hipLaunchCooperativeKernel(fn, dim3(RG), dim3(RB), args, (unsigned int)lds, s) != hipSuccess) {
            (void)hipGetLastError();
            c->pcgFuseRP = 0;
            return MI_ERR_UNSUPPORTED;
        }
    } else if (precond == MI_PRECOND_DIAGONAL) k_pcg_fused_r_p<1><<<RG, RB, lds, s>>>(A);
    else k_pcg_fused_r_p<2><<<RG, RB, lds, s>>>(A);
    if (precond == MI_PRECOND_DIAGONAL) k_pcg_fused_finish<1><<<RG, RB, 0, s>>>(A); else k_pcg_fused_finish<2><<<RG, RB, 0, s>>>(A);
    HIPCHK(hipGetLastError());
    c->stats[4] += 1;
    return MI_OK;
}

} // namespace
