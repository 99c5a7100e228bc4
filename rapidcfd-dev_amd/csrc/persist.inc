// persist.inc -- the PCG iteration of a SMALL matrix as one persistent cooperative kernel (included by engine.hip).
//
// PCG.C:133-204 at 1.26 M cells (108^3: the 8-GPU share of the 10 M-cell benchmark, or a small case on one GPU) is five
// launches per iteration moving 104N + 16F = 191 MB -- 32 us at this part's rates, 45-50 us with the launch boundaries.  A
// matrix of at most TMAX x nCU tiles can do better: ONE workgroup per CU owns up to TMAX tiles for the whole batch of
// iterations and keeps its rows' rA, pA and psi in REGISTERS (one row per thread and tile), the Amul result and diag in LDS
// behind the tile image; per iteration only the coefficient segments, the row entries and the neighbour tiles' pA values
// cross the memory system (~74 MB at 108^3), and the
// three points where the reference synchronises (pA complete before Amul, the two global sums) become grid barriers:
//   phase 1  beta ; pA = rD o rA + beta pA (registers) ; pA -> global for the other tiles' halo          | barrier
//   phase 2  per tile: coefficients -> LDS, own pA from registers, halo pA gathered, row loop (the tile kernel's
//            fma chain, term by term) ; wA stays in LDS ; workgroup partial of wA.pA                    | barrier
//   phase 3  alpha ; psi += alpha pA ; rA -= alpha wA ; workgroup partials of sum|rA| and rA.(rD o rA)   | barrier
//            every workgroup adds the partials in workgroup order (same bits everywhere), evaluates the reference's
//            convergence rule itself, workgroup 0 records it
// Sums are grouped per workgroup here and per block / per tile in the five-launch pipeline: histories agree with it (and with
// the oracle) to rounding, not bit for bit; the Amul itself is the tile kernel's, bit for bit.
// DIST (a matrix with peer windows attached, one rank per device): the same kernel is the whole DISTRIBUTED iteration -- phase 1
// also stores the tile's processor-patch cells into the neighbours' halo windows, the root of the first barrier raises the
// neighbours' flags, a workgroup polls its own flags before its first boundary tile and gathers neighbour-rank values straight
// from the window, and the two summing barriers ARE all-reduces through the replicated slots of the communicator's windows
// (dist_sum_barrier): no launch, no collective call and no host involvement per iteration.
namespace mi {

#ifndef MI_PERSIST_XREG_DIST
#define MI_PERSIST_XREG_DIST 1
#endif

// the rank's neighbours for the distributed form (DIST): the all-reduce windows of the communicator and the halo windows of
// the matrix (peer.inc); unused otherwise
struct PersistDist {
    PeerAR ar;
    const double* myVals; const unsigned long long* myFlags; const int32_t* recvPatch; int32_t nRecv, nExt, parStride;   // my halo window
    unsigned long long* const* dstFlag; int32_t nSend;               // the neighbours' flag pairs of the patches I send
    const int32_t *tileSendStart, *sendLocal;                        // per tile: which of its cells go into a neighbour's window (index into the workgroup's [TMAX][1024] rows) ...
    double* const* sendDst; int32_t nSendTot;                        // ... and where: [2 parities][nSendTot] addresses over there
    const int32_t* tileBoundary;                                     // 1: the tile gathers neighbour-rank values
    unsigned long long* haloEpoch; int32_t* haloStatus; long long maxPolls;
    unsigned long long* fusedEpoch;                                  // labels of the all-reduces through the replicated part of the windows
    double* scal;                                                    // [0] sum wA.rA, [1] sum|rA| (global), as the five-launch loop keeps them
    int32_t nCells;
};

struct PersistArgs {
    TileArgs t;                 // layout + coefficients (x / y unused)
    PcgState* st;
    double *psi, *rA, *pA; const double* rD;
    double *pB, *Z;             // (single rank) the second pA buffer and z = rD o rA of the residual update: see ZP in the kernel
    double* P1;                 // in: RG partials of rA.(rD o rA) from the prologue / the previous batch; out: {rho, 0, ...}
    double* wgPartial;          // [3][G]: wA.pA | sum|rA| | rho
    unsigned int* bar;          // grid barrier words (grid_barrier)
    double* hist; int histLen;
    int nIt, nTiles, tilesPerWG, pmode;   // pmode 1: diagonal, 2: none
    int zpMaxTiles;             // ZP (see the kernel) for at most this many tiles per workgroup
    int offPersist;             // doubles: where the workgroup's resident arrays start in LDS (behind the tile image)
    long long barPolls;         // polls before a grid-barrier wait gives up (BAR_POLLS; MI_PERSIST_BAR_POLLS shortens it in the fault tests)
    int skipArrival;            // fault injection (tests, MI_PERSIST_SKIP_ARRIVAL = n > 0): the last workgroup never arrives at its n-th barrier
    PersistDist d;
};

// (pair_key, the self-validating pair {bits, bits ^ key(label, i)}: peer.inc)
// Grid barrier for G <= 1024 co-resident workgroups (cooperative launch), without read-modify-write atomics and without cache
// maintenance: everything the workgroups exchange (pA values, partial sums, these words) is written with agent-scope stores
// (write-through) and read with agent-scope loads, so a barrier only has to ORDER, not to flush: every workgroup stores the
// generation number into its own arrival slot; thread t of workgroup 0 polls slot t; once all have arrived workgroup 0 does the
// ROOT WORK of this barrier (DIST: adds the workgroups' partial sums and all-reduces them with the other ranks, raises the
// neighbours' halo flags) and lanes 0..63 store the generation -- and NV values as pairs -- into 64 release copies on separate
// lines; workgroup b polls copy b % 64.  Three memory latencies per barrier.
// (Measured, 32 .. 1231 tiles: one counter + one flag + acquire loads in the poll loop 25 us per barrier -- every acquire
// invalidates the poller's L2 --; two-level counters + 64 release copies + device-scope fences 10 us; this one ~4 us.)
// bar: 32-bit words; arrival slot of workgroup b at b * BAR_LINE, release copy c at (1024 + c) * BAR_LINE: {generation, -, NV pairs}.
// pre(): workgroup 0, before it waits for the arrivals (address loads the root work needs: their latency hides in the wait).
constexpr int BAR_LINE = 16;                       // 32-bit words per slot (64 bytes)
constexpr int BAR_WORDS = BAR_LINE * (1024 + 64);
constexpr long long BAR_POLLS = 4000000ll;         // a few seconds
static_assert(sw::table[SW_PERSIST_BAR_POLLS].dflt == BAR_POLLS, "switches.hpp: the default of MI_PERSIST_BAR_POLLS is BAR_POLLS");
template <int NV, class Pre, class Root>
__device__ __forceinline__ void grid_barrier(unsigned int* bar, unsigned int G, unsigned int& gen, bool& barDead, PcgState* st, double (&vals)[NV > 0 ? NV : 1], double* red16, Pre pre, Root root,
                                             long long maxPolls = BAR_POLLS, bool arrive = true)
{
    static_assert(NV <= 3, "a release line holds three pairs");
    const unsigned int target = gen + 1u, b = blockIdx.x, tid = threadIdx.x;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);                     // this wave's stores of the phase have been performed ...
    __syncthreads();                                   // ... and every other wave's of the workgroup
    if (b == 0) {
        pre();
        if (tid > 0 && tid < G) {
            long long polls = 0;
            while (!barDead && __hip_atomic_load(&bar[tid * BAR_LINE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != target) {
                if (++polls > maxPolls) { st->fault = 2; barDead = true; break; }     // a workgroup that never arrives must not hang the device (and is not waited for twice)
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        root(vals);                                    // on return: the values to hand out, in every thread of the workgroup
        if (tid < 64) {
            unsigned int* line = &bar[(1024 + tid) * BAR_LINE];
            unsigned long long* q = reinterpret_cast<unsigned long long*>(line + 2);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(vals[i]);
                __hip_atomic_store(q + 2 * i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(q + 2 * i + 1, bits ^ pair_key(target, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(line, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (tid == 0) {
            if (arrive) __hip_atomic_store(&bar[b * BAR_LINE], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned int* line = &bar[(1024 + (b & 63u)) * BAR_LINE];
            const unsigned long long* q = reinterpret_cast<const unsigned long long*>(line + 2);
            long long polls = 0;
            while (!barDead) {
                bool ok = true;
                if (NV == 0) ok = __hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const unsigned long long v = __hip_atomic_load(q + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long c = __hip_atomic_load(q + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((v ^ c) != pair_key(target, i)) ok = false;
                    red16[i] = __longlong_as_double((long long)v);
                }
                if (ok) break;
                if (++polls > 2 * maxPolls) { st->fault = 2; barDead = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) vals[i] = red16[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    gen = target;
}

// sum of G per-workgroup partials in workgroup order, in every thread of the calling workgroup (G <= 1024)
__device__ __forceinline__ double sum_wg_partials(const double* __restrict__ p, int G, double* red16)
{
    double v = (int)threadIdx.x < G ? __hip_atomic_load(p + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red16[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += red16[w];
    return t;
}
template <int BS>
__device__ __forceinline__ double wg_sum(double v, double* red16)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red16[0];
#pragma unroll
    for (int w = 1; w < BS / 64; ++w) t += red16[w];
    return t;
}
// DIST: a summing barrier IS an all-reduce through the replicated part of the communicator's windows (comm.inc: PEER_REP copies
// of [rank][PEER_FSLOT] per parity).  Workgroup 0 waits for the arrivals, adds the workgroups' partials (workgroup order) and
// stores the rank's sums as PAIRS keyed by the label e into all PEER_REP copies of EVERY rank's window, its own included
// (write-through system-scope stores, lane = copy); every workgroup of every rank polls copy b % PEER_REP of its own window
// until all ranks' pairs carry the label and adds them in rank order -- the same bits in every workgroup of every rank.
// The rank's own pairs appear only after all its workgroups arrived: they are the release of the local barrier too.
// Two parities suffice: a rank issues all-reduce n + 2 after every rank issued n + 1, i.e. after all their workgroups read n.
template <int NV>
__device__ __forceinline__ void dist_sum_barrier(const PersistArgs& a, unsigned int G, unsigned int& gen, bool& barDead, const double* partial,
                                                 unsigned long long e, bool& dead, double (&vals)[NV], double* red16, double* arGot /* LDS: NV x 64 doubles + 1 */)
{
    static_assert(2 * NV <= PEER_FSLOT, "the pairs must fit a replicated window slot");
    const PeerAR& A = a.d.ar;
    const unsigned int target = gen + 1u, b = blockIdx.x, tid = threadIdx.x;
    const int par = (int)(e & 1ull);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (b == 0) {
        if (tid > 0 && tid < G) {
            long long polls = 0;
            while (!barDead && __hip_atomic_load(&a.bar[tid * BAR_LINE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != target) {
                if (++polls > a.barPolls) { a.st->fault = 2; barDead = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        // (one sum at a time, straight into the stores: nothing of this block stays live beside the workgroup's rows)
#pragma unroll 1
        for (int i = 0; i < NV; ++i) {
            const double mine = sum_wg_partials(partial + (size_t)i * G, (int)G, red16);
            if (tid < 64) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(mine);
                const size_t off = (size_t)A.fusedOff + ((size_t)par * PEER_REP + tid) * (size_t)A.repStride + (size_t)A.myRank * PEER_FSLOT + (size_t)(2 * i);
#pragma unroll 1
                for (int k = 0; k < A.nRanks; ++k) {
                    unsigned long long* dst = reinterpret_cast<unsigned long long*>(A.peerWin[k] + off);   // (uniform: a scalar load)
                    __hip_atomic_store(dst, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dst + 1, bits ^ pair_key(e, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        if (tid < 64) __hip_atomic_store(&a.bar[(1024 + tid) * BAR_LINE], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // keeps the generations of the plain barriers in step
    } else if (tid == 0) __hip_atomic_store(&a.bar[b * BAR_LINE], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < (unsigned)A.nRanks) {   // lane r of wave 0 (nRanks <= 64) waits for rank r's pairs in copy b % PEER_REP of this rank's window
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(
            A.myWin + (size_t)A.fusedOff + ((size_t)par * PEER_REP + (b % PEER_REP)) * (size_t)A.repStride + (size_t)tid * PEER_FSLOT);
        long long polls = 0;
        bool gaveUp = false;
        while (!dead) {
            bool ok = true;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const unsigned long long x = __hip_atomic_load(src + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const unsigned long long c = __hip_atomic_load(src + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if ((x ^ c) != pair_key(e, i)) ok = false;
                arGot[i * 64 + tid] = __longlong_as_double((long long)x);
            }
            if (ok) break;
            if (++polls > A.maxPolls) { *A.status = 1; gaveUp = true; break; }   // a rank that never arrives must not hang the device (peer_check reports it)
            __builtin_amdgcn_s_sleep(1);
        }
        if (gaveUp) arGot[2 * 64] = 1.0;   // (fixed slot, zeroed when the kernel starts, never data)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double acc = 0.0;
#pragma unroll 1
        for (int k = 0; k < A.nRanks; ++k) acc += arGot[i * 64 + k];   // rank order: the same bits in every thread, workgroup and rank
        vals[i] = acc;
    }
    dead = dead || arGot[2 * 64] != 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    gen = target;
}

// base + 32-bit byte offset: the access keeps the (uniform) base in scalar registers and needs ONE vector register for all the
// arrays a row touches, where a 64-bit address per array and tile would be hoisted out of the iteration loop and spilled
template <class T>
__device__ __forceinline__ T* at_off(T* base, unsigned int byteOff) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byteOff); }
template <class T>
__device__ __forceinline__ const T* at_off(const T* base, unsigned int byteOff) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byteOff); }

template <int TMAX, bool DIST>
__global__ __launch_bounds__(1024) void k_pcg_persist(const PersistArgs a)
{
    constexpr int BS = 1024;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red16[16];
    __shared__ int tcs[TMAX + 1];
    __shared__ double arGot[DIST ? 2 * 64 + 1 : 1];   // DIST: what the ranks' window slots held (dist_sum_barrier); [2 * 64]: a wait gave up        // first cell of each of the workgroup's tiles (consecutive tiles own consecutive cells): c0 = tcs[k], nc = tcs[k+1] - tcs[k]
    PcgState* st = a.st;
    if (st->done) return;
    const int G = gridDim.x, b = blockIdx.x, per = G >> 3;
    const int g = (b < (per << 3)) ? (b & 7) * per + (b >> 3) : b;          // XCD x owns a contiguous run of tile groups
    const int t0 = g * a.tilesPerWG;
    const int myTiles = max(0, min(a.tilesPerWG, a.nTiles - t0));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double* cU = smem;
    double* xs = smem + a.t.offX;
    // rA and pA of the workgroup's rows live in registers (one row per thread and tile), the Amul result and diag in LDS behind
    // the tile image (2 x TMAX x 8 KB per workgroup); psi is read and written in place by its own thread once per iteration
    // (write-back cached, nobody else touches it); 1/diag is the division itself (the reference's rD = 1/diag)
    double* wS = smem + a.offPersist;
    double* dgS = wS + TMAX * BS;
    // (XREG, the single-rank form: psi in registers too -- the distributed form needs those registers for its exchanges)
    constexpr bool XREG = MI_PERSIST_XREG_DIST ? true : !DIST;
    // ZP (single rank): from the second iteration of a batch on, the barrier between the p-update and the Amul is gone.  The
    // residual update publishes z = rD o rA (the preconditioned residual the next p-update starts from) before ITS barrier; the
    // p-update then needs no barrier because a tile forms the pA of its halo cells itself, pA = z + beta pA_old -- the owner's
    // own fma on the owner's own operands, so the same bits -- from z and the PREVIOUS pA, both complete since that barrier.
    // pA alternates between two buffers (a tile reads the old one while its owner writes the new one); z needs one.
    constexpr bool ZP = !DIST;
    // (worth it while the iteration is barrier-bound: measured 13.9 -> 12.7 us at 32 tiles, 14.7 -> 13.4 at 155, nothing at two tiles
    //  per workgroup and +1 us at five, where the extra vector store and the second gathered value cost what the barrier did)
    const bool zpOn = ZP && a.tilesPerWG <= a.zpMaxTiles;
    double* const pbuf[2] = {a.pA, zpOn ? a.pB : a.pA};
    int pw = 0;                          // the buffer that holds the latest complete pA (the hand-over leaves it in a.pA)
    double r[TMAX], p[TMAX], x[XREG ? TMAX : 1];
    // c0 / nc of tile k: the table lives in LDS (uniform broadcast reads) -- held in scalar registers across the iteration loop,
    // 2 x TMAX of them, they were part of what made the compiler spill (DESIGN 3.3)
    if (tid <= TMAX) tcs[tid] = a.t.tileCellStart[t0 + min(tid, myTiles)];
    if (DIST && tid == 0) arGot[2 * 64] = 0.0;
    __syncthreads();
    auto c0_of = [&](int k) { return __builtin_amdgcn_readfirstlane(tcs[k]); };
    auto nc_of = [&](int k) { return __builtin_amdgcn_readfirstlane(tcs[k + 1] - tcs[k]); };   // 0 for k >= myTiles
    int it = st->it;
    // the psi term the five-launch loop may still owe for iteration it - 1 (deferred psi update, k_pcg_update_p)
    const bool owed = it > 0 && st->rItP1 == it && st->pApplyItP1 != it;
    const double alphaOwed = owed ? st->alpha : 0.0;
#pragma unroll
    for (int k = 0; k < TMAX; ++k) {
        r[k] = p[k] = 0.0;
        if (XREG) x[k] = 0.0;
        if (k < myTiles) {
            if (tid < nc_of(k)) {
                const unsigned int go = 8u * (unsigned int)(c0_of(k) + tid);
                r[k] = *at_off(a.rA, go); p[k] = *at_off(a.pA, go);
                if (XREG) { x[k] = *at_off(a.psi, go); if (owed) x[k] = fma(alphaOwed, p[k], x[k]); }
                else if (owed) *at_off(a.psi, go) = fma(alphaOwed, p[k], *at_off(a.psi, go));
                dgS[k * BS + tid] = *at_off(a.t.diag, go);
            }
        }
    }
    // rho of the first iteration: the RG partials the prologue (or the previous batch) left, k_pcg_update_p's sum; DIST: the
    // global value the prologue / the previous batch's last kernel left in scal[0]
    double rho, sumMag = 0.0;
    if (DIST) { rho = a.d.scal[0]; sumMag = a.d.scal[1]; }
    else {
        double v = 0.0;
        if (tid < RB) {
#pragma unroll
            for (int k = 0; k < RG / RB; ++k) v += a.P1[tid + k * RB];
        }
        v = wave_sum(v);
        __syncthreads();
        if (lane == 0) red16[wave] = v;
        __syncthreads();
        rho = red16[0];
#pragma unroll
        for (int q = 1; q < RB / 64; ++q) rho += red16[q];
    }
    double rhoOld = st->wArA[(it & 1) ^ 1];
    const double normFactor = st->normFactor, tol = st->tolerance, relTol = st->relTol, res0 = st->initialResidual;
    const int maxIter = st->maxIter, minIter = st->minIter;
    unsigned int gen = __hip_atomic_load(&a.bar[(1024 + (blockIdx.x & 63)) * BAR_LINE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // DIST: labels of this batch's exchanges = the counters as the batch found them + n (fixed while the kernel runs: workgroup 0
    // advances them at the end, as the stand-alone k_halo_push / k_peer_allreduce expect)
    const unsigned long long halo0 = DIST ? *a.d.haloEpoch : 0ull, ar0 = DIST ? *a.d.fusedEpoch : 0ull;
    unsigned int nEx = 0, nAr = 0;
    const int myRecvPatch = (DIST && tid < a.d.nRecv) ? a.d.recvPatch[tid] : 0;
    bool arDead = false, haloDead = false, barDead = false;   // a wait that ran out of polls is not repeated
    int resident = -1;               // the tile whose coefficient segment the LDS image holds right now (none yet in this launch)
    bool done = false, singular = false, converged = false;
    double res = st->finalResidual;
    int nIterations = st->nIterations;
    auto nothing = [] {};
    unsigned int nBar = 0;               // barriers this workgroup has been through in this launch (fault injection only)
    auto arrives = [&]() { ++nBar; return !(a.skipArrival > 0 && b == G - 1 && (int)nBar == a.skipArrival); };
    for (int step = 0; step < a.nIt && !done; ++step, ++it) {
        // ---- phase 1: pA = rD o rA + beta pA                                                   [PCG.C:139-160]
        const double beta = (it == 0) ? 0.0 : rho / rhoOld;
        ++nEx;
        const unsigned long long e = halo0 + nEx;
        const int par = (int)(e & 1ull);
        const bool zp = zpOn && step > 0;    // this iteration runs without the first barrier
        double* const pNew = pbuf[zpOn ? (pw ^ 1) : 0];
        const double* const pOld = pbuf[pw];
#pragma unroll
        for (int k = 0; k < TMAX; ++k) if (k < myTiles) {
            if (tid < nc_of(k)) {
                const double wv = zp ? wS[k * BS + tid] : (a.pmode == 1 ? (1.0 / dgS[k * BS + tid]) * r[k] : r[k]);   // zp: the z the residual update left
                p[k] = (it == 0) ? wv : fma(beta, p[k], wv);
                __hip_atomic_store(at_off(pNew, 8u * (unsigned int)(c0_of(k) + tid)), p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through: the other workgroups gather it after a barrier
            }
        }
        if (zpOn) pw ^= 1;
        if (DIST && myTiles > 0) {   // the workgroup's patch cells, straight into the neighbours' windows  [processorFvPatchField initEvaluate: pack + send]
            // (ONE loop over all its tiles' sends -- their table entries are contiguous --, pA staged in the LDS rows that hold
            //  the Amul result later in the iteration: a loop per tile would expose one load latency per tile)
            const int sS = a.d.tileSendStart[t0], nS = a.d.tileSendStart[t0 + myTiles] - sS;
            if (nS > 0) {
#pragma unroll
                for (int k = 0; k < TMAX; ++k) if (k < myTiles && tid < nc_of(k)) wS[k * BS + tid] = p[k];
                __syncthreads();
                for (int q = tid; q < nS; q += BS)
                    __hip_atomic_store(a.d.sendDst[(size_t)par * a.d.nSendTot + sS + q], wS[a.d.sendLocal[sS + q]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if (!zp)
        {
            double none[1];
            unsigned long long* nbrFlag = nullptr;
            grid_barrier<0>(a.bar, (unsigned)G, gen, barDead, st, none, red16,
                [&] { if (DIST && tid < a.d.nSend) nbrFlag = a.d.dstFlag[tid]; },
                [&](double (&)[1]) {
                    // every workgroup's stores into the neighbours' windows have been performed (they waited for them before they
                    // arrived; write-through stores, nothing to flush): raise the neighbours' flags
                    if (DIST && tid < a.d.nSend) __hip_atomic_store(nbrFlag + par, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }, a.barPolls, arrives());
        }
        // ---- phase 2: wA = A pA, wA.pA                                                          [PCG.C:162-166]
        double dot = 0.0;
        bool waited = false;
        // The workgroup walks its tiles forwards in even steps of the batch and backwards in odd ones: the tile it ended the
        // previous iteration with is the one it starts this one with, and that tile's coefficient segment is still in LDS
        // (the coefficients do not change during a solve) -- one staging in five saved at five tiles per workgroup, every
        // staging at one.  (wA.pA is formed after the loop in tile order, so its bits do not depend on the walk.)
        const bool backwards = (step & 1) != 0;
        for (int pass = 0; pass < (DIST ? 2 : 1); ++pass)      // DIST: the tiles that need nothing from another rank first
        for (int kk = 0; kk < myTiles; ++kk) {   // ONE copy of the tile body: the tile's registers are picked through unrolled selects
            const int k = backwards ? myTiles - 1 - kk : kk;
            const int t = t0 + k;
            if (DIST) {
                const int isB = a.d.tileBoundary[t];
                if (isB != pass) continue;
                if (isB && !waited) {
                    if (tid < a.d.nRecv) {
                        const unsigned long long* flag = a.d.myFlags + 2 * (size_t)myRecvPatch + par;
                        long long polls = 0;
                        while (!haloDead && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != e) {
                            if (++polls > a.d.maxPolls) { *a.d.haloStatus = 1; haloDead = true; break; }   // (peer_check reports it; no second wait)
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    __syncthreads();
                    waited = true;
                }
            }
            double pk = 0.0;
#pragma unroll
            for (int j = 0; j < TMAX; ++j) if (j == k) pk = p[j];
            const int nc = nc_of(k);
            const int s0 = a.t.tileSlotStart[t], ns = a.t.tileSlotStart[t + 1] - s0;
            const int h0 = a.t.tileHaloStart[t], nh = a.t.tileHaloStart[t + 1] - h0;
            if (k != resident) {   // (resident: the tile whose segment the image holds right now)
                stage_dma16<BS, true>(reinterpret_cast<const double2*>(a.t.up + s0), reinterpret_cast<double2*>(cU), ns >> 1, wave, lane);
                resident = k;
            }
            if (tid < nc) xs[tid] = pk;
            if (DIST) {
                const double* ext = a.d.myVals + (size_t)par * a.d.parStride;
                for (int q = tid; q < nh; q += BS) {
                    const int idx = a.t.haloCell[h0 + q];
                    xs[nc + q] = idx < a.d.nCells ? __hip_atomic_load(a.pA + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                  : __hip_atomic_load(ext + (idx - a.d.nCells), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            } else
                for (int q = tid; q < nh; q += BS) {
                    const int idx = a.t.haloCell[h0 + q];
                    if (zp) xs[nc + q] = fma(beta, __hip_atomic_load(pOld + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                             __hip_atomic_load(a.Z + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));   // (it > 0 here: the owner's fma)
                    else xs[nc + q] = __hip_atomic_load(pNew + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            const int sl0 = a.t.tileSliceStart[t], nsl = a.t.tileSliceStart[t + 1] - sl0;
            int width = 0, e0 = 0;
            uint32_t en[8];
            const uint32_t padEnt = (uint32_t)(ns - 1) << 16;
            if (wave < nsl) {
                e0 = __builtin_amdgcn_readfirstlane(a.t.sliceEntryStart[sl0 + wave]);
                const int e1 = __builtin_amdgcn_readfirstlane(a.t.sliceEntryStart[sl0 + wave + 1]);
                width = (e1 - e0) >> 6;
                const uint32_t* ent = a.t.entries + e0 + lane;
#pragma unroll
                for (int j = 0; j < 8; ++j) en[j] = (j < width) ? ent[j * 64] : padEnt;
            }
            __syncthreads();
            double acc = 0.0;
            const bool live = tid < nc;
            if (wave < nsl) {
                const double xi = live ? pk : 0.0;
                acc = (live ? dgS[k * BS + tid] : 0.0) * xi;
#pragma unroll
                for (int j = 0; j < 8; ++j) if (j < width) acc = fma(cU[(en[j] >> 16) & 0x7FFFu], xs[en[j] & 0xFFFFu], acc);
                if (width > 8) {
                    const uint32_t* ent = a.t.entries + e0 + lane;
                    for (int j = 8; j < width; ++j) { const uint32_t ee = ent[j * 64]; acc = fma(cU[(ee >> 16) & 0x7FFFu], xs[ee & 0xFFFFu], acc); }
                }
            }
            if (live) wS[k * BS + tid] = acc;
            __syncthreads();       // the image is free for the next tile
        }
#pragma unroll
        for (int k = 0; k < TMAX; ++k) if (k < myTiles && tid < nc_of(k)) dot = fma(wS[k * BS + tid], p[k], dot);   // wA.pA, tile order
        {
            const double tsum = wg_sum<BS>(dot, red16);
            if (tid == 0) __hip_atomic_store(a.wgPartial + g, tsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // DIST (psi not in registers): its loads are issued before the barrier and complete while the workgroup waits
        double xv[XREG ? 1 : TMAX];
        if (!XREG) {
#pragma unroll
            for (int k = 0; k < TMAX; ++k) xv[k] = (k < myTiles && tid < nc_of(k)) ? *at_off(a.psi, 8u * (unsigned int)(c0_of(k) + tid)) : 0.0;
        }
        double wApA;
        if (DIST) {   // the barrier is an all-reduce through the windows (dist_sum_barrier)
            double v1[1];
            ++nAr;
            dist_sum_barrier<1>(a, (unsigned)G, gen, barDead, a.wgPartial, ar0 + nAr, arDead, v1, red16, arGot);
            wApA = v1[0];
        } else {      // every workgroup adds the partials itself (one latency less than a hand-out)
            double none[1];
            grid_barrier<0>(a.bar, (unsigned)G, gen, barDead, st, none, red16, nothing, [](double (&)[1]) {}, a.barPolls, arrives());
            wApA = sum_wg_partials(a.wgPartial, G, red16);
        }
        if (fabs(wApA) / normFactor < SP_VSMALL) { singular = true; done = true; break; }   // checkSingularity: `break`, nIterations not incremented
        const double alpha = rho / wApA;
        // ---- phase 3: psi += alpha pA ; rA -= alpha wA ; sum|rA| ; next rho                     [PCG.C:170-195, 139-142]
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < TMAX; ++k) if (k < myTiles && tid < nc_of(k)) {
            if (XREG) x[k] = fma(alpha, p[k], x[k]);
            else *at_off(a.psi, 8u * (unsigned int)(c0_of(k) + tid)) = fma(alpha, p[k], xv[k]);
            r[k] = fma(-alpha, wS[k * BS + tid], r[k]);
            s1 += fabs(r[k]);
            const double z = a.pmode == 1 ? (1.0 / dgS[k * BS + tid]) * r[k] : r[k];   // rD o rA: what the next p-update starts from
            s2 = fma(z, r[k], s2);
            if (zpOn) {
                wS[k * BS + tid] = z;
                __hip_atomic_store(at_off(a.Z, 8u * (unsigned int)(c0_of(k) + tid)), z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        {
            const double u1 = wg_sum<BS>(s1, red16), u2 = wg_sum<BS>(s2, red16);
            if (tid == 0) {
                __hip_atomic_store(a.wgPartial + G + g, u1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.wgPartial + 2 * G + g, u2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        rhoOld = rho;
        if (DIST) {
            double v2[2];
            ++nAr;
            dist_sum_barrier<2>(a, (unsigned)G, gen, barDead, a.wgPartial + G, ar0 + nAr, arDead, v2, red16, arGot);
            sumMag = v2[0]; rho = v2[1];
        } else {
            double none[1];
            grid_barrier<0>(a.bar, (unsigned)G, gen, barDead, st, none, red16, nothing, [](double (&)[1]) {}, a.barPolls, arrives());
            sumMag = sum_wg_partials(a.wgPartial + G, G, red16);
            rho = sum_wg_partials(a.wgPartial + 2 * G, G, red16);
        }
        res = sumMag / normFactor;
        nIterations = it + 1;
        converged = (res < tol) || (relTol > SP_SMALL && res < relTol * res0);
        const bool cont = (it < maxIter && !converged) || (it + 1 < minIter);
        if (b == 0 && tid == 0 && it + 1 < a.histLen) a.hist[it + 1] = res;
        if (!cont) { done = true; ++it; break; }
    }
    // ---- hand the state back: vectors, scalars, the partial slots the five-launch kernels read
#pragma unroll
    for (int k = 0; k < TMAX; ++k) if (k < myTiles && tid < nc_of(k)) {
        const unsigned int go = 8u * (unsigned int)(c0_of(k) + tid);
        *at_off(a.rA, go) = r[k]; *at_off(a.pA, go) = p[k];
        if (XREG) *at_off(a.psi, go) = x[k];
    }
    if (b == 0) {
        if (!DIST) for (int i = tid; i < RG; i += BS) a.P1[i] = (i == 0) ? rho : 0.0;
        if (tid == 0) {
            if (DIST) { a.d.scal[0] = rho; a.d.scal[1] = sumMag; *a.d.haloEpoch = halo0 + nEx; *a.d.fusedEpoch = ar0 + nAr; }
            st->it = it; st->nIterations = nIterations; st->finalResidual = res; st->converged = converged ? 1 : 0;
            st->wArA[(it & 1) ^ 1] = rhoOld;      // what k_pcg_update_p(it) would find as the previous iteration's
            if (singular) st->singular = 1;
            if (done) st->done = 1;
            st->rItP1 = 0; st->pApplyItP1 = 0;    // nothing deferred: psi is complete
        }
    }
}

// Start-up litmus of the grid barrier (once per context, before the persistent kernel is ever used).  What the barrier ASSUMES
// of the hardware, beyond the HIP memory model: an agent-scope relaxed store that a wave has waited for (s_waitcnt 0) has been
// performed at the device-coherent level (write-through), so an agent-scope relaxed load issued by ANY workgroup after it has
// observed the barrier's generation word -- itself stored after that wait -- returns the new value.  The litmus runs `rounds`
// generations of exactly that pattern on the full cooperative grid: every workgroup publishes a payload line and a partial sum
// that depend on (generation, workgroup), crosses the barrier, and checks the payload of three other workgroups and the sum of
// all partials.  Any stale value counts as an error; a wait that runs out raises `fault`.  The persistent kernels are only
// enabled on a context whose litmus came back clean (persist_fits_layout).
__global__ __launch_bounds__(1024) void k_barrier_litmus(unsigned int* bar, double* payload /* [2][G][8] */, double* partial /* [G] */, PcgState* st, int* errors, int rounds, long long maxPolls)
{
    __shared__ double red16[16];
    const int G = gridDim.x, b = blockIdx.x, tid = threadIdx.x;
    unsigned int gen = __hip_atomic_load(&bar[(1024 + (b & 63)) * BAR_LINE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool barDead = false;
    int bad = 0;
    auto nothing = [] {};
    for (int r = 1; r <= rounds; ++r) {
        double* mine = payload + ((size_t)(r & 1) * G + b) * 8;
        if (tid < 8) __hip_atomic_store(mine + tid, (double)(r * 4096 + b * 8 + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) __hip_atomic_store(partial + b, (double)(r + b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double none[1];
        grid_barrier<0>(bar, (unsigned)G, gen, barDead, st, none, red16, nothing, [](double (&)[1]) {}, maxPolls);
        if (tid < 24) {
            const int o = (b + 1 + (tid >> 3) * (G / 3 + r)) % G, w = tid & 7;
            const double v = __hip_atomic_load(payload + ((size_t)(r & 1) * G + o) * 8 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v != (double)(r * 4096 + o * 8 + w)) ++bad;
        }
        const double tot = sum_wg_partials(partial, G, red16);
        if (tid == 0 && tot != (double)G * r + 0.5 * (double)G * (double)(G - 1)) ++bad;
        // the partial slots are rewritten next round: nobody may still be adding them (the payload alternates between two copies)
        grid_barrier<0>(bar, (unsigned)G, gen, barDead, st, none, red16, nothing, [](double (&)[1]) {}, maxPolls);
    }
    if (bad) atomicAdd(errors, bad);
}

} // namespace mi

namespace {
// The kernel is instantiated for 1, 2, 3 and 5 tiles per workgroup: a matrix of one tile per workgroup carries one row's
// r / p / psi per thread, not five (round 3 instantiated TMAX = 5 only, and that form spilled: DESIGN 3.3)
constexpr int PERSIST_TMAX = 5;
// dynamic LDS the kernels may ask for: the 160 KB of a CU minus their static arrays (red16, the tile table, and in the
// distributed form the 1 KB the window all-reduce lands in)
constexpr size_t PERSIST_LDS_MAX = 157 * 1024;
int persist_tmax_for(int tilesPerWG) { return tilesPerWG <= 1 ? 1 : tilesPerWG == 2 ? 2 : tilesPerWG == 3 ? 3 : 5; }
const void* persist_fn(int tmax, bool dist)
{
    switch (tmax) {
    case 1: return dist ? (const void*)k_pcg_persist<1, true> : (const void*)k_pcg_persist<1, false>;
    case 2: return dist ? (const void*)k_pcg_persist<2, true> : (const void*)k_pcg_persist<2, false>;
    case 3: return dist ? (const void*)k_pcg_persist<3, true> : (const void*)k_pcg_persist<3, false>;
    default: return dist ? (const void*)k_pcg_persist<5, true> : (const void*)k_pcg_persist<5, false>;
    }
}
int persist_grid(const mi_ctx_s* c)
{
    const int all = std::min(1024, (c->nCU / 8) * 8);
    return c->persistGrid >= 8 ? std::min(all, (c->persistGrid / 8) * 8) : all;
}
int32_t persist_tiles_per_wg(const mi_matrix_s* m)
{
    const int G = persist_grid(m->addr->ctx);
    return std::max(1, (m->addr->L.nTiles + G - 1) / std::max(G, 1));
}
size_t persist_lds(const mi_addr_s* a, int tmax, TileArgs* t, int* offPersist)
{
    TileArgs tmp;
    if (!t) t = &tmp;
    const size_t ldsImage = lds_bytes(a->L, false, false, &t->offLow, &t->offX, &t->offRD, &t->offSB);
    const int off = (int)((ldsImage + 15) / 16 * 2);
    if (offPersist) *offPersist = off;
    return sizeof(double) * ((size_t)off + (size_t)2 * (size_t)tmax * 1024);
}
// Grid-barrier litmus (k_barrier_litmus): `rounds` generations with payload and sum checks on the cooperative grid the
// persistent kernels use.  *ok = false: stale data, a wait that ran out, or a launch the runtime refused.
int persist_litmus(mi_ctx_s* c, int rounds, bool* ok)
{
    *ok = false;
    const int G = persist_grid(c);
    hipStream_t s = c->stream;
    DevBuf<unsigned int> bar; DevBuf<double> pay, part; DevBuf<PcgState> st; DevBuf<int> err;
    MICHK(bar.alloc(BAR_WORDS)); MICHK(pay.alloc((size_t)2 * (size_t)G * 8)); MICHK(part.alloc((size_t)G)); MICHK(st.alloc(1)); MICHK(err.alloc(1));
    HIPCHK(hipMemsetAsync(bar.p, 0, sizeof(unsigned int) * BAR_WORDS, s));
    HIPCHK(hipMemsetAsync(pay.p, 0, sizeof(double) * 2 * (size_t)G * 8, s));
    HIPCHK(hipMemsetAsync(part.p, 0, sizeof(double) * (size_t)G, s));
    HIPCHK(hipMemsetAsync(st.p, 0, sizeof(PcgState), s));
    HIPCHK(hipMemsetAsync(err.p, 0, sizeof(int), s));
    unsigned int* barP = bar.p; double* payP = pay.p; double* partP = part.p; PcgState* stP = st.p; int* errP = err.p;
    long long polls = 400000ll;            // a fraction of a second per wait
    void* args[7] = {&barP, &payP, &partP, &stP, &errP, &rounds, &polls};
    if (hipLaunchCooperativeKernel((const void*)k_barrier_litmus, dim3(G), dim3(1024), args, 0u, s) != hipSuccess) { (void)hipGetLastError(); return MI_OK; }
    PcgState h; int nerr = 0;
    HIPCHK(hipMemcpyAsync(&h, st.p, sizeof(PcgState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nerr, err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *ok = h.fault == 0 && nerr == 0;
    return MI_OK;
}
// the part of "usable" that depends on the rank's own layout and device: every CU can own its share of the tiles in registers
// and the runtime agrees that the grid is co-resident (ranks of a communicator AGREE on it at attach time: a rank inside the
// persistent kernel and a neighbour in the five-launch loop would wait for each other's exchanges forever)
bool persist_fits_layout(const mi_matrix_s* m)
{
    const mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    if (a->compact || !a->ami.empty()) return false;
    const int G = persist_grid(c);
    if (G < 8 || a->L.nTiles > PERSIST_TMAX * G || a->L.maxCells > 1024) return false;
    const size_t lds = persist_lds(a, persist_tmax_for(persist_tiles_per_wg(m)), nullptr, nullptr);
    if (lds > PERSIST_LDS_MAX) return false;
    if (c->persistCoop < 0) {   // once per context: cooperative launches supported, one 1024-thread workgroup per CU resident, barrier litmus clean
        int coop = 0, perCU = 0;
        c->persistCoop = 0;
        if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device) == hipSuccess && coop) {
            bool ok = true;
            for (int tm : {1, 2, 3, 5})
                for (int dist = 0; dist < 2; ++dist) {
                    const void* fn = persist_fn(tm, dist != 0);
                    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PERSIST_LDS_MAX) != hipSuccess) ok = false;
                    if (ok && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, fn, 1024, PERSIST_LDS_MAX) != hipSuccess || perCU < 1)) ok = false;
                    if (!ok && sw::get(SW_DEBUG_PERSIST)) { fprintf(stderr, "[persist] instantiation TMAX %d DIST %d refused (LDS attribute / occupancy)\n", tm, dist); break; }
                }
            // Ranks that SHARE a device (tests) would run their litmus grids side by side with the other processes' work, where a
            // short wait can run out for scheduling reasons alone; their grids are sized by hand anyway (MI_PERSIST_GRID).
            if (ok && sw::get(SW_PERSIST_LITMUS) != 0 && !c->persistShared) {
                bool clean = false;
                if (persist_litmus(c, 64, &clean) != MI_OK || !clean) ok = false;
                if (!ok && sw::get(SW_DEBUG_PERSIST)) fprintf(stderr, "[persist] the grid-barrier litmus failed: persistent kernels off on this context\n");
                c->stats[2] += 1;   // mi_ctx_stat(2): barrier litmus runs on this context
            }
            c->persistCoop = ok ? 1 : 0;
        }
        (void)hipGetLastError();
    }
    return c->persistCoop == 1;
}
bool persist_fits(const mi_matrix_s* m, int precond)
{
    if (m->addr->ctx->pcgPersist == 0 || m->asym) return false;
    if (precond != MI_PRECOND_DIAGONAL && precond != MI_PRECOND_NONE) return false;
    return persist_fits_layout(m);
}
bool pcg_persist_usable(const mi_matrix_s* m, int precond) { return !comm_attached(m) && persist_fits(m, precond); }
// attached matrices: halo and sums through the peer windows, inside the kernel; ranks that share a device cannot (two
// cooperative grids would wait for each other's workgroups)
bool dpcg_persist_usable(const mi_matrix_s* m)
{
    return peer_halo_ready(m) && m->dpc->reduce->peerReady && m->dpc->ph->persistAgreed && m->addr->ctx->pcgPersist != 0 && !m->asym;
}
// enqueue up to n_iters iterations as ONE cooperative launch (device no-op once the solve is done)
int persist_enqueue(mi_matrix_s* m, int n_iters, int precond, bool dist)
{
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    hipStream_t s = c->stream;
    double *psi, *pA, *rA;
    if (dist) { psi = m->dp.psi; pA = m->dp.pA; rA = m->dp.rA; }
    else { MICHK(m->vecs({{WV_PSI, &psi}, {WV_PA, &pA}, {WV_RA, &rA}})); }
    if (precond != MI_PRECOND_NONE) MICHK(ensure_rD(m));
    const int G = persist_grid(c);
    const size_t scratch = (size_t)3 * (size_t)G + 16 + BAR_WORDS / 2;
    // barrier words and partial slots start from zero: on allocation, and again after ANY fault this context has reported
    // since this matrix last ran here (fetch_state counts them) -- a barrier that gave up leaves arrival slots and release
    // copies on different generations, and every workgroup seeds its generation from a release copy
    if (m->persistScratch.n < scratch || m->persistFaultEpoch != c->faultEpoch) {
        if (m->persistScratch.n < scratch) MICHK(m->persistScratch.alloc(scratch));
        HIPCHK(hipMemsetAsync(m->persistScratch.p, 0, sizeof(double) * m->persistScratch.n, s));
        m->persistFaultEpoch = c->faultEpoch;
    }
    PersistArgs P;
    memset(&P, 0, sizeof(P));
    TileArgs& t = P.t;
    t.tileCellStart = a->tileCellStart.p; t.tileSlotStart = a->tileSlotStart.p; t.tileIfaceSlot0 = a->tileIfaceSlot0.p; t.tileHaloStart = a->tileHaloStart.p;
    t.haloCell = a->haloCell.p; t.tileSliceStart = a->tileSliceStart.p; t.sliceEntryStart = a->sliceEntryStart.p;
    t.entries = a->entries.p; t.entries16 = nullptr; t.sliceEntryStart16 = nullptr; t.slotBase = nullptr; t.tileSbStart = nullptr;
    t.diag = m->diagE.p; t.up = m->upE.p; t.low = nullptr; t.x = nullptr; t.b = nullptr; t.rD = nullptr; t.y = nullptr; t.omega = 0.0;
    t.dotPartial = nullptr; t.dotPartial2 = nullptr; t.flags = c->tileFlags; t.tileList = nullptr; t.nPos = a->L.nTiles; t.done = nullptr;
    P.tilesPerWG = persist_tiles_per_wg(m);
    const int tmax = persist_tmax_for(P.tilesPerWG);
    const size_t lds = persist_lds(a, tmax, &t, &P.offPersist);
    P.st = c->state.p; P.psi = psi; P.rA = rA; P.pA = pA; P.rD = m->rD.p; P.P1 = c->partial.p;
    P.pB = pA; P.Z = nullptr; P.zpMaxTiles = sw::get(SW_PERSIST_ZP);
    if (!dist) {   // ZP: the second pA buffer (the Amul result vector of the five-launch pipeline, unused here) and z
        MICHK(m->vec(WV_WA, &P.pB));
        // (z is gathered like pA: halo entries of an un-attached matrix's processor patches index the ext region behind the
        //  owned cells, which reads as zero in every engine vector -- ADVICE r03: it used to be nCells long and uninitialised)
        const size_t zLen = (size_t)a->L.nCells + (size_t)a->L.nExt;
        if (m->persistZ.n < zLen) {
            MICHK(m->persistZ.alloc(std::max(zLen, (size_t)1)));
            HIPCHK(hipMemsetAsync(m->persistZ.p, 0, sizeof(double) * std::max(zLen, (size_t)1), s));
        }
        P.Z = m->persistZ.p;
    }
    P.wgPartial = m->persistScratch.p;
    P.bar = reinterpret_cast<unsigned int*>(m->persistScratch.p + (((size_t)3 * (size_t)G + 15) & ~(size_t)15));
    P.hist = m->hist.p; P.histLen = m->histLen; P.nIt = n_iters; P.nTiles = a->L.nTiles;
    P.pmode = precond == MI_PRECOND_DIAGONAL ? 1 : 2;
    P.barPolls = (long long)sw::get(SW_PERSIST_BAR_POLLS); P.skipArrival = sw::get(SW_PERSIST_SKIP_ARRIVAL);
    if (dist) {
        PeerHalo* H = m->dpc->ph;
        PersistDist& d = P.d;
        d.ar = peer_ar(m->dpc->reduce);
        const HaloRecvDev R = halo_recv_dev(H, false);
        d.myVals = R.myVals; d.myFlags = R.myFlags; d.recvPatch = R.recvPatch; d.nRecv = R.nRecv; d.nExt = R.nExt; d.parStride = R.parStride;
        d.dstFlag = H->dstFlag.p; d.nSend = H->nSend;
        d.tileSendStart = H->tileSendStart.p; d.sendLocal = H->sendLocal.p; d.sendDst = H->sendDst.p; d.nSendTot = H->nSendTot;
        d.tileBoundary = H->tileBoundary.p; d.haloEpoch = H->epoch; d.haloStatus = H->status; d.maxPolls = PEER_POLLS;
        d.fusedEpoch = m->dpc->reduce->fusedEpoch; d.scal = m->dp.scal; d.nCells = a->L.nCells;
        if (d.nRecv > 1024 || d.nSend > 1024) return fail(MI_ERR_LIMIT, "persistent PCG: more than 1024 processor patches");
    }
    const void* fn = persist_fn(tmax, dist);
    void* args[1] = {&P};
    if (hipLaunchCooperativeKernel(fn, dim3(G), dim3(1024), args, (unsigned int)lds, s) != hipSuccess) {
        // the runtime refuses the cooperative grid after all (nothing ran): no persistent kernel on this context from now on.
        // A single-rank solve carries on with the five-launch pipeline (the caller sees MI_ERR_UNSUPPORTED); ranks of a
        // communicator cannot change path one by one, so there it is an error
        (void)hipGetLastError();
        c->persistCoop = 0;
        return dist ? fail(MI_ERR_DEVICE, "persistent distributed PCG: the cooperative launch was refused") : MI_ERR_UNSUPPORTED;
    }
    c->stats[dist ? 1 : 0] += 1;
    return MI_OK;
}
int pcg_persist_enqueue(mi_matrix_s* m, int n_iters, int precond) { return persist_enqueue(m, n_iters, precond, false); }
int dpcg_persist_enqueue(mi_matrix_s* m, int n_iters) { return persist_enqueue(m, n_iters, m->dp.precond, true); }
} // namespace
