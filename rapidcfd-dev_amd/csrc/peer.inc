// peer.inc -- halo exchange and the distributed PCG iteration over peer-mapped WINDOWS instead of collective calls.
// (included by comm.inc once mi_comm_s / mi_dpcg_comm_s and the base transport are defined)
//
// What it replaces: the processor-patch exchange of every Amul (lduMatrixUpdateMatrixInterfaces.C:30-276,
// processorFvPatchScalarField.C:36-170: pack -> MPI_Isend/Irecv through host staging -> unpack) and the three Foam::reduce
// calls of a PCG iteration (PCG.C:142,166,195 -> src/Pstream/mpi/allReduceTemplates.C:195-208).  At the 8-GPU share of the
// 10 M-cell benchmark (1.26 M cells per rank) an iteration is ~30 us of HBM traffic; a collective call costs a launch plus
// link hops each (RCCL: ~10-25 us), so the iteration was latency-, not bandwidth-bound.  On a fully connected xGMI node a
// rank can instead STORE into its neighbours' memory:
//   * every attached matrix owns a halo WINDOW ([2 parities][n_ext] values + [n_patches][2] epoch flags, fine-grained device
//     memory exported over hipIpc); a sender writes its patch values straight into the neighbour's window and then, behind a
//     system-scope release, the epoch flag of that patch; the receiver polls its own flags.  Two parities suffice: a rank can
//     only start exchange e+2 after it has seen its neighbour's exchange e+1, which the neighbour issues after consuming e.
//   * generic operators (tile_op: Amul / Tmul / residual / Jacobi of every solver, GAMG levels included): k_halo_push (pack +
//     remote stores + flags, one launch) and k_halo_pull (one workgroup: wait, copy into the operand's ext region) replace
//     k_halo_pack + event + second stream + ncclGroup{Send,Recv} + event;
//   * the distributed PCG iteration needs no collective call at all: k_dpcg_update_p (p-update + convergence test of the
//     previous iteration + deferred psi update; every block packs the patch cells of its own chunk into the neighbours'
//     windows), tile_kernel_dist (Amul over all tiles in ONE launch, interior tiles first; block 0 raises the neighbours' flags,
//     a boundary tile polls its own flags before it stages its halo and reads the window directly), k_dpcg_ar_fold (one
//     workgroup: wA.pA folded from the tile partials and all-reduced through the communicator's windows), k_dpcg_update_psi_r,
//     k_dpcg_ar_two (one workgroup: sum|rA| and the next wA.rA) -- five launches, ~51 us per iteration at the 8-GPU share of the
//     benchmark against 81 us for the phase loop over RCCL (profiles/r03_a_*).  The all-reduces can also live INSIDE the passes
//     (MI_DPCG_FUSED=3|4: block 0 sends, every block gathers; three / four launches): measured slower, see dpcg_fused_iterate.
//     The sums are formed in the order the separate reduction kernels use, so every variant gives the phase loop's bits.
// Everything is opt-in per communicator (mi_comm_peer_auto: set-up, coherence self-test and agreement between the ranks) and
// every wait is bounded: a peer that never arrives raises a status word that the solvers turn into MI_ERR_DEVICE.

namespace mi {

// A value that crosses workgroups or devices WITHOUT an ordering between it and a flag: the pair {bits, bits ^ key(label, i)}.
// A reader that finds the two words consistent for the label it expects has the value of exactly that label -- whatever order
// the two stores became visible in (a stale pair carries another label's key; a torn pair matches with probability 2^-64) --
// so a writer needs no wait between value and flag and a reader no second load: one store latency + one load latency.
__device__ __forceinline__ unsigned long long pair_key(unsigned long long label, int i)
{
    return ((label + 1ull) * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)(i + 1) * 0xD6E8FEB86659FD93ull);
}


// Window layout (doubles, nx = the owner's n_ext): [2 parities][nx] PAIRS (2 words each: tile_kernel_win, below) | [2 parities]
// [HALO_NV][nx] values | [n_patches][2] epoch flags.  Every offset depends on nx only, which a sender learns at set-up.
__host__ __device__ inline size_t halo_win_vals_off(long long nx) { return (size_t)4 * (size_t)nx; }
// A window holds up to HALO_NV operand vectors per exchange ([2 parities][HALO_NV][n_ext] values): the multi-right-hand-side
// PBiCG (multi.inc) sends pA and pT of three components in ONE exchange; every other operator uses operand slot 0.
// (HALO_NV = 6: engine.hip)
struct HaloOperands { const double* x[HALO_NV]; double* ext[HALO_NV]; int32_t n; };
struct HaloSendDev {
    double* const* dstVals;                 // [nSend] where the neighbour wants this patch's values (parity 0, operand 0)
    unsigned long long* const* dstPair;     // [nSend] ... and its pairs (parity 0; the other parity 2 x its n_ext words further)
    const long long* dstParStride;          // [nSend] doubles between the two parities over there (HALO_NV x the neighbour's n_ext)
    unsigned long long* const* dstFlag;     // [nSend] the neighbour's flag pair of the matching patch
    int32_t nSend;
    const int32_t *packStart, *packCell, *packSend, *packFace;   // pack plan sorted by owning block of the RG-block vector passes
    const int32_t *sendStart, *faceCellE;   // generic push: faces of send patch q are faceCellE[sendStart[q] .. sendStart[q+1])
    unsigned long long* epoch;              // exchanges done through the window (device counter)
    unsigned int* ticket;
};
struct HaloRecvDev {
    const double* myVals;                   // [2][nExt]
    const unsigned long long* myFlags;      // [nPatches][2]
    const int32_t* recvPatch;               // patches that receive from a neighbour rank
    const int32_t* recvOffset; const int32_t* recvSize; const double* recvFactor;  // their ext ranges (generic pull) and transformCoupleField factors
    int32_t nRecv, nExt, parStride;         // parStride = HALO_NV * nExt: doubles between the two parities of my window
    const unsigned long long* myPairs;      // pair region of my window: [2 parities][nExt][2]
    const unsigned long long* epoch;
    int32_t* status; long long maxPolls;
};

// RELAXED polls (round 4): an acquire load at system scope invalidates the poller's caches on every iteration -- hundreds of
// boundary tiles polling inside a tile kernel kept wiping the XCDs' L2 under the tiles that were computing (finest residual
// pass 165 -> 215 us).  Nothing cached is read after the wait: the window values are themselves read with system-scope
// atomic loads (fine-grained memory, never cached); the writer ordered its value stores before the flag with a system-scope
// release.  What the wait still owes is ORDER: the value loads may not be issued before the flag has been seen.  One acquire
// fence after the poll loop does that -- executed only by the wavefronts that polled (lanes r < nRecv; the others never looked
// at a flag and reach the values through the caller's workgroup barrier): an acquire at system scope is also a cache
// invalidate, so it is paid once per polling wavefront, not per iteration and not by the waves that had nothing to wait for
// (ADVICE r04: the acquire; ADVICE r05: narrowed to the polling lanes).
__device__ __forceinline__ void halo_wait_flags(const HaloRecvDev& R, unsigned long long e, int par, int tid, int stride)
{
    for (int r = tid; r < R.nRecv; r += stride) {
        const unsigned long long* flag = R.myFlags + 2 * (size_t)R.recvPatch[r] + par;
        long long polls = 0;
        const bool dead = *R.status != 0;
        while (!dead && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != e) {
            if (++polls > R.maxPolls) { *R.status = 1; break; }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    if (tid < R.nRecv) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

// generic push: pack x[patch cells] into the neighbours' windows, last block raises the flags
__global__ __launch_bounds__(256) void k_halo_push(const HaloOperands X, const HaloSendDev H)
{
    __shared__ int lastSh;
    const unsigned long long e = *H.epoch + 1;
    const int par = (int)(e & 1ull);
    // Operand 0 also goes out as self-validating pairs (the one-launch operators' form, tile_kernel_win): which form a rank
    // READS is its own choice -- a rank with cyclicAMI or transformed patches pulls values behind flags, its neighbour may read
    // pairs -- so every push writes both and any two neighbours interoperate.
    const unsigned long long key = pair_key(e, 0);
    for (int v = 0; v < X.n; ++v) {
        const double* __restrict__ x = X.x[v];
        for (int q = 0; q < H.nSend; ++q) {
            const long long ps = H.dstParStride[q];
            double* dst = H.dstVals[q] + (long long)par * ps + (long long)v * (ps / HALO_NV);
            unsigned long long* dp = H.dstPair[q] + (long long)par * 2 * (ps / HALO_NV);
            const int f0 = H.sendStart[q], nf = H.sendStart[q + 1] - f0;
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
                const double val = x[H.faceCellE[f0 + i]];
                __hip_atomic_store(dst + i, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (v == 0) {
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(val);
                    __hip_atomic_store(dp + 2 * i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dp + 2 * i + 1, bits ^ key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) lastSh = (__hip_atomic_fetch_add(H.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) ? 1 : 0;
    __syncthreads();
    if (!lastSh) return;
    for (int q = threadIdx.x; q < H.nSend; q += blockDim.x)
        __hip_atomic_store(H.dstFlag[q] + par, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) { *H.ticket = 0u; *H.epoch = e; }
}
// generic pull: wait for every neighbour's flags of the current exchange, then window -> ext region of the operand (scaled by
// the patch's transformCoupleField factor, processorGAMGInterfaceField.C:213,230)
__global__ __launch_bounds__(256) void k_halo_pull(const HaloOperands X, const HaloRecvDev R)
{
    const unsigned long long e = *R.epoch;
    const int par = (int)(e & 1ull);
    halo_wait_flags(R, e, par, threadIdx.x, blockDim.x);   // (a handful of workgroups at most: every one of them waits itself)
    __syncthreads();
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
    for (int v = 0; v < X.n; ++v) {
        const double* win = R.myVals + (size_t)par * R.parStride + (size_t)v * R.nExt;
        double* __restrict__ ext = X.ext[v];
        for (int r = 0; r < R.nRecv; ++r) {
            const int o = R.recvOffset[r], n = R.recvSize[r];
            const double f = R.recvFactor ? R.recvFactor[r] : 1.0;
            if (f == 1.0) for (int i = t0; i < n; i += T) ext[o + i] = __hip_atomic_load(win + o + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else for (int i = t0; i < n; i += T) ext[o + i] = __hip_atomic_load(win + o + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) * f;
        }
    }
}

// Every tile operator of an attached matrix over windows (tile_op: Amul / Tmul / residual / H / Jacobi of every solver and of
// every GAMG level) as ONE launch (round 4; round 3 paid k_halo_push + interior launch + k_halo_pull + boundary launch):
//   blocks [0, nPush)            the PUSH: this rank's patch values straight into the neighbours' windows as self-validating
//                                PAIRS {bits, bits ^ key(label)} -- no fence, no flag: the value is its own flag;
//   the nInterior blocks after   interior tiles: they need nothing from another rank and never look at the exchange;
//   the remaining blocks         boundary tiles: every lane that stages a neighbour-rank value polls ITS pair in this rank's
//                                window until the two words agree for the label of this exchange (tile_body, EXTWIN == 2).
// One store latency plus one load latency between the ranks (flags cost store -> fence -> ticket -> flag store -> poll -> load:
// measured 10.9 us per Jacobi sweep of a coarse level with flags against ~5 us for the same sweep without neighbours).
// The exchange's label is epoch + 1 for every block that needs it (push and boundary blocks); the LAST of those blocks to finish
// advances the epoch (a relaxed ticket: it only counts), so the counter is stable while any block may still read it and the
// next launch -- or replay of a captured hipGraph -- finds the next label.  Two parities, as for the flag protocol: a rank
// pushes exchange e + 2 only after it has read its neighbours' e + 1, which they pushed after reading e.
// Workgroups are dispatched in block order, so the push blocks of a rank that is its own neighbour run before its boundary
// tiles poll.  Ranks that SHARE a device (tests) keep the four-launch form unless MI_WIN_DIRECT=2: a boundary tile here waits
// for ANOTHER process's push, and many waiting workgroups of one process could keep the other's kernel off the device.
struct WinHead { HaloRecvDev R; HaloSendDev H; int32_t nInterior, nTiles, nPush; unsigned int* allTicket; };
template <int OP, bool ASYM, bool TRANS, int BS>
__global__ __launch_bounds__(BS, BS >= 512 ? 8 : 1) void tile_kernel_win(TileArgs a, const WinHead D)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // A solve that has converged inside a batch of enqueued iterations (`done`) skips the operator but NOT the exchange: a
    // neighbour in the four-launch form (cyclicAMI / transformed patches / 16-bit entries over there) keeps pushing and waiting
    // in k_halo_push / k_halo_pull, which do not know the flag -- every rank must count the same exchanges whichever form it
    // runs.  The push blocks push as always; the boundary blocks wait for the neighbours' FLAGS of this exchange instead of
    // their pairs (which keeps "push e + 2 only after the neighbours' e + 1"), then the epoch advances as always.
    const bool isDone = a.done && *a.done;
    const int b = (int)blockIdx.x - D.nPush, nI = D.nInterior;
    if (b >= 0 && b < nI) {
        if (isDone) return;
        const int per = nI >> 3;
        tile_body<OP, ASYM, TRANS, BS, false, false, 0>(a, (b < (per << 3)) ? (b & 7) * per + (b >> 3) : b, smem);
        return;
    }
    const unsigned long long e = *D.R.epoch + 1;
    const int par = (int)(e & 1ull);
    const unsigned long long key = pair_key(e, 0);
    if (b < 0) {
        const HaloSendDev& H = D.H;
        for (int q = 0; q < H.nSend; ++q) {
            const long long ps = H.dstParStride[q];
            unsigned long long* dst = H.dstPair[q] + (long long)par * 2 * (ps / HALO_NV);
            double* dv = H.dstVals[q] + (long long)par * ps;
            const int f0 = H.sendStart[q], nf = H.sendStart[q + 1] - f0;
            for (int i = (int)blockIdx.x * BS + (int)threadIdx.x; i < nf; i += D.nPush * BS) {
                const double val = a.x[H.faceCellE[f0 + i]];
                const unsigned long long bits = (unsigned long long)__double_as_longlong(val);
                __hip_atomic_store(dst + 2 * i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(dst + 2 * i + 1, bits ^ key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(dv + i, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // a neighbour that PULLS (cyclicAMI / transformed patches over there) reads values behind flags
            }
        }
        // ... and their flags, off the critical path of this rank's own boundary tiles (they poll pairs): the values are ordered
        // before the flag by a system-scope release fence per push block, the last push block raises the flags
        __shared__ int lastSh;
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) lastSh = (__hip_atomic_fetch_add(H.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)D.nPush - 1u) ? 1 : 0;
        __syncthreads();
        if (lastSh) {
            // the relaxed ticket only counts; what orders the OTHER push blocks' value stores (each behind its own system-scope
            // release fence) before these flags is the acquire fence here + the release on the flag stores -- paid by the last
            // push block only, not by every block (ADVICE r04)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            for (int q = threadIdx.x; q < H.nSend; q += BS) __hip_atomic_store(H.dstFlag[q] + par, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            if (threadIdx.x == 0) __hip_atomic_store(H.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (isDone) halo_wait_flags(D.R, e, par, (int)threadIdx.x, BS);
    else {
        const int bb = b - nI, per = (D.nTiles - nI) >> 3;
        const int p = nI + ((bb < (per << 3)) ? (bb & 7) * per + (bb >> 3) : bb);
        a.xPairs = D.R.myPairs + (size_t)par * 2 * (size_t)D.R.nExt;
        a.xKey = key; a.xStatus = D.R.status; a.xPolls = D.R.maxPolls;
        tile_body<OP, ASYM, TRANS, BS, false, false, 2>(a, p, smem);
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the last block that read the epoch advances it
        const unsigned int readers = (unsigned)D.nPush + (unsigned)(D.nTiles - nI);
        // relaxed: it only counts.  A block increments it after its last use of `e` (the epoch load has returned long before),
        // and the epoch store below only has to be visible to the NEXT launch (kernel boundary)
        if (__hip_atomic_fetch_add(D.allTicket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == readers - 1u) {
            __hip_atomic_store(D.allTicket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *D.H.epoch = e;
        }
    }
}

// ---- fused distributed PCG iteration ------------------------------------------------------------------------------------
// No workgroup of these kernels ever waits for another workgroup of the same launch and none issues a device-scope fence in
// the middle of its stream (measured: a threadfence + ticket per block -- the "last block reduces" pattern -- costs a full L2
// write-back per block on this multi-XCD part and made the iteration 7x slower).  What one launch produces for all blocks of
// the next is handed over at the kernel boundary; what the RANKS exchange goes through the windows with system-scope atomics:
//   * a sum over the ranks: every block forms the local sum itself from the per-block partials (the order the separate
//     reduction kernels use -- every block, every rank: the same bits), block 0 stores it into the peers' windows, EVERY block
//     waits for all ranks' slots and adds them in rank order (peer_ar_block);
//   * labels instead of "++epoch": the n-th all-reduce / halo exchange of a batch carries the label base + n, with the base in
//     device memory (fixed while the batch runs) and n a kernel argument; block 0 of the kernels that really exchanged counts
//     them, the batch's final kernel adds the count to the base -- so a batch that converges half-way leaves the counters where
//     the stand-alone k_peer_allreduce / k_halo_push expect them.
// scal: [0] sum wA.rA (global), [1] sum|rA| (global), [2] sum wA.pA (global)
struct FusedCtl {
    unsigned long long* arBase;   // labels of the all-reduces the fused passes perform themselves (the communicator's fusedEpoch; the replicated part of the windows)
    unsigned long long* haloBase; // the matrix's halo epoch
    unsigned int* used;           // [0] all-reduces, [1] halo exchanges done since the bases were last advanced
};

// all-reduce of v[0..N) over the ranks with an explicit label; called by ALL threads of EVERY block of a launch: wave 0 of
// every block gathers (block 0 also sends), the result is returned to every thread.  g: N doubles of LDS.
// the two halves: peer_ar_send by wave 0 of ONE block (lane = copy), peer_ar_gather by all threads of EVERY block
template <int N>
__device__ __forceinline__ void peer_ar_send(const PeerAR& A, unsigned long long label, const double (&v)[N])
{
    static_assert(N < PEER_FSLOT, "a fused all-reduce carries at most 3 values");
    const int r = threadIdx.x & 63;
    const int par = (int)(label & 1ull);
    const size_t mine = (size_t)A.fusedOff + ((size_t)par * PEER_REP + (size_t)r) * (size_t)A.repStride + (size_t)A.myRank * PEER_FSLOT;
    for (int k = 0; k < A.nRanks; ++k) {
        double* dst = A.peerWin[k] + mine;
#pragma unroll
        for (int i = 0; i < N; ++i) __hip_atomic_store(dst + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: the values before the labels
    for (int k = 0; k < A.nRanks; ++k)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(A.peerWin[k] + mine + (PEER_FSLOT - 1)), label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <int N>
__device__ __forceinline__ void peer_ar_gather(const PeerAR& A, unsigned long long label, double (&v)[N], double* g)
{
    if (threadIdx.x < 64) {
        const int r = threadIdx.x;
        const int par = (int)(label & 1ull);
        double got[N];
#pragma unroll
        for (int i = 0; i < N; ++i) got[i] = 0.0;
        if (r < A.nRanks) {
            const double* src = A.myWin + (size_t)A.fusedOff + ((size_t)par * PEER_REP + (size_t)(blockIdx.x % PEER_REP)) * (size_t)A.repStride + (size_t)r * PEER_FSLOT;
            const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(src + (PEER_FSLOT - 1));
            long long polls = 0;
            const bool dead = *A.status != 0;
            while (!dead && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != label) {
                if (++polls > A.maxPolls) { *A.status = 1; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
#pragma unroll
            for (int i = 0; i < N; ++i) got[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double acc = 0.0;
            for (int k = 0; k < A.nRanks; ++k) acc += __shfl(got[i], k, 64);
            if (r == 0) g[i] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = g[i];
}
template <int N>
__device__ __forceinline__ void peer_ar_block(const PeerAR& A, unsigned long long label, double (&v)[N], double* g)
{
    if (blockIdx.x == 0 && threadIdx.x < 64) peer_ar_send<N>(A, label, v);
    peer_ar_gather<N>(A, label, v, g);
}

// k_fold_final's arithmetic (fold n values into RG slots, then the RG/RB-structured sum) with BS threads: same bits
template <int BS>
__device__ __forceinline__ double fold_final_block(const double* __restrict__ in, int n, double* __restrict__ lds /* RG + RB/64 doubles */)
{
    double* folded = lds;
    double* red = lds + RG;
    for (int v = threadIdx.x; v < RG; v += BS) {
        double s = 0.0;
        for (int k = v; k < n; k += 1024) s += in[k];
        folded[v] = s;
    }
    __syncthreads();
    for (int w = threadIdx.x >> 6; w < RB / 64; w += BS / 64) {
        const int u = w * 64 + (threadIdx.x & 63);
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < RG / RB; ++k) t += folded[u + k * RB];
        t = wave_sum(t);
        if ((threadIdx.x & 63) == 0) red[w] = t;
    }
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int w = 1; w < RB / 64; ++w) r += red[w];
    return r;
}

// p-update.  AR: the two sums the previous residual update left as per-block partials (P1: next wA.rA, P3: sum|rA|) are
// all-reduced HERE, in every block (label arBase + arOff); otherwise scal[0], scal[1] already hold the global values (first
// iteration of a batch: the prologue / the previous batch's final kernel put them there).  Then the pack: every block stores
// the patch cells of its own chunk into the neighbours' windows (label haloBase + haloOff decides the parity); the flags are
// raised by block 0 of the NEXT launch (tile_kernel_dist), when every store of this one has completed.
template <int PMODE, bool AR>
__global__ __launch_bounds__(RB) void k_dpcg_update_p(PcgState* __restrict__ st, int it, const double* __restrict__ scal,
                                                      const double* __restrict__ rD, const double* __restrict__ rA, double* __restrict__ pA,
                                                      int64_t n, double* __restrict__ hist, int histLen, double* __restrict__ psi,
                                                      const double* P1, const double* P3, const PeerAR ar, const FusedCtl F, int arOff, int haloOff,
                                                      const HaloSendDev H)
{
    __shared__ double red[RB / 64];
    __shared__ double g[2];
    const double* s0 = scal + 0; const double* s1 = scal + 1;
    if (AR && !st->done) {
        // block 0 sends first; then every block does the part of the pass that does not need the sums -- the psi term the
        // previous iteration owes (deferred psi update: it needs alpha, not beta) -- and only then waits for the ranks
        const unsigned long long label = *F.arBase + (unsigned long long)arOff;
        double v[2] = {0.0, 0.0};
        if (blockIdx.x == 0) {
            v[0] = sum_partials(P1, red);          // k_reduce_final2's arithmetic
            v[1] = sum_partials(P3, red);
            if (threadIdx.x < 64) peer_ar_send<2>(ar, label, v);
            if (threadIdx.x == 0) F.used[0] += 1u;
        }
        if (psi != nullptr && it > 0 && st->rItP1 == it && st->pApplyItP1 != it) {   // `owed`, as in pcg_update_p_body
            const double alpha = st->alpha;
            chunk_loop(n, [&](int64_t i) { const double2 p = ld2(pA, i); double2 x = ld2_stream(psi, i); x.x = fma(alpha, p.x, x.x); x.y = fma(alpha, p.y, x.y); st2_stream(psi, i, x); },
                       [&](int64_t i) { psi[i] = fma(alpha, pA[i], psi[i]); });
        }
        psi = nullptr;                                // added: the body below must not add it again
        peer_ar_gather<2>(ar, label, v, g);
        s0 = g; s1 = g + 1;
    }
    if (!pcg_update_p_body<PMODE, true>(st, it, s0, nullptr, rD, rA, pA, n, s1, hist, histLen, psi, red)) return; // every block decides alike
    if (H.nSend == 0) return;
    const int par = (int)((*F.haloBase + (unsigned long long)haloOff) & 1ull);
    __syncthreads();                             // this block's pA stores are visible to its own threads
    for (int q = H.packStart[blockIdx.x] + threadIdx.x; q < H.packStart[blockIdx.x + 1]; q += RB) {
        const int sidx = H.packSend[q];
        __hip_atomic_store(H.dstVals[sidx] + (long long)par * H.dstParStride[sidx] + H.packFace[q], pA[H.packCell[q]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct DistHead {
    HaloRecvDev R;
    HaloSendDev H;
    FusedCtl F;
    int32_t nInterior, nTiles, it, haloOff;
    PcgState* st;
};
// Amul over all tiles in one launch: interior tiles first (they do not wait), boundary tiles last; a boundary tile polls the
// flags of this exchange and stages its neighbour-rank values straight from the window.  Block 0 first raises the NEIGHBOURS'
// flags: the stores of the p-update before it are complete (kernel boundary).
template <int BS>
__global__ __launch_bounds__(BS, BS >= 512 ? 8 : 1) void tile_kernel_dist(TileArgs a, const DistHead D)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x;
    if (b == 0 && threadIdx.x == 0 && D.st->rItP1 >= D.it) D.st->pApplyItP1 = D.it;   // k_pcg_final's note: the p-update of this iteration has added the psi term it owed
    if (D.st->done) return;
    const unsigned long long e = *D.F.haloBase + (unsigned long long)D.haloOff;
    const int par = (int)(e & 1ull);
    if (b == 0) {
        for (int q = threadIdx.x; q < D.H.nSend; q += BS) __hip_atomic_store(D.H.dstFlag[q] + par, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (threadIdx.x == 0) D.F.used[1] += 1u;
    }
    const int nI = D.nInterior;
    if (b < nI) {
        const int per = nI >> 3;
        tile_body<OP_AMUL, false, false, BS, false, false, 0>(a, (b < (per << 3)) ? (b & 7) * per + (b >> 3) : b, smem);
    } else {
        const int bb = b - nI, per = (D.nTiles - nI) >> 3;
        const int p = nI + ((bb < (per << 3)) ? (bb & 7) * per + (bb >> 3) : bb);
        if (threadIdx.x < 64) halo_wait_flags(D.R, e, par, threadIdx.x, 64);
        __syncthreads();
        a.xExt = D.R.myVals + (size_t)par * D.R.parStride;
        tile_body<OP_AMUL, false, false, BS, false, false, 1>(a, p, smem);
    }
}

// residual update.  AR: wA.pA is folded from the tile partials and all-reduced here, in every block; otherwise scal[2] holds it.
template <int PMODE, bool AR>
__global__ __launch_bounds__(RB) void k_dpcg_update_psi_r(PcgState* __restrict__ st, int it, const double* __restrict__ scal,
                                                          const double* __restrict__ pA, const double* __restrict__ wA, const double* __restrict__ rD,
                                                          double* __restrict__ psi, double* __restrict__ rA, int64_t n,
                                                          double* __restrict__ P3, double* __restrict__ P1, int deferPsi,
                                                          const double* tilePartial, int nTiles, const PeerAR ar, const FusedCtl F, int arOff)
{
    __shared__ double red[RB / 64];
    __shared__ double lds[AR ? RG + RB / 64 : 1];
    __shared__ double g[1];
    if (st->done) return;
    const double* s2 = scal + 2;
    if (AR) {
        double v[1] = {0.0};
        const unsigned long long label = *F.arBase + (unsigned long long)arOff;
        if (blockIdx.x == 0) {
            v[0] = fold_final_block<RB>(tilePartial, nTiles, lds);
            if (threadIdx.x < 64) peer_ar_send<1>(ar, label, v);
            if (threadIdx.x == 0) F.used[0] += 1u;
        }
        peer_ar_gather<1>(ar, label, v, g);
        s2 = g;
    }
    (void)pcg_update_psi_r_body<PMODE, true>(st, it, s2, pA, wA, rD, psi, rA, n, P3, P1, deferPsi, red);
}

// one workgroup: fold a tile-partial array and all-reduce it / reduce two partial arrays and all-reduce both (the 5-launch form
// of the iteration, for ranks that SHARE a device: there only single workgroups may wait for another process)
__global__ __launch_bounds__(1024) void k_dpcg_ar_fold(const PcgState* __restrict__ st, const double* __restrict__ tilePartial, int nTiles, double* __restrict__ out, const PeerAR ar)
{
    __shared__ double lds[RG + RB / 64];
    if (st->done) return;
    const double tot = fold_final_block<1024>(tilePartial, nTiles, lds);
    if (threadIdx.x < 64) { double v[1] = {tot}; peer_ar_wave<1>(ar, v, 1); if (threadIdx.x == 0) *out = v[0]; }
}
__global__ __launch_bounds__(RB) void k_dpcg_ar_two(const PcgState* __restrict__ st, const double* __restrict__ P1, const double* __restrict__ P3, double* __restrict__ scal, const PeerAR ar)
{
    __shared__ double red[RB / 64];
    if (st->done) return;
    const double s1 = sum_partials(P1, red), s3 = sum_partials(P3, red);
    if (threadIdx.x < 64) { double v[2] = {s1, s3}; peer_ar_wave<2>(ar, v, 2); if (threadIdx.x == 0) { scal[0] = v[0]; scal[1] = v[1]; } }
}
// end of a batch (one workgroup): the all-reduce the next p-update would have done (AR), the convergence test of the last
// iteration (k_pcg_final<true>), and the label bases advanced by what the batch really exchanged
template <bool AR>
__global__ __launch_bounds__(RB) void k_dpcg_final(PcgState* __restrict__ st, int it, double* __restrict__ scal, const double* __restrict__ P1, const double* __restrict__ P3,
                                                   double* __restrict__ hist, int histLen, const PeerAR ar, const FusedCtl F, int arOff)
{
    __shared__ double red[RB / 64];
    __shared__ double g[2];
    if (threadIdx.x == 0 && st->rItP1 >= it) st->pApplyItP1 = it;
    unsigned int mine = 0u;
    if (!st->done) {
        if (AR) {
            double v[2];
            v[0] = sum_partials(P1, red); v[1] = sum_partials(P3, red);
            peer_ar_block<2>(ar, *F.arBase + (unsigned long long)arOff, v, g);   // one block: it sends and gathers
            mine = 1u;
            if (threadIdx.x == 0) { scal[0] = v[0]; scal[1] = v[1]; }
        }
        if (threadIdx.x == 0) {
            const double s = scal[1];
            if (s < 0.0) { st->singular = 1; st->done = 1; }
            else {
                const double res = s / st->normFactor;
                st->finalResidual = res;
                if (it + 1 < histLen) hist[it + 1] = res;
                st->nIterations = it + 1;
                st->it = it + 1;
                const bool conv = sp_converged(st, res);
                st->converged = conv;
                const bool cont = (it < st->maxIter && !conv) || (it + 1 < st->minIter);
                if (!cont) st->done = 1;
            }
        }
    }
    if (threadIdx.x == 0) {
        *F.arBase += (unsigned long long)(F.used[0] + mine);
        *F.haloBase += (unsigned long long)F.used[1];
        F.used[0] = 0u; F.used[1] = 0u;
    }
}

// globalize (engine.hip) / globalize_n (multi.inc) on a communicator in peer mode, as ONE single-workgroup launch: the final
// reductions of up to six RG-partial arrays (sum_partials' order: the bits k_reduce_final gives), one all-reduce of those sums
// through the windows, and the global sums spread back into the arrays as {sum, 0, 0, ...} for the consumers' own re-reduction.
// Round 3 issued three launches per sum point (k_reduce_final*, k_peer_allreduce, k_spread_partials): nine per PBiCG iteration.
struct GlobPtrs { double* p[6]; };
__global__ __launch_bounds__(RB) void k_globalize_ar(const GlobPtrs P, int n, const PeerAR ar)
{
    __shared__ double red[RB / 64];
    __shared__ double g[6];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) if (k < n) v[k] = sum_partials(P.p[k], red);
    if (threadIdx.x < 64) {
        peer_ar_wave<6>(ar, v, n);
        if (threadIdx.x == 0) for (int k = 0; k < n; ++k) g[k] = v[k];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        double* q = P.p[k];
        const double t = g[k];
        for (int i = threadIdx.x; i < RG; i += RB) q[i] = (i == 0) ? t : 0.0;
    }
}

__global__ void k_count_mismatch(const double* __restrict__ a, const double* __restrict__ b, int n, int* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) if (!(a[i] == b[i])) atomicAdd(out, 1);
}

} // namespace mi

// ---- host side ---------------------------------------------------------------------------------------------------------
struct PeerHalo {
    bool ready = false, fineGrained = false;
    void* window = nullptr;                       // [2][nExt] doubles, then [nPatches][2] flags
    Table<void*> mapped;                    // every rank's window as mapped here (own entry = window; nullptr = not a neighbour)
    DevBuf<double*> dstVals; DevBuf<long long> dstParStride; DevBuf<unsigned long long*> dstFlag, dstPair;
    DevBuf<int32_t> packStart, packCell, packSend, packFace, sendStart, faceCellE, recvPatch, recvOffset, recvSize, distTiles;
    DevBuf<int32_t> tileSendStart, sendLocal, tileBoundary;   // the same pack plan per TILE (persist.inc) ...
    DevBuf<double*> sendDst; int32_t nSendTot = 0;
    bool persistAgreed = false;                               // EVERY rank's sub-domain fits the persistent kernel (agreed at set-up)            // ... with the address of every value in the neighbour's window, [2 parities][nSendTot]
    DevBuf<double> recvFactor; Table<double> recvFactorHost;
    unsigned long long* epoch = nullptr;          // device
    unsigned int* tickets = nullptr;              // device: [0] ticket of k_halo_push (and of the push blocks of tile_kernel_win), [1] [2] all-reduces / halo exchanges counted by the fused iteration (FusedCtl::used), [4] tile_kernel_win's ticket of the blocks that read the epoch
    int32_t* status = nullptr;                    // device
    int32_t nSend = 0, nRecv = 0, nExt = 0, nPatches = 0;
    Table<int32_t> patchRank;
    int myRank = 0;
    ~PeerHalo()
    {
        for (size_t r = 0; r < mapped.size(); ++r) if (mapped[r] && (int)r != myRank) (void)hipIpcCloseMemHandle(mapped[r]);
        if (window) (void)hipFree(window);
        if (epoch) (void)hipFree(epoch);
        if (tickets) (void)hipFree(tickets);
        if (status) (void)hipFree(status);
    }
};

bool peer_halo_ready(const mi_matrix_s* m) { return m->dpc && m->dpc->ph && m->dpc->ph->ready; }
bool peer_reduce_ready(const mi_matrix_s* m) { return m->dpc && m->dpc->reduce && m->dpc->reduce->peerReady && sw::get(SW_PEER_GLOBALIZE) != 0; }
int peer_globalize(mi_matrix_s* m, int n, double* const* P)
{
    if (n < 1 || n > 6) return fail(MI_ERR_LIMIT, "peer_globalize: one to six sums");
    GlobPtrs q;
    for (int k = 0; k < 6; ++k) q.p[k] = P[k < n ? k : 0];
    k_globalize_ar<<<1, RB, 0, m->addr->ctx->stream>>>(q, n, peer_ar(m->dpc->reduce));
    HIPCHK(hipGetLastError());
    return MI_OK;
}
namespace {
bool persist_fits_layout(const mi_matrix_s* m);          // persist.inc
int32_t persist_tiles_per_wg(const mi_matrix_s* m);
HaloSendDev halo_send_dev(const PeerHalo* P, int ticket)
{
    return HaloSendDev{P->dstVals.p, P->dstPair.p, P->dstParStride.p, P->dstFlag.p, P->nSend, P->packStart.p, P->packCell.p, P->packSend.p, P->packFace.p,
                       P->sendStart.p, P->faceCellE.p, P->epoch, P->tickets + ticket};
}
HaloRecvDev halo_recv_dev(const PeerHalo* P, bool withFactors, long long maxPolls = PEER_POLLS)
{
    const double* vals = static_cast<const double*>(P->window) + halo_win_vals_off(P->nExt);
    const unsigned long long* flags = reinterpret_cast<const unsigned long long*>(vals + 2 * (size_t)HALO_NV * (size_t)P->nExt);
    return HaloRecvDev{vals, flags, P->recvPatch.p, P->recvOffset.p, P->recvSize.p, withFactors ? P->recvFactor.p : nullptr, P->nRecv, P->nExt, HALO_NV * P->nExt,
                       reinterpret_cast<const unsigned long long*>(P->window), P->epoch, P->status, maxPolls};
}


// the two halves of a peer exchange of engine vector x (n_cells + n_ext): stores into the neighbours' windows; wait + copy
// into x's ext region (factors of transformed patches applied there)
} // namespace
int peer_exchange_push_n(mi_matrix_s* m, int nv, const double* const* xs)
{
    PeerHalo* P = m->dpc->ph;
    if (P->nSend == 0) return MI_OK;
    if (nv < 1 || nv > HALO_NV) return fail(MI_ERR_LIMIT, "peer halo exchange: too many operands");
    HaloOperands X;
    memset(&X, 0, sizeof(X));
    X.n = nv;
    for (int v = 0; v < nv; ++v) X.x[v] = xs[v];
    const int blocks = std::max(1, std::min(64, (P->nExt * nv + 1023) / 1024));
    k_halo_push<<<blocks, 256, 0, m->addr->ctx->stream>>>(X, halo_send_dev(P, 0));
    HIPCHK(hipGetLastError());
    return MI_OK;
}
int peer_exchange_push(mi_matrix_s* m, const double* x) { return peer_exchange_push_n(m, 1, &x); }
int peer_exchange_pull_n(mi_matrix_s* m, int nv, double* const* xs);
int peer_exchange_pull(mi_matrix_s* m, double* x) { return peer_exchange_pull_n(m, 1, &x); }
// true when some received patch carries a transformCoupleField factor != 1 (the factors then sit in P->recvFactor)
int peer_recv_factors(mi_matrix_s* m, bool* any)
{
    PeerHalo* P = m->dpc->ph;
    *any = false;
    if (m->patchFactor.empty() || P->nRecv == 0) return MI_OK;
    Table<double> f((size_t)P->nRecv, 1.0);
    for (int r = 0; r < P->nRecv; ++r) { f[(size_t)r] = m->patchFactor[(size_t)m->dpc->recvs_patch[(size_t)r]]; if (f[(size_t)r] != 1.0) *any = true; }
    if (*any && f != P->recvFactorHost) { MICHK(P->recvFactor.upload(f, m->addr->ctx->stream)); P->recvFactorHost = f; }
    return MI_OK;
}
int peer_exchange_pull_n(mi_matrix_s* m, int nv, double* const* xs)
{
    const long long maxPolls = PEER_POLLS;
    PeerHalo* P = m->dpc->ph;
    if (P->nRecv == 0) return MI_OK;
    if (nv < 1 || nv > HALO_NV) return fail(MI_ERR_LIMIT, "peer halo exchange: too many operands");
    bool any = false;
    MICHK(peer_recv_factors(m, &any));
    HaloOperands X;
    memset(&X, 0, sizeof(X));
    X.n = nv;
    for (int v = 0; v < nv; ++v) X.ext[v] = xs[v] + m->addr->L.nCells;
    k_halo_pull<<<std::max(1, std::min(16, (P->nExt * nv + 2047) / 2048)), 256, 0, m->addr->ctx->stream>>>(X, halo_recv_dev(P, any, maxPolls));
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// may the boundary tiles read the window themselves?  Received values of a transformed (processorCyclic) patch are scaled on
// arrival and cyclicAMI values are interpolated into the operand's ext region: both keep the pull + second-launch form.
bool peer_win_direct(mi_matrix_s* m)
{
    mi_addr_s* a = m->addr;
    if (!a->ctx->winDirect || a->compact || !a->ami.empty() || m->callerY) return false;
    if (m->dpc->reduce->sharedDevice && a->ctx->winDirect < 2) return false;   // ranks sharing a device (tests): MI_WIN_DIRECT=2 forces it for small cases
    for (double f : m->patchFactor) if (f != 1.0) return false;
    return true;
}
namespace {
template <int OP, bool ASYM, bool TRANS>
int launch_tile_win_bs(mi_matrix_s* m, const TileArgs& t, const WinHead& W, size_t lds)
{
    mi_ctx_s* cx = m->addr->ctx;
    hipStream_t s = cx->stream;
    int bs = cx->amulBS;
    if (bs == 0) bs = (lds > 53 * 1024) ? 1024 : (m->addr->L.maxCells <= 256 ? 256 : 512);
    if (W.nTiles <= 0) return MI_OK;
    const int grid = W.nTiles + W.nPush;
#define MI_LAUNCH_WIN(BS)                                                                                               \
    {                                                                                                                   \
        const void* fn = (const void*)tile_kernel_win<OP, ASYM, TRANS, BS>;                                             \
        if (!cx->ldsAttrSet.count(fn)) { HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024)); cx->ldsAttrSet.insert(fn); } \
        if (m->kevStart) hipExtLaunchKernelGGL((tile_kernel_win<OP, ASYM, TRANS, BS>), dim3(grid), dim3(BS), (uint32_t)lds, s, m->kevStart, m->kevStop, 0, t, W); \
        else tile_kernel_win<OP, ASYM, TRANS, BS><<<grid, BS, lds, s>>>(t, W);                                          \
    }
    if (bs == 1024) MI_LAUNCH_WIN(1024) else if (bs == 512) MI_LAUNCH_WIN(512) else MI_LAUNCH_WIN(256)
#undef MI_LAUNCH_WIN
    HIPCHK(hipGetLastError());
    return MI_OK;
}
template <int OP>
int launch_tile_win(mi_matrix_s* m, bool trans, const double* x, const double* b, const double* rD, double* y,
                    double omega, double* dotPartial, double* dotPartial2)
{
    if constexpr (OP == OP_AMUL || OP == OP_RESIDUAL || OP == OP_H || OP == OP_JACOBI || OP == OP_PROLOGUE) {
        mi_addr_s* a = m->addr;
        PeerHalo* P = m->dpc->ph;
        if (!m->bound) return fail(MI_ERR_STATE, "matrix coefficients not bound (mi_matrix_set_coeffs)");
        TileArgs t;
        t.tileCellStart = a->tileCellStart.p; t.tileSlotStart = a->tileSlotStart.p; t.tileIfaceSlot0 = a->tileIfaceSlot0.p; t.tileHaloStart = a->tileHaloStart.p;
        t.haloCell = a->haloCell.p; t.tileSliceStart = a->tileSliceStart.p; t.sliceEntryStart = a->sliceEntryStart.p;
        t.entries = a->entries.p; t.entries16 = nullptr; t.sliceEntryStart16 = nullptr; t.slotBase = nullptr; t.tileSbStart = nullptr;
        t.diag = m->diagE.p; t.up = m->upE.p; t.low = m->lowE.p;
        t.x = x; t.b = b; t.rD = rD; t.y = y; t.omega = omega; t.dotPartial = dotPartial; t.dotPartial2 = dotPartial2; t.flags = a->ctx->tileFlags;
        if (OP == OP_PROLOGUE) { t.y2 = m->proY2; t.y3 = m->proY3; }
        t.tileList = P->distTiles.p; t.nPos = a->L.nTiles; t.nCells = a->L.nCells;
        t.done = m->gateDone ? &a->ctx->state.p->done : nullptr;
        const size_t lds = lds_bytes(a->L, m->asym, false, &t.offLow, &t.offX, &t.offRD, &t.offSB);
        if (lds > 159 * 1024) return fail(MI_ERR_LIMIT, "tile needs more than 159 KiB of LDS");
        WinHead W;
        W.R = halo_recv_dev(P, false); W.H = halo_send_dev(P, 0); W.nInterior = a->nInterior; W.nTiles = a->L.nTiles;
        W.nPush = std::max(1, std::min(32, (P->nExt + 2047) / 2048)); W.allTicket = P->tickets + 4;
        if (m->asym) {
            if (trans) return launch_tile_win_bs<OP, true, true>(m, t, W, lds);
            return launch_tile_win_bs<OP, true, false>(m, t, W, lds);
        }
        return launch_tile_win_bs<OP, false, false>(m, t, W, lds);
    } else {
        (void)m; (void)trans; (void)x; (void)b; (void)rD; (void)y; (void)omega; (void)dotPartial; (void)dotPartial2;
        return fail(MI_ERR_STATE, "window form of an operator that reads no neighbour values");
    }
}
} // namespace

// Set the halo windows of an attached matrix up (collective: every rank of the communicator calls it for its matching matrix,
// in the same order): allocate + all-gather the handles over the communicator's base transport + map the neighbours + two
// set-up exchanges (where does the neighbour want my patch: its patch offset and its n_ext) + a self-test against the base
// exchange.  *enabled_out = 0 (and nothing changes) when any rank could not.
extern "C" int mi_matrix_peer_halo_auto(mi_matrix_t m, int32_t* enabled_out)
{
    if (!m || !enabled_out) return fail(MI_ERR_ARG, "mi_matrix_peer_halo_auto: bad argument");
    *enabled_out = 0;
    if (!comm_attached(m)) return fail(MI_ERR_STATE, "mi_matrix_peer_halo_auto: attach the communicators first (mi_matrix_attach_comm)");
    mi_dpcg_comm_s& D = *m->dpc;
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    mi_comm_s* base = D.halo;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const TileLayout& L = a->L;
    delete D.ph; D.ph = nullptr;
    PeerHalo* P = new PeerHalo();
    struct Guard { PeerHalo*& p; bool keep = false; ~Guard() { if (!keep) { delete p; p = nullptr; } } } guard{P};
    P->nExt = L.nExt; P->nPatches = L.nPatches; P->myRank = base->rank;
    bool ok = base->nRanks <= 4096, all = false;
    unsigned char mine[sizeof(hipIpcMemHandle_t)] = {0};
    const size_t bytes = sizeof(double) * (halo_win_vals_off(L.nExt) + 2 * (size_t)HALO_NV * (size_t)std::max(L.nExt, 1)) + sizeof(unsigned long long) * 2 * (size_t)std::max(L.nPatches, 1);
    if (ok) {
        ok = alloc_ipc_window(bytes, &P->window, &P->fineGrained) == MI_OK;
        hipIpcMemHandle_t h;
        if (ok) ok = hipIpcGetMemHandle(&h, P->window) == hipSuccess;
        if (ok) memcpy(mine, &h, sizeof(h));
        if (ok) ok = hipMalloc(reinterpret_cast<void**>(&P->epoch), sizeof(unsigned long long)) == hipSuccess && hipMemset(P->epoch, 0, sizeof(unsigned long long)) == hipSuccess &&
                     hipMalloc(reinterpret_cast<void**>(&P->tickets), 8 * sizeof(unsigned int)) == hipSuccess && hipMemset(P->tickets, 0, 8 * sizeof(unsigned int)) == hipSuccess &&
                     hipMalloc(reinterpret_cast<void**>(&P->status), sizeof(int32_t)) == hipSuccess && hipMemset(P->status, 0, sizeof(int32_t)) == hipSuccess;
        (void)hipGetLastError();
    }
    MICHK(comm_agree(base, ok, &all));
    if (!all) return MI_OK;
    Table<unsigned char> handles;
    MICHK(comm_gather_bytes(base, mine, sizeof(mine), handles));
    // map the neighbours (a rank that is its own neighbour uses its own window)
    P->mapped.assign((size_t)base->nRanks, nullptr);
    bool oneDevice = true;
    for (const auto& e : D.sends) {
        if (P->mapped[(size_t)e.peer]) continue;
        if (e.peer == base->rank) { P->mapped[(size_t)e.peer] = P->window; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, handles.data() + (size_t)e.peer * sizeof(h), sizeof(h));
        void* q = nullptr;
        if (hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
        P->mapped[(size_t)e.peer] = q;
        if (!on_my_device(c, q)) oneDevice = false;
    }
    if (ok && !P->fineGrained && !oneDevice && !sw::get(SW_PEER_ALLOW_COARSE)) ok = false;
    // From here to the end every LOCAL failure (an allocation, a copy) is folded into `ok` and the rank carries on to the next
    // agreement: the function is called collectively from mi_matrix_attach_comm, and a rank that returned early would leave
    // the others blocked in their next all-reduce (ADVICE r03).  Collective calls are issued by every rank regardless.
    double *v0 = nullptr, *v1 = nullptr;
    if (ok && (m->vec(WV_OP_X, &v0) != MI_OK || m->vec(WV_OP_Y, &v1) != MI_OK)) ok = false;
    if (ok && m->sendBuf.n < (size_t)std::max(L.nExt, 1) && m->sendBuf.alloc((size_t)std::max(L.nExt, 1)) != MI_OK) ok = false;
    MICHK(comm_agree(base, ok, &all));      // also: every window is mapped before anyone writes into it
    if (!all) return MI_OK;
    // where the neighbour wants my patch p: its offset of the matching patch and its n_ext, through two ordinary exchanges
    Table<double> hs((size_t)std::max(L.nExt, 1), 0.0), hr((size_t)std::max(L.nExt, 1), 0.0);
    Table<long long> nbrOffset((size_t)L.nPatches, 0), nbrNExt((size_t)L.nPatches, 0);
    for (int pass = 0; pass < 2 && L.nExt > 0; ++pass) {
        for (int32_t p = 0; p < L.nPatches; ++p)
            for (int32_t i = L.patchOffset[p]; i < L.patchOffset[(size_t)p + 1]; ++i) hs[(size_t)i] = pass == 0 ? (double)L.patchOffset[p] : (double)L.nExt;
        if (hipMemcpyAsync(m->sendBuf.p, hs.data(), sizeof(double) * (size_t)L.nExt, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
        if (comm_p2p_raw(base, s, D.sends, D.recvs, m->sendBuf.p, v0 + L.nCells) != MI_OK) ok = false;
        if (hipMemcpyAsync(hr.data(), v0 + L.nCells, sizeof(double) * (size_t)L.nExt, hipMemcpyDeviceToHost, s) != hipSuccess) ok = false;
        if (hipStreamSynchronize(s) != hipSuccess) ok = false;
        (void)hipGetLastError();
        for (const auto& e : D.sends) (pass == 0 ? nbrOffset : nbrNExt)[(size_t)e.patch] = (long long)(hr[(size_t)e.offset] + 0.5);
    }
    // send side tables
    P->nSend = (int32_t)D.sends.size(); P->nRecv = (int32_t)D.recvs.size();
    Table<double*> dv; Table<long long> ds; Table<unsigned long long*> df, dp;
    Table<int32_t> sendStart(1, 0), faceCellE, recvPatch, recvOffset, recvSize;
    Table<int32_t> sendOfPatch((size_t)L.nPatches, -1);
    for (size_t q = 0; q < D.sends.size(); ++q) {
        const auto& e = D.sends[q];
        const long long nx = nbrNExt[(size_t)e.patch];
        double* vals = static_cast<double*>(P->mapped[(size_t)e.peer]) + halo_win_vals_off(nx);
        dp.push_back(reinterpret_cast<unsigned long long*>(P->mapped[(size_t)e.peer]) + 2 * nbrOffset[(size_t)e.patch]);
        dv.push_back(vals + nbrOffset[(size_t)e.patch]);
        ds.push_back((long long)HALO_NV * nx);
        df.push_back(reinterpret_cast<unsigned long long*>(vals + 2 * (long long)HALO_NV * nx) + 2 * (size_t)e.nbrPatch);
        for (int32_t i = 0; i < e.size; ++i) faceCellE.push_back(L.patchFaceCellsE[(size_t)e.offset + (size_t)i]);
        sendStart.push_back((int32_t)faceCellE.size());
        sendOfPatch[(size_t)e.patch] = (int32_t)q;
    }
    D.recvs_patch.clear();
    for (const auto& e : D.recvs) { recvPatch.push_back(e.patch); recvOffset.push_back(e.offset); recvSize.push_back(e.size); D.recvs_patch.push_back(e.patch); }
    // pack plan of the fused p-update: patch faces sorted by the block (of the RG-block vector passes) that owns their cell
    int64_t chunk = ((int64_t)L.nCells + RG - 1) / RG;
    chunk = (chunk + 1) & ~int64_t(1);
    if (chunk < 2) chunk = 2;
    Table<Table<int32_t>> byBlock((size_t)RG);
    Table<int32_t> faceSend, faceIdx, faceCell;
    for (size_t q = 0; q < D.sends.size(); ++q)
        for (int32_t i = 0; i < D.sends[q].size; ++i) {
            const int32_t cell = L.patchFaceCellsE[(size_t)D.sends[q].offset + (size_t)i];
            byBlock[(size_t)std::min<int64_t>(cell / chunk, RG - 1)].push_back((int32_t)faceSend.size());
            faceSend.push_back((int32_t)q); faceIdx.push_back(i); faceCell.push_back(cell);
        }
    Table<int32_t> packStart(1, 0), packCell, packSend, packFace;
    for (int b = 0; b < RG; ++b) {
        for (int32_t k : byBlock[(size_t)b]) { packCell.push_back(faceCell[(size_t)k]); packSend.push_back(faceSend[(size_t)k]); packFace.push_back(faceIdx[(size_t)k]); }
        packStart.push_back((int32_t)packCell.size());
    }
    // ... and sorted by tile, with the cell's index inside its tile (the persistent kernel keeps pA in registers, persist.inc)
    Table<Table<int32_t>> byTile((size_t)L.nTiles);
    for (size_t k = 0; k < faceCell.size(); ++k) {
        const int32_t tile = (int32_t)(std::upper_bound(L.tileCellStart.begin(), L.tileCellStart.end(), faceCell[k]) - L.tileCellStart.begin()) - 1;
        byTile[(size_t)tile].push_back((int32_t)k);
    }
    Table<int32_t> tileSendStart(1, 0), sendLocal, tileBoundary((size_t)L.nTiles, 0);
    const int32_t tilesPerWG = persist_tiles_per_wg(m);
    Table<double*> sendDst0, sendDst1;
    for (int32_t t = 0; t < L.nTiles; ++t) {
        for (int32_t k : byTile[(size_t)t]) {
            const size_t q = (size_t)faceSend[(size_t)k];
            sendLocal.push_back((t % tilesPerWG) * 1024 + (faceCell[(size_t)k] - L.tileCellStart[(size_t)t]));   // row of the cell in its workgroup's [tile][1024] staging
            sendDst0.push_back(dv[q] + faceIdx[(size_t)k]);
            sendDst1.push_back(dv[q] + ds[q] + faceIdx[(size_t)k]);
        }
        tileSendStart.push_back((int32_t)sendLocal.size());
    }
    P->nSendTot = (int32_t)sendLocal.size();
    Table<double*> sendDst(sendDst0);
    sendDst.insert(sendDst.end(), sendDst1.begin(), sendDst1.end());
    if (sendDst.empty()) sendDst.push_back(nullptr);
    for (int32_t t : L.boundaryTiles) tileBoundary[(size_t)t] = 1;
    Table<int32_t> distTiles(L.interiorTiles);
    distTiles.insert(distTiles.end(), L.boundaryTiles.begin(), L.boundaryTiles.end());
    auto nonEmpty = [](Table<int32_t>& v) { if (v.empty()) v.push_back(0); };
    nonEmpty(sendLocal); nonEmpty(tileBoundary);
    nonEmpty(packCell); nonEmpty(packSend); nonEmpty(packFace); nonEmpty(faceCellE); nonEmpty(recvPatch); nonEmpty(recvOffset); nonEmpty(recvSize); nonEmpty(distTiles);
    if (dv.empty()) { dv.push_back(nullptr); ds.push_back(0); df.push_back(nullptr); dp.push_back(nullptr); }
    auto up = [&](int rc) { if (rc != MI_OK) ok = false; };
    up(P->dstVals.upload(dv, s)); up(P->dstParStride.upload(ds, s)); up(P->dstFlag.upload(df, s)); up(P->dstPair.upload(dp, s));
    up(P->packStart.upload(packStart, s)); up(P->packCell.upload(packCell, s)); up(P->packSend.upload(packSend, s)); up(P->packFace.upload(packFace, s));
    up(P->sendStart.upload(sendStart, s)); up(P->faceCellE.upload(faceCellE, s));
    up(P->recvPatch.upload(recvPatch, s)); up(P->recvOffset.upload(recvOffset, s)); up(P->recvSize.upload(recvSize, s));
    up(P->distTiles.upload(distTiles, s));
    up(P->tileSendStart.upload(tileSendStart, s)); up(P->sendLocal.upload(sendLocal, s)); up(P->sendDst.upload(sendDst, s));
    up(P->tileBoundary.upload(tileBoundary, s));
    up(P->recvFactor.alloc((size_t)std::max(P->nRecv, 1)));
    if (hipStreamSynchronize(s) != hipSuccess) ok = false;
    D.ph = P; guard.keep = true;   // (owned by the matrix from here on; `ready` only after the agreed self-test)
    // self-test: three exchanges of known vectors through the windows against the base exchange (a rank whose set-up failed
    // still takes part in the base exchanges; its neighbours' window waits run out -- bounded -- and everybody falls back)
    if (L.nExt > 0) {
        DevBuf<int32_t> bad;
        up(bad.upload(Table<int32_t>(1, 0), s));
        for (int round = 0; round < 3; ++round) {
            const double* x = round == 0 ? m->diagE.p : (round == 1 ? v0 : m->diagE.p);
            if (round == 1 && hipMemcpyAsync(v0, m->diagE.p, sizeof(double) * (size_t)L.nCells, hipMemcpyDeviceToDevice, s) != hipSuccess) ok = false;
            k_halo_pack<<<(L.nExt + 255) / 256, 256, 0, s>>>(x, a->patchFaceCellsE.p, m->sendBuf.p, L.nExt);
            if (comm_p2p_raw(base, s, D.sends, D.recvs, m->sendBuf.p, v1 + L.nCells) != MI_OK) ok = false;
            if (!ok) { (void)hipStreamSynchronize(s); (void)hipGetLastError(); continue; }
            if (hipMemsetAsync(v0 + L.nCells, 0, sizeof(double) * (size_t)L.nExt, s) != hipSuccess) ok = false;
            HaloOperands X;
            memset(&X, 0, sizeof(X));
            X.n = 1; X.x[0] = x; X.ext[0] = v0 + L.nCells;
            k_halo_push<<<std::max(1, std::min(64, (L.nExt + 1023) / 1024)), 256, 0, s>>>(X, halo_send_dev(P, 0));
            k_halo_pull<<<std::max(1, std::min(16, (L.nExt + 2047) / 2048)), 256, 0, s>>>(X, halo_recv_dev(P, false, 4000000ll));
            k_count_mismatch<<<64, 256, 0, s>>>(v0 + L.nCells, v1 + L.nCells, L.nExt, bad.p);
            int32_t nb = 1, st = 1;
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nb, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&st, P->status, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) ok = false;
            if (nb != 0 || st != 0) ok = false;
        }
        if (!ok) (void)hipMemset(P->status, 0, sizeof(int32_t));
    }
    MICHK(comm_agree(base, ok, &all));
    if (!all) { delete D.ph; D.ph = nullptr; return MI_OK; }
    // the persistent kernel (persist.inc) only when EVERY rank's sub-domain fits it and no two ranks share a device
    {
        const bool fits = persist_fits_layout(m) && (!D.reduce->sharedDevice || c->persistShared) && D.reduce->nRanks <= 64 && P->nSend <= 1024 && P->nRecv <= 1024;
        bool allFit = false;
        MICHK(comm_agree(base, fits, &allFit));
        P->persistAgreed = allFit;
    }
    P->patchRank.clear();
    for (const auto& e : D.sends) P->patchRank.push_back(e.peer);
    P->ready = true;
    *enabled_out = 1;
    return MI_OK;
}

extern "C" int mi_matrix_peer_halo_status(mi_matrix_t m, int32_t* enabled_out, int32_t* status_out)
{
    if (!m || !enabled_out) return fail(MI_ERR_ARG, "mi_matrix_peer_halo_status: bad argument");
    *enabled_out = peer_halo_ready(m) ? 1 : 0;
    if (status_out) {
        *status_out = 0;
        if (peer_halo_ready(m)) {
            HIPCHK(hipSetDevice(m->addr->ctx->device));
            HIPCHK(hipStreamSynchronize(m->addr->ctx->stream));
            HIPCHK(hipMemcpy(status_out, m->dpc->ph->status, sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    }
    return MI_OK;
}

// after a host synchronisation of a solver loop on an attached matrix: did a window wait run out of polls?  (the sums and
// halo values after that are garbage: ADVICE r02 -- the loops used to carry on)
int peer_check(mi_matrix_s* m)
{
    if (!m->dpc) return MI_OK;
    int32_t st = 0;
    if (m->dpc->reduce && m->dpc->reduce->peerReady && m->dpc->reduce->peerStatus) {
        HIPCHK(hipMemcpy(&st, m->dpc->reduce->peerStatus, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (st != 0) return fail(MI_ERR_DEVICE, "peer all-reduce: a rank never arrived (window wait ran out of polls); the results of this solve are not valid");
    }
    if (m->dpc->ph && m->dpc->ph->ready) {
        HIPCHK(hipMemcpy(&st, m->dpc->ph->status, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (st != 0) return fail(MI_ERR_DEVICE, "peer halo exchange: a neighbour never arrived (window wait ran out of polls); the results of this solve are not valid");
    }
    return MI_OK;
}

namespace {
bool dpcg_persist_usable(const mi_matrix_s* m);          // persist.inc: the whole batch as ONE persistent cooperative kernel
int dpcg_persist_enqueue(mi_matrix_s* m, int n_iters);
// the fused iteration: three launches, no collective call
bool dpcg_fused_usable(const mi_matrix_s* m)
{
    return peer_halo_ready(m) && m->dpc->reduce->peerReady && !m->asym && !comm_any_compact(m) && sw::get(SW_DPCG_FUSED) != 0;
}
int dpcg_fused_iterate(mi_matrix_s* m, int32_t n_iters, int32_t record_amul_events)
{
    mi_dpcg_comm_s& D = *m->dpc;
    const mi_dpcg_s& B = m->dp;
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    hipStream_t s = c->stream;
    PeerHalo* P = D.ph;
    const int64_t n = a->L.nCells;
    if (n_iters <= 0) return MI_OK;
    if (record_amul_events <= 0 && dpcg_persist_usable(m)) {   // a sub-domain small enough for the CUs' registers (persist.inc)
        MICHK(dpcg_persist_enqueue(m, n_iters));
        D.it += n_iters;
        return MI_OK;
    }
    double* P3 = c->partial.p + RG; double* P1 = c->partial.p + 2 * RG;
    TileArgs t;
    t.tileCellStart = a->tileCellStart.p; t.tileSlotStart = a->tileSlotStart.p; t.tileIfaceSlot0 = a->tileIfaceSlot0.p; t.tileHaloStart = a->tileHaloStart.p;
    t.haloCell = a->haloCell.p; t.tileSliceStart = a->tileSliceStart.p; t.sliceEntryStart = a->sliceEntryStart.p;
    t.entries = a->entries.p; t.entries16 = nullptr; t.sliceEntryStart16 = nullptr; t.slotBase = nullptr; t.tileSbStart = nullptr;
    t.diag = m->diagE.p; t.up = m->upE.p; t.low = nullptr;
    t.x = B.pA; t.b = nullptr; t.rD = nullptr; t.y = B.wA; t.omega = 0.0; t.dotPartial = m->tilePartial.p; t.dotPartial2 = nullptr; t.flags = c->tileFlags;
    t.tileList = P->distTiles.p; t.nPos = a->L.nTiles; t.done = nullptr; t.nCells = a->L.nCells;
    const size_t lds = lds_bytes(a->L, false, false, &t.offLow, &t.offX, &t.offRD, &t.offSB);
    if (lds > 159 * 1024) return fail(MI_ERR_LIMIT, "tile needs more than 159 KiB of LDS");
    int bs = c->amulBS;
    if (bs == 0) bs = (lds > 53 * 1024) ? 1024 : (a->L.maxCells <= 256 ? 256 : 512);
    // ranks that SHARE a device (tests, rehearsals): only single workgroups may wait for another process there -- a launch whose
    // every block polls could fill the device while the process it waits for cannot get a workgroup in; five launches then
    // How the two sums of an iteration meet the other ranks (measured at 108^3 per rank, profiles/r03_a_selfcomm_108.json):
    //   5 (default)  two one-workgroup kernels (fold / reduce + all-reduce through the windows, ~3.7 us each): 50.7 us per iteration
    //   4            the two-scalar one inside the p-update instead -- block 0 sends, every block adds the psi term it owes
    //                meanwhile and then gathers -- : 56.0 us (a gather in a thousand blocks costs more than a launch)
    //   3            both inside the passes: 62.2 us
    // (the phase loop over RCCL: 80.6 us.)  Ranks that share a device always take 5: there only single workgroups may wait
    // for another process.
    const int want = sw::get(SW_DPCG_FUSED);
    const int mode = (D.reduce->sharedDevice || (want != 3 && want != 4)) ? 5 : want;
    const PeerAR ar = peer_ar(D.reduce);
    const FusedCtl F{D.reduce->fusedEpoch, P->epoch, P->tickets + 1};
    DistHead T;
    T.R = halo_recv_dev(P, false); T.H = halo_send_dev(P, 0); T.F = F; T.nInterior = a->nInterior; T.nTiles = a->L.nTiles; T.st = c->state.p;
    const bool diag = B.precond == MI_PRECOND_DIAGONAL;
    const int defer = c->deferPsi ? 1 : 0;
    double* psiD = defer ? B.psi : nullptr;
    const double* rD = diag ? m->rD.p : nullptr;
    int lab = 0;   // in-kernel all-reduces issued so far in this batch: the next one carries the label fusedEpoch + lab + 1
    for (int32_t k = 0; k < n_iters; ++k) {
        const int32_t it = D.it;
        const bool arP = k > 0 && mode != 5;
        if (arP) ++lab;
#define MI_K1(PM, AR) k_dpcg_update_p<PM, AR><<<RG, RB, 0, s>>>(c->state.p, it, B.scal, rD, B.rA, B.pA, n, m->hist.p, m->histLen, psiD, P1, P3, ar, F, lab, k + 1, T.H)
        if (diag) { if (arP) MI_K1(1, true); else MI_K1(1, false); }
        else { if (arP) MI_K1(2, true); else MI_K1(2, false); }
#undef MI_K1
        T.it = it; T.haloOff = k + 1;
        const bool rec = record_amul_events > 0 && (k % record_amul_events) == 0;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (rec) {
            const size_t ev = (size_t)2 * (size_t)(k / record_amul_events);
            while (m->evPool.size() < ev + 2) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); m->evPool.push_back(e); }
            e0 = m->evPool[ev]; e1 = m->evPool[ev + 1];
        }
#define MI_LAUNCH_DIST(BS)                                                                                              \
        {                                                                                                               \
            const void* fn = (const void*)tile_kernel_dist<BS>;                                                         \
            if (!c->ldsAttrSet.count(fn)) { HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024)); c->ldsAttrSet.insert(fn); } \
            if (rec) hipExtLaunchKernelGGL((tile_kernel_dist<BS>), dim3(a->L.nTiles), dim3(BS), (uint32_t)lds, s, e0, e1, 0, t, T); \
            else tile_kernel_dist<BS><<<a->L.nTiles, BS, lds, s>>>(t, T);                                               \
        }
        if (bs == 1024) MI_LAUNCH_DIST(1024) else if (bs == 512) MI_LAUNCH_DIST(512) else MI_LAUNCH_DIST(256)
#undef MI_LAUNCH_DIST
        const bool arR = mode == 3;
        if (!arR) k_dpcg_ar_fold<<<1, 1024, 0, s>>>(c->state.p, m->tilePartial.p, a->L.nTiles, B.scal + 2, ar);
        else ++lab;
#define MI_K3(PM, AR) k_dpcg_update_psi_r<PM, AR><<<RG, RB, 0, s>>>(c->state.p, it, B.scal, B.pA, B.wA, rD, B.psi, B.rA, n, P3, P1, defer, m->tilePartial.p, a->L.nTiles, ar, F, lab)
        if (diag) { if (arR) MI_K3(1, true); else MI_K3(1, false); }
        else { if (arR) MI_K3(2, true); else MI_K3(2, false); }
#undef MI_K3
        if (mode == 5) k_dpcg_ar_two<<<1, RB, 0, s>>>(c->state.p, P1, P3, B.scal, ar);
        D.it++;
    }
    if (mode == 5) k_dpcg_final<false><<<1, RB, 0, s>>>(c->state.p, D.it - 1, B.scal, P1, P3, m->hist.p, m->histLen, ar, F, 0);
    else k_dpcg_final<true><<<1, RB, 0, s>>>(c->state.p, D.it - 1, B.scal, P1, P3, m->hist.p, m->histLen, ar, F, lab + 1);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// end of a batch / of the solve: the psi term the last iteration still owes (deferred psi update of the fused loop)
int dpcg_fused_flush(mi_matrix_s* m)
{
    mi_ctx_s* c = m->addr->ctx;
    if (!c->deferPsi || !m->dp.psi) return MI_OK;
    k_pcg_flush_psi<<<RG, RB, 0, c->stream>>>(c->state.p, m->dp.pA, m->dp.psi, m->addr->L.nCells);
    k_pcg_flush_mark<<<1, 1, 0, c->stream>>>(c->state.p);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
} // namespace
int dpcg_flush_if_fused(mi_matrix_s* m) { return (m->dpc && dpcg_fused_usable(m)) ? dpcg_fused_flush(m) : MI_OK; }
