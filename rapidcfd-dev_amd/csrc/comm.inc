// comm.inc -- RCCL communicator + the host loop of the distributed PCG, in C++.
//
// The reference meets its neighbours through MPI: Foam::reduce (PCG.C:142,166,195 ->
// src/Pstream/mpi/allReduceTemplates.C:195-208) and the processor-patch exchange inside
// Amul (lduMatrixUpdateMatrixInterfaces.C:30-276, processorFvPatchScalarField.C:36-170,
// host-staged MPI_Isend/Irecv).  Here one rank drives one MI355X; the collectives are
// RCCL calls (xGMI) enqueued by this file on the engine's stream (all-reduces) and on a
// second stream (halo send/recv), so the interior tiles of Amul run while the halo is in
// flight and the host never waits inside the iteration loop.
//
// RCCL is bound at run time (dlopen) so that the library also loads on machines without
// it (the ABI / host tests); a missing RCCL is an error at mi_comm_* time, never a fallback.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <fstream>

namespace {
struct RcclApi {
    void* h = nullptr;
    bool tried = false;
    std::string err;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;

    bool load()
    {
        if (tried) return h != nullptr;
        tried = true;
        // prefer the copy the process already holds (PyTorch ships its own librccl.so)
        std::string path;
        {
            std::ifstream maps("/proc/self/maps");
            std::string line;
            while (std::getline(maps, line)) {
                const size_t k = line.find("librccl.so");
                if (k == std::string::npos) continue;
                const size_t b = line.find('/');
                if (b != std::string::npos) { path = line.substr(b); break; }
            }
        }
        if (!path.empty()) h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
#define SYM(name) name = reinterpret_cast<decltype(name)>(dlsym(h, "nccl" #name)); if (!name) { err = "librccl lacks nccl" #name; h = nullptr; return false; }
        SYM(GetUniqueId) SYM(CommInitRank) SYM(CommDestroy) SYM(AllReduce) SYM(Send) SYM(Recv) SYM(GroupStart) SYM(GroupEnd) SYM(GetErrorString)
#undef SYM
        return true;
    }
};
RcclApi& rccl() { static RcclApi r; return r; }
} // namespace

#define NCCLCHK(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) return fail(MI_ERR_DEVICE, std::string("rccl: ") + rccl().GetErrorString(r_) + " at " #expr); } while (0)

struct mi_comm_s {
    mi_ctx_s* ctx = nullptr;
    ncclComm_t comm = nullptr;
    int nRanks = 0, rank = 0;
    // external transport (mi_comm_create_external): the caller's own message passing -- the reference's is MPI through
    // Pstream (UPstream.C:185-262, processorLduInterfaceTemplates.C:127-298) -- instead of RCCL.  Blocking by contract:
    // the engine synchronises the producing stream, the callback returns once the data is in place in device memory.
    mi_comm_allreduce_fn extAllreduce = nullptr;
    mi_comm_exchange_fn extExchange = nullptr;
    void* extUser = nullptr;
    bool external() const { return extAllreduce != nullptr; }
    // one-shot peer all-reduce (SURVEY.md 8e "one-shot P2P all-to-all on the fully connected node"; opt-in, see peer_allreduce)
    double* window = nullptr;               // this rank's window: [2 parities][nRanks slots][PEER_SLOT doubles]
    Table<double*> peerWindow;        // every rank's window as mapped here (own entry = window)
    unsigned long long* epoch = nullptr;    // device counter of the all-reduces done through the windows
    unsigned long long* fusedEpoch = nullptr; // the same for the all-reduces the fused solver passes perform (replicated part of the windows, peer.inc)
    int32_t* peerStatus = nullptr;          // device flag: a wait ran out of polls
    double** peerTable = nullptr;           // device copy of peerWindow (what the kernel reads)
    bool windowFineGrained = false;
    bool peerReady = false;
    bool sharedDevice = false;              // a peer's window lives on THIS device (ranks sharing a GPU: tests, rehearsals)
    ~mi_comm_s();
};
constexpr int PEER_MAX = 8;                 // doubles per all-reduce through the windows (the Krylov loops send 1-3)
constexpr int PEER_SLOT = PEER_MAX + 1;     // + the epoch flag
// second part of a window, for the all-reduces that EVERY block of a fused solver pass performs (peer.inc, peer_ar_block): the
// sender writes PEER_REP copies of its (<= 3) values + label, block b of the reading launch polls copy b % PEER_REP -- a
// thousand blocks polling ONE uncached line cost ~15 us per all-reduce (measured, profiles/r03_a), spread over 64 lines in
// different memory channels they cost what one poller costs
constexpr int PEER_REP = 64;
constexpr int PEER_FSLOT = 4;               // 3 values + label
inline size_t peer_rep_stride(int nRanks) { return (size_t)std::max(32, nRanks * PEER_FSLOT); }   // doubles between two copies (>= 256 B)
inline size_t peer_fused_off(int nRanks) { return (size_t)2 * (size_t)nRanks * PEER_SLOT; }
inline size_t peer_window_doubles(int nRanks) { return peer_fused_off(nRanks) + (size_t)2 * PEER_REP * peer_rep_stride(nRanks); }

namespace {
int ext_allreduce(mi_comm_s* c, hipStream_t stream, double* p, size_t n)
{
    HIPCHK(hipStreamSynchronize(stream));
    if (c->extAllreduce(c->extUser, p, (int64_t)n) != 0) return fail(MI_ERR_DEVICE, "external communicator: all-reduce callback failed");
    return MI_OK;
}
// sends are tagged with the sender's patch index, receives with the neighbour's patch index: the same number on both ends
template <class P2P>
int ext_exchange(mi_comm_s* c, hipStream_t stream, const Table<P2P>& sends, const Table<P2P>& recvs, const double* send, double* recv)
{
    HIPCHK(hipStreamSynchronize(stream));
    Table<int32_t> sp, st, rp, rt; Table<const double*> sb; Table<double*> rb; Table<int64_t> sc, rc;
    for (const auto& x : sends) { sp.push_back(x.peer); st.push_back(x.patch); sb.push_back(send + x.offset); sc.push_back(x.size); }
    for (const auto& x : recvs) { rp.push_back(x.peer); rt.push_back(x.nbrPatch); rb.push_back(recv + x.offset); rc.push_back(x.size); }
    if (c->extExchange(c->extUser, (int32_t)sp.size(), sp.data(), st.data(), sb.data(), sc.data(), (int32_t)rp.size(), rp.data(), rt.data(), rb.data(), rc.data()) != 0)
        return fail(MI_ERR_DEVICE, "external communicator: exchange callback failed");
    return MI_OK;
}
} // namespace

// ---- one-shot peer all-reduce -------------------------------------------------------------------------------------------
// The two or three scalars a Krylov iteration all-reduces are latency, not bandwidth: a ring or tree collective costs a
// launch plus several link hops per call.  On a fully connected xGMI node every rank can write straight into every other
// rank's memory instead: each rank owns a WINDOW (a few hundred bytes of device memory exported with hipIpcGetMemHandle and
// mapped by its peers); an all-reduce of n <= PEER_MAX doubles is ONE single-workgroup kernel per rank that
//   1. takes the next epoch e from a device counter (so the kernel can sit in a hipGraph),
//   2. lane r stores the rank's n values and then, after a system-scope release fence, the flag e into slot [e&1][myRank]
//      of rank r's window,
//   3. lane r polls slot [e&1][r] of its OWN window until the flag reads e (system-scope acquire), bounded,
//   4. adds the nRanks contributions in RANK ORDER -- the same order on every rank, so all ranks hold the same bits.
// Two parities suffice: a peer can only be two epochs ahead of a rank that has not read yet if that rank had already
// written the epoch in between, which it does after its own read (stream order).  Memory: fine-grained device memory when
// the runtime exports it over IPC, ordinary device memory otherwise (sufficient between processes that share ONE device,
// which is how tests/test_distributed.py exercises it; between devices only the fine-grained form is coherent while a
// kernel runs).  Opt-in (mi_comm_peer_window + mi_comm_peer_connect); RCCL / the external transport stay the default and
// carry everything larger than PEER_MAX doubles.
// what a kernel needs of a communicator's all-reduce windows (by value in the kernel arguments)
struct PeerAR {
    double* const* peerWin; double* myWin; unsigned long long* epoch; int32_t* status;
    int32_t nRanks, myRank; long long maxPolls;
    int32_t fusedOff, repStride;   // the replicated part of the windows (doubles)
};
// The all-reduce itself, executed by the 64 lanes of ONE wavefront (the launch of k_peer_allreduce, or the last workgroup of a
// fused solver pass -- peer.inc): v[i], i < n, holds this rank's values in every lane; on return every lane holds the sums.
template <int NMAX>
__device__ __forceinline__ void peer_ar_wave(const PeerAR& A, double (&v)[NMAX], int n)
{
    const int r = threadIdx.x & 63;
    unsigned long long e = 0;
    if (r == 0) e = ++(*A.epoch);
    e = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(e >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(e & 0xffffffffull));
    const int par = (int)(e & 1ull);
    double got[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i) got[i] = 0.0;
    if (r < A.nRanks) {
        double* dst = A.peerWin[r] + ((size_t)par * A.nRanks + A.myRank) * PEER_SLOT;
#pragma unroll
        for (int i = 0; i < NMAX; ++i) if (i < n) __hip_atomic_store(dst + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst + PEER_MAX), e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        const double* src = A.myWin + ((size_t)par * A.nRanks + r) * PEER_SLOT;
        const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(src + PEER_MAX);
        long long polls = 0;
        const bool dead = *A.status != 0;                           // an earlier wait gave up: do not wait again
        while (!dead && __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != e) {
            if (++polls > A.maxPolls) { *A.status = 1; break; }     // a peer that never arrives must not hang the device
            __builtin_amdgcn_s_sleep(2);
        }
#pragma unroll
        for (int i = 0; i < NMAX; ++i) if (i < n) got[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
        double acc = 0.0;
        if (i < n) for (int k = 0; k < A.nRanks; ++k) acc += __shfl(got[i], k, 64);   // rank order: the same bits on every rank
        v[i] = acc;
    }
}
__global__ __launch_bounds__(64) void k_peer_allreduce(const PeerAR A, double* __restrict__ p, int n)
{
    double v[PEER_MAX];
#pragma unroll
    for (int i = 0; i < PEER_MAX; ++i) v[i] = i < n ? p[i] : 0.0;
    peer_ar_wave<PEER_MAX>(A, v, n);
    if (threadIdx.x == 0) for (int i = 0; i < n; ++i) p[i] = v[i];
}
namespace {
const long long PEER_POLLS = (long long)sw::get(SW_PEER_POLLS);   // several seconds (tests shorten it)
PeerAR peer_ar(const mi_comm_s* c, long long maxPolls = PEER_POLLS)
{
    return PeerAR{c->peerTable, c->window, c->epoch, c->peerStatus, c->nRanks, c->rank, maxPolls, (int32_t)peer_fused_off(c->nRanks), (int32_t)peer_rep_stride(c->nRanks)};
}
int peer_allreduce(mi_comm_s* c, hipStream_t stream, double* p, size_t n)
{
    k_peer_allreduce<<<1, 64, 0, stream>>>(peer_ar(c), p, (int)n);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
bool peer_takes(const mi_comm_s* c, size_t n) { return c->peerReady && n >= 1 && n <= (size_t)PEER_MAX; }
} // namespace
mi_comm_s::~mi_comm_s()
{
    for (size_t r = 0; r < peerWindow.size(); ++r) if (peerWindow[r] && (int)r != rank) (void)hipIpcCloseMemHandle(peerWindow[r]);
    if (window) (void)hipFree(window);
    if (epoch) (void)hipFree(epoch);
    if (peerStatus) (void)hipFree(peerStatus);
    if (peerTable) (void)hipFree(peerTable);
}

namespace {
// device memory a peer can map and poll: fine-grained when the runtime exports such an allocation over IPC (coherent between
// devices while a kernel runs), ordinary device memory otherwise (coherent only between processes that share ONE device)
int alloc_ipc_window(size_t bytes, void** out, bool* fineGrained)
{
    void* w = nullptr;
    hipIpcMemHandle_t h;
    *fineGrained = false;
    if (sw::get(SW_PEER_FINEGRAINED) && hipExtMallocWithFlags(&w, bytes, hipDeviceMallocFinegrained) == hipSuccess) {
        if (hipIpcGetMemHandle(&h, w) == hipSuccess) *fineGrained = true;
        else { (void)hipFree(w); w = nullptr; (void)hipGetLastError(); }
    } else (void)hipGetLastError();
    if (!w) HIPCHK(hipMalloc(&w, bytes));
    HIPCHK(hipMemset(w, 0, bytes));
    *out = w;
    return MI_OK;
}
// does the mapped pointer q live on this context's device? (windows in ordinary device memory are only usable then)
bool on_my_device(const mi_ctx_s* ctx, const void* q)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.device == ctx->device;
}
} // namespace

// this rank's window: allocates it and returns its 64-byte IPC handle for the peers
extern "C" int mi_comm_peer_window(mi_comm_t c, void* handle_out, int32_t len)
{
    if (!c || !handle_out || len < (int32_t)sizeof(hipIpcMemHandle_t)) return fail(MI_ERR_ARG, "mi_comm_peer_window: need a 64-byte buffer");
    if (c->nRanks > 64) return fail(MI_ERR_LIMIT, "mi_comm_peer_window: at most 64 ranks");
    HIPCHK(hipSetDevice(c->ctx->device));
    const size_t bytes = sizeof(double) * peer_window_doubles(c->nRanks);
    if (!c->window) {
        void* w = nullptr;
        MICHK(alloc_ipc_window(bytes, &w, &c->windowFineGrained));
        c->window = static_cast<double*>(w);
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->epoch), 2 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(c->epoch, 0, 2 * sizeof(unsigned long long)));
        c->fusedEpoch = c->epoch + 1;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->peerStatus), sizeof(int32_t)));
        HIPCHK(hipMemset(c->peerStatus, 0, sizeof(int32_t)));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->peerTable), sizeof(double*) * (size_t)c->nRanks));
        HIPCHK(hipMemset(c->peerTable, 0, sizeof(double*) * (size_t)c->nRanks));
    }
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, c->window));
    memcpy(handle_out, &h, sizeof(h));
    return MI_OK;
}
// handles of ALL ranks' windows in rank order (own entry ignored); afterwards every all-reduce of <= 8 doubles on this
// communicator goes through the windows.  Collective in the sense that every rank must have called it before the first
// all-reduce (the caller's barrier, e.g. the all-gather that distributed the handles plus one more barrier).
// Refused (MI_ERR_UNSUPPORTED, the communicator keeps its RCCL / external all-reduce) when the windows could not be
// allocated fine-grained AND a peer's window lives on another device: polling ordinary device memory of another GPU is not
// coherent while the kernel runs, every wait would run into its poll limit.
extern "C" int mi_comm_peer_connect(mi_comm_t c, const void* handles, int32_t n_handles)
{
    if (!c || !handles || n_handles != c->nRanks) return fail(MI_ERR_ARG, "mi_comm_peer_connect: bad argument");
    if (!c->window) return fail(MI_ERR_STATE, "mi_comm_peer_connect: call mi_comm_peer_window first");
    HIPCHK(hipSetDevice(c->ctx->device));
    c->peerWindow.assign((size_t)c->nRanks, nullptr);
    bool oneDevice = true;
    for (int r = 0; r < c->nRanks; ++r) {
        if (r == c->rank) { c->peerWindow[(size_t)r] = c->window; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, static_cast<const char*>(handles) + (size_t)r * sizeof(h), sizeof(h));
        void* q = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess));
        c->peerWindow[(size_t)r] = static_cast<double*>(q);
        if (!on_my_device(c->ctx, q)) oneDevice = false; else c->sharedDevice = true;
    }
    HIPCHK(hipMemcpy(c->peerTable, c->peerWindow.data(), sizeof(double*) * (size_t)c->nRanks, hipMemcpyHostToDevice));
    if (!c->windowFineGrained && !oneDevice && !sw::get(SW_PEER_ALLOW_COARSE))
        return fail(MI_ERR_UNSUPPORTED, "mi_comm_peer_connect: the window is ordinary (coarse-grained) device memory and a peer is on another device: "
                                        "not coherent while a kernel polls it; the communicator keeps its RCCL / external all-reduce");
    c->peerReady = true;
    return MI_OK;
}
// 0 = every wait so far met its peers; 1 = a wait ran out of polls (the sums after that are garbage: treat as fatal)
extern "C" int mi_comm_peer_status(mi_comm_t c, int32_t* status_out, int32_t* fine_grained_out)
{
    if (!c || !status_out) return fail(MI_ERR_ARG, "mi_comm_peer_status: bad argument");
    *status_out = 0;
    if (fine_grained_out) *fine_grained_out = c->windowFineGrained ? 1 : 0;
    if (!c->peerStatus) return MI_OK;
    HIPCHK(hipSetDevice(c->ctx->device));
    HIPCHK(hipStreamSynchronize(c->ctx->stream));
    HIPCHK(hipMemcpy(status_out, c->peerStatus, sizeof(int32_t), hipMemcpyDeviceToHost));
    return MI_OK;
}

namespace {
// the communicator's BASE transport (RCCL or the external callbacks), never the windows: what the peer set-up itself talks over
int base_allreduce(mi_comm_s* c, hipStream_t stream, double* p, size_t n)
{
    if (c->external()) return ext_allreduce(c, stream, p, n);
    NCCLCHK(rccl().AllReduce(p, p, n, ncclDouble, ncclSum, c->comm, stream));
    return MI_OK;
}
// all-gather of a few bytes per rank over the base all-reduce: the bytes travel as 16-bit integers in doubles (exact under
// summation with the other ranks' zeros, whatever the bit patterns of an IPC handle are)
int comm_gather_bytes(mi_comm_s* c, const unsigned char* mine, size_t nbytes, Table<unsigned char>& all)
{
    hipStream_t s = c->ctx->stream;
    const size_t per = (nbytes + 1) / 2, tot = per * (size_t)c->nRanks;
    Table<double> h(tot, 0.0);
    for (size_t k = 0; k < per; ++k) {
        const unsigned lo = mine[2 * k], hi = (2 * k + 1 < nbytes) ? mine[2 * k + 1] : 0u;
        h[(size_t)c->rank * per + k] = (double)(lo | (hi << 8));
    }
    DevBuf<double> d;
    MICHK(d.upload(h, s));
    MICHK(base_allreduce(c, s, d.p, tot));
    HIPCHK(hipMemcpyAsync(h.data(), d.p, sizeof(double) * tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    all.assign(nbytes * (size_t)c->nRanks, 0);
    for (int r = 0; r < c->nRanks; ++r)
        for (size_t k = 0; k < per; ++k) {
            const unsigned v = (unsigned)(h[(size_t)r * per + k] + 0.5);
            all[(size_t)r * nbytes + 2 * k] = (unsigned char)(v & 0xffu);
            if (2 * k + 1 < nbytes) all[(size_t)r * nbytes + 2 * k + 1] = (unsigned char)(v >> 8);
        }
    return MI_OK;
}
// true on every rank iff `ok` on every rank (one base all-reduce; doubles as a barrier); *agreed false also when the
// transport itself failed here
// the same for a few facts at once: sums[k] = how many ranks said yes to fact k
int comm_count_yes(mi_comm_s* c, int n, const bool* mine, int* sums)
{
    hipStream_t s = c->ctx->stream;
    Table<double> h((size_t)n);
    for (int k = 0; k < n; ++k) h[(size_t)k] = mine[k] ? 1.0 : 0.0;
    DevBuf<double> d;
    MICHK(d.upload(h, s));
    MICHK(base_allreduce(c, s, d.p, (size_t)n));
    HIPCHK(hipMemcpyAsync(h.data(), d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < n; ++k) sums[k] = (int)(h[(size_t)k] + 0.5);
    return MI_OK;
}
int comm_agree(mi_comm_s* c, bool ok, bool* agreed)
{
    hipStream_t s = c->ctx->stream;
    Table<double> h(1, ok ? 0.0 : 1.0);
    DevBuf<double> d;
    *agreed = false;
    MICHK(d.upload(h, s));
    MICHK(base_allreduce(c, s, d.p, 1));
    HIPCHK(hipMemcpyAsync(h.data(), d.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *agreed = h[0] < 0.5;
    return MI_OK;
}
__global__ void k_selftest_fill(double* p, int n, int rank, int round) { if ((int)threadIdx.x < n) p[threadIdx.x] = (double)((rank + 1) * (round + 1) + (int)threadIdx.x * 1000); }
} // namespace

// Coherence self-test of the all-reduce windows: `rounds` all-reduces of known values against every peer with a SHORT poll
// limit; *ok_out = 1 when every sum is right and no wait ran out.  All ranks call together, after every rank has connected
// (a window must be mapped before a peer writes into it: the caller's barrier, or mi_comm_peer_auto which does all of this).
extern "C" int mi_comm_peer_selftest(mi_comm_t c, int32_t rounds, int32_t* ok_out)
{
    if (!c || !ok_out || rounds < 1) return fail(MI_ERR_ARG, "mi_comm_peer_selftest: bad argument");
    if (!c->peerTable || c->peerWindow.empty()) return fail(MI_ERR_STATE, "mi_comm_peer_selftest: connect the windows first");
    HIPCHK(hipSetDevice(c->ctx->device));
    hipStream_t s = c->ctx->stream;
    DevBuf<double> d;
    MICHK(d.alloc(PEER_MAX));
    Table<double> h(PEER_MAX);
    bool ok = true;
    const long long R = c->nRanks;
    for (int round = 0; round < rounds; ++round) {
        const int n = 1 + round % PEER_MAX;
        k_selftest_fill<<<1, 64, 0, s>>>(d.p, n, c->rank, round);
        k_peer_allreduce<<<1, 64, 0, s>>>(peer_ar(c, 4000000ll), d.p, n);   // a fraction of a second per wait at most
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.data(), d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) if (h[(size_t)i] != (double)((R * (R + 1) / 2) * (round + 1) + R * i * 1000)) ok = false;
    }
    int32_t st = 0;
    HIPCHK(hipMemcpy(&st, c->peerStatus, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (st != 0) { ok = false; HIPCHK(hipMemset(c->peerStatus, 0, sizeof(int32_t))); }
    *ok_out = ok ? 1 : 0;
    return MI_OK;
}
// switch the windows on or off for the all-reduces of <= 8 doubles (after a self-test the ranks have agreed on)
extern "C" int mi_comm_peer_enable(mi_comm_t c, int32_t on)
{
    if (!c) return fail(MI_ERR_ARG, "mi_comm_peer_enable: bad argument");
    if (on && (!c->peerTable || c->peerWindow.empty())) return fail(MI_ERR_STATE, "mi_comm_peer_enable: connect the windows first");
    c->peerReady = on != 0;
    return MI_OK;
}
// Everything in one collective call: allocate the window, all-gather the IPC handles over the communicator's own transport,
// map the peers, self-test, agree.  *enabled_out = 1: the scalars of the Krylov loops (and the halo of matrices attached from
// now on, peer.inc) travel through the windows; 0: some rank could not (no IPC, not coherent, self-test failed) and EVERY rank
// keeps the base transport.  Never an error for that reason.
extern "C" int mi_comm_peer_auto(mi_comm_t c, int32_t* enabled_out)
{
    if (!c || !enabled_out) return fail(MI_ERR_ARG, "mi_comm_peer_auto: bad argument");
    *enabled_out = 0;
    HIPCHK(hipSetDevice(c->ctx->device));
    unsigned char mine[sizeof(hipIpcMemHandle_t)] = {0};
    bool ok = c->nRanks <= 64 && mi_comm_peer_window(c, mine, (int32_t)sizeof(mine)) == MI_OK;
    bool all = false;
    MICHK(comm_agree(c, ok, &all));
    if (!all) return MI_OK;
    Table<unsigned char> handles;
    MICHK(comm_gather_bytes(c, mine, sizeof(mine), handles));
    ok = mi_comm_peer_connect(c, handles.data(), c->nRanks) == MI_OK;
    c->peerReady = false;                                   // not before the ranks have agreed
    MICHK(comm_agree(c, ok, &all));                         // also the barrier: every window is mapped before anyone writes
    if (!all) return MI_OK;
    int32_t pass = 0;
    ok = mi_comm_peer_selftest(c, 24, &pass) == MI_OK && pass == 1;
    MICHK(comm_agree(c, ok, &all));
    if (!all) return MI_OK;
    c->peerReady = true;
    *enabled_out = 1;
    return MI_OK;
}

// state of a C++-driven distributed PCG session (buffers come from mi_dpcg_set_buffers)
struct PeerHalo;
struct mi_dpcg_comm_s {
    mi_comm_s *reduce = nullptr, *halo = nullptr;
    struct P2P { int32_t patch, peer, nbrPatch, offset, size; };
    Table<P2P> sends, recvs;   // sends in patch order; recvs in the peer's send order
    PeerHalo* ph = nullptr;          // halo windows of this matrix (peer.inc), or nullptr: the communicator's own send/recv
    Table<int32_t> recvs_patch; // patch of every entry of recvs (factors of transformed patches)
    hipStream_t commStream = nullptr;
    hipEvent_t evPack = nullptr, evHalo = nullptr;
    bool anyFactor = false;          // ... has a transformed (processorCyclic) patch, factor != 1: no phase pipeline (it does not scale what it receives)
    bool anyCompact = false;         // ... runs the 16-bit entry form (MI_ENTRY16=1 and a mesh that allows it): no paired / batched passes anywhere
    bool anyAmi = false;             // SOME rank's matrix of this decomposed case has cyclicAMI patches (agreed at attach time): every rank then takes the tile-operator pipelines, so that all ranks issue the same exchanges and all-reduces
    int64_t nGlobal = 0;
    int32_t it = 0;
};

extern "C" int mi_comm_unique_id(void* id_out, int32_t len)
{
    if (!id_out || len < (int32_t)NCCL_UNIQUE_ID_BYTES) return fail(MI_ERR_ARG, "mi_comm_unique_id: need a 128-byte buffer");
    if (!rccl().load()) return fail(MI_ERR_DEVICE, rccl().err);
    ncclUniqueId id;
    NCCLCHK(rccl().GetUniqueId(&id));
    memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
    return MI_OK;
}

extern "C" int mi_comm_create(mi_ctx_t ctx, int32_t n_ranks, int32_t rank, const void* id, mi_comm_t* out)
{
    if (!ctx || !id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MI_ERR_ARG, "mi_comm_create: bad argument");
    if (!rccl().load()) return fail(MI_ERR_DEVICE, rccl().err);
    HIPCHK(hipSetDevice(ctx->device));
    ncclUniqueId uid;
    memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
    mi_comm_s* c = new mi_comm_s;
    c->ctx = ctx; c->nRanks = n_ranks; c->rank = rank;
    const ncclResult_t r = rccl().CommInitRank(&c->comm, n_ranks, uid, rank);
    if (r != ncclSuccess) { delete c; return fail(MI_ERR_DEVICE, std::string("rccl: ncclCommInitRank: ") + rccl().GetErrorString(r)); }
    *out = c;
    return MI_OK;
}

extern "C" int mi_comm_create_external(mi_ctx_t ctx, int32_t n_ranks, int32_t rank, mi_comm_allreduce_fn allreduce, mi_comm_exchange_fn exchange,
                                       void* user, mi_comm_t* out)
{
    if (!ctx || !out || !allreduce || !exchange || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MI_ERR_ARG, "mi_comm_create_external: bad argument");
    mi_comm_s* c = new mi_comm_s;
    c->ctx = ctx; c->nRanks = n_ranks; c->rank = rank;
    c->extAllreduce = allreduce; c->extExchange = exchange; c->extUser = user;
    *out = c;
    return MI_OK;
}

extern "C" int mi_comm_destroy(mi_comm_t c)
{
    if (!c) return MI_OK;
    (void)hipSetDevice(c->ctx->device);
    if (c->comm) rccl().CommDestroy(c->comm);
    delete c;
    return MI_OK;
}

// in-place sum over the ranks on the engine's stream (Foam::reduce(..., sumOp<scalar>()))
extern "C" int mi_comm_allreduce_sum(mi_comm_t c, double* buf_dev, int64_t n)
{
    if (!c || !buf_dev || n < 0) return fail(MI_ERR_ARG, "mi_comm_allreduce_sum: bad argument");
    HIPCHK(hipSetDevice(c->ctx->device));
    if (peer_takes(c, (size_t)n)) return peer_allreduce(c, c->ctx->stream, buf_dev, (size_t)n);
    if (c->external()) return ext_allreduce(c, c->ctx->stream, buf_dev, (size_t)n);
    NCCLCHK(rccl().AllReduce(buf_dev, buf_dev, (size_t)n, ncclDouble, ncclSum, c->comm, c->ctx->stream));
    return MI_OK;
}

bool comm_attached(const mi_matrix_s* m) { return m->dpc && m->dpc->reduce; }
bool comm_remote(const mi_matrix_s* m) { return m->dpc && m->dpc->halo && !m->dpc->sends.empty(); }
bool comm_any_ami(const mi_matrix_s* m) { return !m->addr->ami.empty() || (m->dpc && m->dpc->reduce && m->dpc->anyAmi); }
// (declared, whatever its present value: the factor of a transformed patch changes with the component being solved)
bool matrix_has_factor(const mi_matrix_s* m) { return !m->patchFactor.empty(); }
// (attached: ONLY what the ranks agreed on -- a factor of 1 declared on one rank after the attach must not change that rank's pipeline)
bool comm_any_factor(const mi_matrix_s* m) { return (m->dpc && m->dpc->reduce) ? m->dpc->anyFactor : matrix_has_factor(m); }
// a GAMG level matrix takes its transformation factors from the finest matrix AFTER it was attached: what the ranks agreed on for
// the finest matrix (transformed patches somewhere in the case) holds for its levels
void comm_inherit_factor_flag(mi_matrix_s* level, const mi_matrix_s* fine) { if (level->dpc && fine->dpc) level->dpc->anyFactor = fine->dpc->anyFactor; }
bool comm_any_compact(const mi_matrix_s* m) { return m->addr->compact || (m->dpc && m->dpc->reduce && m->dpc->anyCompact); }
int64_t comm_n_global(const mi_matrix_s* m) { return m->dpc ? m->dpc->nGlobal : 0; }

int comm_exchange_start(mi_matrix_s* m, const double* send, double* vec)
{
    mi_dpcg_comm_s& D = *m->dpc;
    if (D.sends.empty()) return MI_OK;
    mi_ctx_s* c = m->addr->ctx;
    const int64_t n = m->addr->L.nCells;
    if (D.halo->external()) return ext_exchange(D.halo, c->stream, D.sends, D.recvs, send, vec + n);   // blocking: nothing to wait for later
    HIPCHK(hipEventRecord(D.evPack, c->stream));          // the pack kernel has to finish first
    HIPCHK(hipStreamWaitEvent(D.commStream, D.evPack, 0));
    NCCLCHK(rccl().GroupStart());
    for (const auto& s : D.sends) NCCLCHK(rccl().Send(send + s.offset, (size_t)s.size, ncclDouble, s.peer, D.halo->comm, D.commStream));
    for (const auto& r : D.recvs) NCCLCHK(rccl().Recv(vec + n + r.offset, (size_t)r.size, ncclDouble, r.peer, D.halo->comm, D.commStream));
    NCCLCHK(rccl().GroupEnd());
    HIPCHK(hipEventRecord(D.evHalo, D.commStream));
    return MI_OK;
}
int comm_exchange_wait(mi_matrix_s* m)
{
    mi_dpcg_comm_s& D = *m->dpc;
    if (D.sends.empty() || D.halo->external()) return MI_OK;
    HIPCHK(hipStreamWaitEvent(m->addr->ctx->stream, D.evHalo, 0));
    return MI_OK;
}
int comm_allreduce(mi_matrix_s* m, double* p, size_t n)
{
    mi_dpcg_comm_s& D = *m->dpc;
    if (peer_takes(D.reduce, n)) return peer_allreduce(D.reduce, m->addr->ctx->stream, p, n);
    if (D.reduce->external()) return ext_allreduce(D.reduce, m->addr->ctx->stream, p, n);
    NCCLCHK(rccl().AllReduce(p, p, n, ncclDouble, ncclSum, D.reduce->comm, m->addr->ctx->stream));
    return MI_OK;
}

// one grouped exchange of doubles with explicit plans (GAMG hierarchy build: restrict addressing of the patch cells)
int comm_p2p_raw(mi_comm_s* halo, hipStream_t stream, const Table<mi_dpcg_comm_s::P2P>& sends,
                 const Table<mi_dpcg_comm_s::P2P>& recvs, const double* send, double* recv)
{
    if (sends.empty()) return MI_OK;
    if (halo->external()) return ext_exchange(halo, stream, sends, recvs, send, recv);
    NCCLCHK(rccl().GroupStart());
    for (const auto& s : sends) NCCLCHK(rccl().Send(send + s.offset, (size_t)s.size, ncclDouble, s.peer, halo->comm, stream));
    for (const auto& r : recvs) NCCLCHK(rccl().Recv(recv + r.offset, (size_t)r.size, ncclDouble, r.peer, halo->comm, stream));
    NCCLCHK(rccl().GroupEnd());
    return MI_OK;
}
int comm_allreduce_raw(mi_comm_s* reduce, hipStream_t stream, double* p, size_t n)
{
    if (peer_takes(reduce, n)) return peer_allreduce(reduce, stream, p, n);
    if (reduce->external()) return ext_allreduce(reduce, stream, p, n);
    NCCLCHK(rccl().AllReduce(p, p, n, ncclDouble, ncclSum, reduce->comm, stream));
    return MI_OK;
}

#include "peer.inc"

// Attach the communicators to a matrix.  From here on the matrix behaves like the reference's lduMatrix on a
// decomposed case: Amul/Tmul/residual/H/Jacobi exchange the processor-patch values themselves, every global sum of
// the solvers is all-reduced, and mi_pcg/pbicg/pbicgstab/smooth_solve solve the global system (all ranks call them
// together, like the MPI ranks of the reference).
// patch_rank[p] = rank that owns the other side of processor patch p (ignored for local/cyclic patches);
// patch_nbr_patch[p] = index of the matching patch over there (NULL: same index).
extern "C" int mi_matrix_attach_comm(mi_matrix_t m, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                                     const int32_t* patch_nbr_patch, int64_t n_global)
{
    if (!m || !reduce || !halo || n_global <= 0) return fail(MI_ERR_ARG, "mi_matrix_attach_comm: bad argument");
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    if (reduce->ctx != c || halo->ctx != c) return fail(MI_ERR_ARG, "mi_matrix_attach_comm: communicator belongs to another context");
    HIPCHK(hipSetDevice(c->device));
    if (!m->dpc) {
        m->dpc = new mi_dpcg_comm_s;
        HIPCHK(hipStreamCreateWithFlags(&m->dpc->commStream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&m->dpc->evPack, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->dpc->evHalo, hipEventDisableTiming));
    }
    mi_dpcg_comm_s& D = *m->dpc;
    D.reduce = nullptr; D.halo = nullptr; D.nGlobal = n_global; D.it = 0;
    D.sends.clear(); D.recvs.clear();
    const TileLayout& L = a->L;
    for (int32_t p = 0; p < L.nPatches; ++p) {
        if (a->patchIsLocal[(size_t)p]) continue;
        if (!patch_rank) return fail(MI_ERR_ARG, "mi_matrix_attach_comm: patch_rank is required with processor patches");
        const int32_t peer = patch_rank[p];
        if (peer < 0 || peer >= halo->nRanks) return fail(MI_ERR_ARG, "mi_matrix_attach_comm: patch_rank out of range");
        const int32_t size = L.patchOffset[(size_t)p + 1] - L.patchOffset[p];
        if (size == 0) continue;
        mi_dpcg_comm_s::P2P e{p, peer, patch_nbr_patch ? patch_nbr_patch[p] : p, L.patchOffset[p], size};
        D.sends.push_back(e); D.recvs.push_back(e);
    }
    // a peer sends its patches in ITS patch order: post our receives from that peer in the same order
    std::stable_sort(D.recvs.begin(), D.recvs.end(), [](const mi_dpcg_comm_s::P2P& x, const mi_dpcg_comm_s::P2P& y) {
        return x.peer != y.peer ? x.peer < y.peer : x.nbrPatch < y.nbrPatch; });
    D.reduce = reduce; D.halo = halo;
    // which solver pipeline a rank takes depends on whether the case has cyclicAMI patches, transformed patches or the 16-bit
    // entry form -- on ANY rank: ranks that decided it from their own patches would issue different sequences of exchanges and
    // all-reduces (collective: as the window set-up below, every rank attaches its matching matrix at this point; the factors
    // of transformed patches are therefore set BEFORE the attach, mi_matrix_set_patch_transform refuses a new one after it)
    {
        const bool mine[3] = {!a->ami.empty(), matrix_has_factor(m), a->compact};
        int yes[3] = {0, 0, 0};
        MICHK(comm_count_yes(reduce, 3, mine, yes));
        D.anyAmi = yes[0] > 0; D.anyFactor = yes[1] > 0; D.anyCompact = yes[2] > 0;
    }
    // halo windows: kept while the exchange plan is the one they were built for; built (COLLECTIVELY -- every rank attaches its
    // matching matrix at this point, as every caller in this engine does) when the communicator runs in peer mode
    if (D.ph) {
        bool same = D.ph->patchRank.size() == D.sends.size() && D.ph->nExt == L.nExt;
        for (size_t q = 0; same && q < D.sends.size(); ++q) same = D.ph->patchRank[q] == D.sends[q].peer;
        if (!same) { delete D.ph; D.ph = nullptr; }
    }
    if (!D.ph && reduce->peerReady && sw::get(SW_PEER_HALO)) {
        int32_t on = 0;
        MICHK(mi_matrix_peer_halo_auto(m, &on));
    }
    return MI_OK;
}

// coupledFvPatchField::patchNeighbourField (processorFvPatchField.C:107-135: the values received from the neighbour
// processor; cyclicFvPatchField.C:109-150: the partner patch's internal values): for every interface face the value of
// psi in the cell on the other side, caller patch order.  Remote patches: pack -> one grouped send/recv on the halo
// communicator (all ranks call together); without an attached communicator they return what mi_matrix_set_ext placed.
extern "C" int mi_matrix_patch_neighbour_field(mi_matrix_t m, const double* psi, double* out)
{
    if (!m || !psi) return fail(MI_ERR_ARG, "mi_matrix_patch_neighbour_field: bad argument");
    mi_addr_s* a = m->addr;
    const int32_t nExt = a->L.nExt;
    if (nExt == 0) return MI_OK;
    if (!out) return fail(MI_ERR_ARG, "mi_matrix_patch_neighbour_field: out is NULL");
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (a->ifaceNbrCaller.n != (size_t)nExt) {
        Table<int32_t> nb((size_t)nExt, -1);
        for (int32_t p = 0; p < a->L.nPatches; ++p)
            if (a->patchIsLocal[(size_t)p])
                for (size_t i = 0; i < a->patchNbrCellsHost[(size_t)p].size(); ++i) nb[(size_t)a->L.patchOffset[p] + i] = a->patchNbrCellsHost[(size_t)p][i];
        MICHK(a->ifaceNbrCaller.upload(nb, s));
    }
    double* v0;
    MICHK(m->vec(WV_OP_X, &v0));
    if (comm_remote(m) || !a->ami.empty()) k_gather_perm<<<RG, RB, 0, s>>>(psi, a->perm(), v0, a->L.nCells);
    if (!a->ami.empty() && !(a->amiRemote && comm_remote(m))) MICHK(ami_fill(m, v0)); // cyclicAMI: interpolated (and transformed) partner values
    if (comm_remote(m)) {
        if (m->sendBuf.n < (size_t)nExt) MICHK(m->sendBuf.alloc((size_t)nExt));
        MICHK(mi_halo_pack_engine(a, v0, m->sendBuf.p));
        MICHK(comm_exchange_start(m, m->sendBuf.p, v0));
        MICHK(comm_exchange_wait(m));
        MICHK(scale_received(m, v0));
        if (a->amiRemote) MICHK(ami_fill(m, v0));   // partner on another rank: interpolate from what the transport patch received
    }
    k_patch_nbr_field<<<(nExt + 255) / 256, 256, 0, s>>>(psi, a->ifaceNbrCaller.p, v0 + a->L.nCells, out, nExt);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_matrix_detach_comm(mi_matrix_t m)
{
    if (!m) return fail(MI_ERR_ARG, "mi_matrix_detach_comm: bad argument");
    if (m->dpc) { m->dpc->reduce = nullptr; m->dpc->halo = nullptr; m->dpc->sends.clear(); m->dpc->recvs.clear(); delete m->dpc->ph; m->dpc->ph = nullptr; }
    return MI_OK;
}

namespace {
// prologue of the distributed PCG (PCG.C:75-118): everything up to the first convergence test
int dpcg_prologue(mi_matrix_s* m)
{
    mi_ctx_s* c = m->addr->ctx;
    const mi_dpcg_s& B = m->dp;
    m->dpc->it = 0;
    MICHK(mi_dpcg_phase(m, 0, 0, 0.0));
    MICHK(comm_exchange_start(m, B.send, B.psi));
    MICHK(comm_exchange_wait(m));
    MICHK(mi_dpcg_phase(m, 1, 0, 0.0));
    MICHK(comm_allreduce(m, B.scal + 3, 1));
    double sumPsi = 0.0;                                  // gAverage(psi): the one host read of the prologue
    HIPCHK(hipMemcpyAsync(&sumPsi, B.scal + 3, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    MICHK(mi_dpcg_phase(m, 2, 0, sumPsi / (double)m->dpc->nGlobal));
    MICHK(comm_allreduce(m, B.scal + 0, 2));
    MICHK(comm_allreduce(m, B.scal + 4, 1));
    MICHK(mi_dpcg_phase(m, 3, 0, 0.0));
    return MI_OK;
}
} // namespace

// attach + prologue in one call (buffers and controls come from mi_dpcg_set_buffers)
extern "C" int mi_dpcg_comm_begin(mi_matrix_t m, mi_comm_t reduce, mi_comm_t halo, const int32_t* patch_rank,
                                  const int32_t* patch_nbr_patch, int64_t n_global)
{
    if (!m || !m->dp.psi) return fail(MI_ERR_STATE, "mi_dpcg_comm_begin: call mi_dpcg_set_buffers first");
    MICHK(mi_matrix_attach_comm(m, reduce, halo, patch_rank, patch_nbr_patch, n_global));
    return dpcg_prologue(m);
}

// enqueue n_iters iterations (device no-ops once converged); no host synchronisation.  record_amul_events = s > 0
// brackets the Amul phases of every s-th enqueued iteration (k = 0, s, 2s, ...) with the events 2(k/s), 2(k/s)+1
// (read them with mi_event_elapsed_ms); sampling keeps the event records out of the latency-bound small-domain loop
extern "C" int mi_dpcg_comm_iterate(mi_matrix_t m, int32_t n_iters, int32_t record_amul_events)
{
    if (!m || !comm_attached(m) || !m->dp.psi || n_iters < 0) return fail(MI_ERR_STATE, "mi_dpcg_comm_iterate: call mi_dpcg_comm_begin first");
    mi_dpcg_comm_s& D = *m->dpc;
    const mi_dpcg_s& B = m->dp;
    HIPCHK(hipSetDevice(m->addr->ctx->device));
    if (dpcg_fused_usable(m)) return dpcg_fused_iterate(m, n_iters, record_amul_events);   // three launches, no collective call (peer.inc)
    for (int32_t k = 0; k < n_iters; ++k) {
        const int32_t it = D.it;
        MICHK(mi_dpcg_phase(m, 10, it, 0.0));
        MICHK(comm_exchange_start(m, B.send, B.pA));
        const bool rec = record_amul_events > 0 && (k % record_amul_events) == 0;
        if (rec) MICHK(mi_event_record(m, 2 * (k / record_amul_events)));
        MICHK(mi_dpcg_phase(m, 11, it, 0.0));             // interior tiles overlap the exchange
        MICHK(comm_exchange_wait(m));
        MICHK(mi_dpcg_phase(m, 12, it, 0.0));             // boundary tiles
        if (rec) MICHK(mi_event_record(m, 2 * (k / record_amul_events) + 1));
        MICHK(comm_allreduce(m, B.scal + 2, 1));
        MICHK(mi_dpcg_phase(m, 13, it, 0.0));
        MICHK(comm_allreduce(m, B.scal + 0, 2));
        D.it++;
    }
    if (n_iters > 0) MICHK(mi_dpcg_phase(m, 14, D.it - 1, 0.0));
    return MI_OK;
}

// mi_pcg_solve on a matrix with a communicator attached: the global system, all ranks together.
// diagonal / no preconditioner: the device-resident phase pipeline above; AINV (= DIC): host-stepped loop
// (PCG.C:68-208) on the communicator-aware operators.
int pcg_solve_attached(mi_matrix_s* m, double* psi_io, const double* source, const mi_solver_controls* ctl, int precond,
                       mi_solver_perf* perf, double* hist_host, int32_t hist_len)
{
    mi_addr_s* a = m->addr;
    mi_ctx_s* c = a->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = a->L.nCells;
    PcgVecs v;
    MICHK(stage_in(m, v, psi_io, source));
    double *psi = v.psi, *src = v.src, *pA = v.pA, *wA = v.wA, *rA = v.rA;
    // (cyclicAMI / transformed patches: the phase pipeline below does not interpolate them; the tile-operator pipeline does)
    if ((precond == MI_PRECOND_DIAGONAL || precond == MI_PRECOND_NONE) && !comm_any_ami(m) && !comm_any_factor(m)) {
        if (m->dscal.n < 8) { MICHK(m->dscal.alloc(8)); HIPCHK(hipMemsetAsync(m->dscal.p, 0, 8 * sizeof(double), s)); }
        if (m->sendBuf.n < (size_t)std::max(a->L.nExt, 1)) MICHK(m->sendBuf.alloc((size_t)std::max(a->L.nExt, 1)));
        MICHK(mi_dpcg_set_buffers(m, psi, src, pA, wA, rA, m->dscal.p, m->sendBuf.p, ctl, precond, ctl->maxIter + 2));
        MICHK(dpcg_prologue(m));
        MICHK(fetch_state(c));
        // full batches from the start; mi_dpcg_comm_iterate counts the iterations in m->dpc->it
        MICHK(drive_batches(m, ctl, m->dpc->it, c->pcgBatch, [m](int nb) { return mi_dpcg_comm_iterate(m, nb, 0); }));
        MICHK(finish_device(m, psi, psi_io, perf, hist_host, hist_len, dpcg_flush_if_fused));
        m->dp = mi_dpcg_s();
        return MI_OK;
    }
    if (c->pbicgHostStepped == 0) {
        // AINV (= DIC): the single-GPU device-resident pipeline (pcg_enqueue: AINV tile pass with the fused wA.rA sum, Amul with
        // the fused wA.pA sum, one vector pass), its sums all-reduced on the device (globalize); the host polls `done` per batch
        MICHK(solve_prologue(m, ctl, psi, src, wA, rA, ctl->maxIter + 2));
        MICHK(pcg_first_dot(m, precond, v));   // (diagonal / none on this pipeline: a case with cyclicAMI or transformed patches)
        MICHK(fetch_state(c));
        int it = 0;
        MICHK(drive_batches(m, ctl, it, 2, [&](int nb) { it += nb; return pcg_enqueue(m, it - nb, nb, precond, 0); }));
        return finish_device(m, psi, psi_io, perf, hist_host, hist_len, pcg_flush);
    }
    HostPerf hp; Table<double> hist;
    MICHK(host_prologue(m, ctl, psi, src, wA, rA, hp, hist));
    double wArA = SP_GREAT, wArAold = wArA;
    if (hp.minIter > 0 || !hp.checkConvergence()) {
        do {
            wArAold = wArA;
            MICHK(precond_engine(m, precond, false, rA, wA));
            MICHK(reduce_sync<RED_PROD>(m, wA, rA, &wArA));
            if (hp.nIterations == 0) HIPCHK(hipMemcpyAsync(pA, wA, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
            else k_xpsy<<<RG, RB, 0, s>>>(pA, wA, wArA / wArAold, pA, n);
            MICHK(tile_op<OP_AMUL>(m, false, pA, nullptr, nullptr, wA, 0.0));
            double wApA = 0;
            MICHK(reduce_sync<RED_PROD>(m, wA, pA, &wApA));
            if (hp.checkSingularity(fabs(wApA) / hp.normFactor)) break;
            const double alpha = wArA / wApA;
            k_xpsy<<<RG, RB, 0, s>>>(psi, psi, alpha, pA, n);
            k_xpsy<<<RG, RB, 0, s>>>(rA, rA, -alpha, wA, n);
            double sm = 0;
            MICHK(reduce_sync<RED_MAG>(m, rA, nullptr, &sm));
            hp.finalResidual = sm / hp.normFactor;
            hist.push_back(hp.finalResidual);
        } while ((hp.nIterations++ < hp.maxIter && !hp.checkConvergence()) || hp.nIterations < hp.minIter);
    }
    return finish_host(m, hp, hist, psi, psi_io, perf, hist_host, hist_len);
}
