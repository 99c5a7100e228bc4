// switches.hpp -- the ONE list of the MI_* environment switches that csrc/ reads, and the only code that reads them.
// Plain C++: the host-only translation units (tiling.cpp, gamg.cpp) include it as well as engine.hip.
//
// One X(...) line per switch:
//   X(id, environment name | nullptr, default, read when, purpose group, run-time option name | nullptr, meaning)
// A reader calls sw::get(SW_id), at the place in the control flow that the "read when" column names -- WHEN a switch is read is
// part of its behaviour (the tests set and unset variables around calls on live contexts), so a read must not move:
//   ONCE     once per process: when the library loads (MI_PEER_POLLS) or at first use, then frozen (static const)
//   CTX      at mi_ctx_create, into a member of mi_ctx_s (engine.hip: CTX_SWITCHES); those with an option name also by mi_ctx_set_option
//   ADDR     when an addressing is created (mi_addr_create*, the level addressings of a GAMG hierarchy, mi_layout_*_host)
//   ROWS     at the first caller-order operator of an addressing (assembly.inc: ensure_caller_tables)
//   HIER     at hierarchy creation (mi_gamg_create*)
//   ATTACH   at attach / window set-up (mi_comm_peer_*, mi_matrix_attach_comm)
//   PERSIST  at persistent-kernel set-up (persist.inc: the first persist_fits_layout of a context)
//   CALL     on every call of the operator / solver / launch that asks
// Purpose groups (DESIGN.md, appendix "switches", which tests/test_switches.py holds to this list): USER a user may need; AB the
// A/B hook of a default that won, same results either way; TRANSPORT transports and their self-tests; DIAG fault injection and
// diagnostics (tests).
// The hashed part of gamg_engine.inc (tools/source_fingerprint.py) still spells four reads as env_int("MI_...", default); the
// same test holds those defaults to this list.
#pragma once
#include <cstdlib>

namespace mi {
// clang-format off
#define MI_SWITCHES(X) \
    X(HOST_THREADS,            "MI_HOST_THREADS",            0,        ONCE,          USER,      nullptr,               "host threads of the one-time builds, clamped to 1..64; unset: the hardware's, divided by the launcher's local world size (host_parallel.hpp)") \
    X(HOST_THP,                "MI_HOST_THP",                1,        ONCE,          USER,      nullptr,               "host tables >= 4 MiB on 2 MiB boundaries, advised to transparent huge pages; a value that starts with 0: plain malloc (host_tables.hpp)") \
    X(PCG_PERSIST,             "MI_PCG_PERSIST",             1,        CTX,           USER,      "pcg_persist",         "0 never, 1 the persistent PCG kernel whenever the tiles fit the CUs' registers (persist.inc)") \
    X(WIN_DIRECT,              "MI_WIN_DIRECT",              1,        CTX,           USER,      "win_direct",          "tile operators of attached matrices read neighbour-rank values straight from the halo window (one launch for all tiles) instead of k_halo_pull + a second launch; 2 = also between processes that share a device") \
    X(PEER_POLLS,              "MI_PEER_POLLS",              20000000, ONCE,          USER,      nullptr,               "polls before a wait on a peer window gives up: several seconds (tests shorten it); read when the library loads (comm.inc: PEER_POLLS)") \
    X(GAMG_GRAPH,              "MI_GAMG_GRAPH",              1,        CTX,           USER,      nullptr,               "the V-cycle replays as a hipGraph; 0 = plain launches") \
    X(GAMG_GRAPH_ATTACHED,     "MI_GAMG_GRAPH_ATTACHED",     1,        CTX,           USER,      "gamg_graph_attached", "the V-cycle of a decomposed case replays as a hipGraph when every exchange of it is stream work (peer windows)") \
    X(TILE_REORDER,            "MI_TILE_REORDER",            -1,       ADDR,          USER,      nullptr,               "-1: Cuthill-McKee pre-ordering when the numbering has no locality, 0 never, 1 always (tiling.hpp)") \
    X(TILE_CELLS,              "MI_TILE_CELLS",              0,        ADDR,          USER,      nullptr,               "cells per tile; 0: 1024, coarse GAMG levels by MI_SMALL_TILES (engine.hip: addr_tile_params)") \
    X(TILE_SLOTS,              "MI_TILE_SLOTS",              4094,     ADDR,          USER,      nullptr,               "coefficient slots per tile") \
    \
    X(GAMG_FUSE,               "MI_GAMG_FUSE",               1,        CTX,           AB,        nullptr,               "fused transfers of the V-cycle (default cycle shape, single rank); 0 = the separate kernels") \
    X(FUSE_PROLOGUE,           "MI_FUSE_PROLOGUE",           1,        CTX,           AB,        "fuse_prologue",       "A psi, source - A psi and sumA in one pass over the coefficients, the prologue's sums batched; 0 = the separate passes, same bits") \
    X(PCG_FUSE_RP,             "MI_PCG_FUSE_RP",             1,        CTX,           AB,        "pcg_fuse_rp",         "residual update + next direction update as one launch (pcg_fused.inc); stored as 0 never, -1 once the device has been asked") \
    X(GAMG_INVERT_V2,          "MI_GAMG_INVERT_V2",          1,        CALL,          AB,        nullptr,               "the rewritten register-resident inversion kernel of the coarsest level; 0 = its first form, same bits") \
    X(MULTI_PIPE,              "MI_MULTI_PIPE",              1,        CTX,           AB,        nullptr,               "the multi-vector tile passes of the Krylov iterations as persistent pipelined workgroups (multi_pipe.inc): same bits, three-component PBiCG + DILU iteration 1 812 -> 1 643 us (profiles/r05_f_multi_pipe_ab.md)") \
    X(MULTI_TILE,              "MI_MULTI_TILE",              1,        CALL,          AB,        nullptr,               "multi-vector tile kernel for several right-hand sides; 0 = one single-vector launch each (multi.inc)") \
    X(PBICG_MULTI,             "MI_PBICG_MULTI",             1,        CALL,          AB,        nullptr,               "mi_pbicg_solve_multi runs its components as one multi-vector solve; 0 = one after the other (multi.inc)") \
    X(PBICG_PAIR,              "MI_PBICG_PAIR",              1,        CTX,           AB,        nullptr,               "PBiCG's A p / A^T pT (and the DILU pair) in one pass over the coefficients") \
    X(ROW16,                   "MI_ROW16",                   1,        ROWS,          AB,        nullptr,               "block-local 16-bit row tables of the assembly row passes (assembly.inc: R16)") \
    X(ENTRY16,                 "MI_ENTRY16",                 0,        ADDR,          AB,        nullptr,               "opt-in 16-bit row entries: half the entry bytes, measured 2-4 % slower (profiles/r01_n_compact_entries_ab.md)") \
    X(GAMG_DIRECT_SLOTS,       "MI_GAMG_DIRECT_SLOTS",       1,        HIER,          AB,        nullptr,               "direct agglomeration: slot-to-slot children lists between the levels' tile layouts") \
    X(GAMG_REG_INVERT,         "MI_GAMG_REG_INVERT",         1,        CALL,          AB,        nullptr,               "coarsest systems of up to 192 rows are inverted in registers") \
    X(GAMG_INVERT_OVERLAP,     "MI_GAMG_INVERT_OVERLAP",     1,        CALL,          AB,        nullptr,               "the coarsest-level inversion runs on the side stream beside the solve's prologue and first down-sweep") \
    X(GAMG_PIPELINE,           "MI_GAMG_PIPELINE",           1,        HIER,          AB,        nullptr,               "level layouts and transfer maps are built on other threads while the next level is matched") \
    X(GAMG_INHERIT_TILES,      "MI_GAMG_INHERIT_TILES",      0,        HIER,          AB,        nullptr,               "opt-in: a level takes its tiles from its fine side's tiles instead of clustering again (tiling.hpp: inherit_tiles); no gain measured") \
    X(GAMG_DEVICE_INVERT,      "MI_GAMG_DEVICE_INVERT",      -1,       CTX,           AB,        nullptr,               "inversion of the coarsest level: -1 by size, 0 on the host, 1 on the device") \
    X(PCG_DEFER_PSI,           "MI_PCG_DEFER_PSI",           1,        CTX,           AB,        nullptr,               "psi += alpha pA rides in the next k_pcg_update_p: one vector read less per iteration") \
    X(PCG_FUSE_FINAL,          "MI_PCG_FUSE_FINAL",          0,        CTX,           AB,        nullptr,               "convergence test fused into the next update_p; measured: no gain (332.0 vs 332.3 us/iter), kept as an option") \
    X(PCG_FUSE_COOP,           "MI_PCG_FUSE_COOP",           0,        ONCE,          AB,        nullptr,               "1: the fused PCG launch goes through hipLaunchCooperativeKernel -- ~22 us per launch on this runtime (pcg_fused.inc)") \
    X(FUSE_PERM,               "MI_FUSE_PERM",               1,        CTX,           AB,        nullptr,               "caller-order operators gather / scatter through e2c inside the tile kernel") \
    X(DPCG_FUSED,              "MI_DPCG_FUSED",              1,        CALL,          AB,        nullptr,               "distributed PCG with the halo exchange and the sums inside its kernels (peer.inc)") \
    X(PBICG_HOST_STEPPED,      "MI_PBICG_HOST_STEPPED",      0,        CTX,           AB,        nullptr,               "1: PBiCG / PBiCGStab through their host-stepped loops instead of the device-resident ones") \
    X(TILE_FLAGS,              "MI_TILE_FLAGS",              1,        CTX,           AB,        nullptr,               "bit0: coefficient segments are staged with non-temporal loads (read once per launch): Amul -4 % (profiles/r02_b_cache_policy_ab.md); bit1: non-temporal loads of the row entries; bit2: non-temporal stores of the result y; bit3: non-temporal loads of the diagonal (Amul); same bits in every combination") \
    X(TILE_PERSIST,            "MI_TILE_PERSIST",            0,        CTX,           AB,        nullptr,               "persistent tile launches: workgroups = resident slots, each walks a run of tiles") \
    X(XCD_ROWS,                "MI_XCD_ROWS",                1,        CTX,           AB,        nullptr,               "XCD-aware block mapping of the caller-order row passes") \
    X(SMALL_TILES,             "MI_SMALL_TILES",             1,        ADDR,          AB,        nullptr,               "coarse GAMG levels are cut into enough tiles for every CU, down to 128 cells (engine.hip: addr_tile_params)") \
    X(AMUL_BS,                 "MI_AMUL_BS",                 0,        CTX,           AB,        nullptr,               "threads per workgroup of the tile kernels: 256, 512 or 1024; anything else = 0 = chosen per launch from the LDS footprint") \
    X(PCG_BATCH,               "MI_PCG_BATCH",               16,       CTX,           AB,        nullptr,               "iterations per batch of the device-resident solver loops; below 1 = 1") \
    X(PCG_GRAPH,               "MI_PCG_GRAPH",               -1,       CTX,           AB,        nullptr,               "batches of PCG iterations replay as a hipGraph: -1 up to 4 M cells, 0 never, 1 always") \
    \
    X(PEER_HALO,               "MI_PEER_HALO",               1,        ATTACH,        TRANSPORT, nullptr,               "halo windows between the ranks when the communicator runs in peer mode") \
    X(PEER_FINEGRAINED,        "MI_PEER_FINEGRAINED",        1,        ATTACH | HIER, TRANSPORT, nullptr,               "peer windows in fine-grained device memory; 0 = ordinary device memory (coherent only between processes that share one device); HIER: the gather window of the coarsest level") \
    X(PEER_GLOBALIZE,          "MI_PEER_GLOBALIZE",          1,        CALL,          TRANSPORT, nullptr,               "a matrix's all-reduces go through the peer windows (peer.inc: peer_reduce_ready)") \
    X(PEER_ALLOW_COARSE,       "MI_PEER_ALLOW_COARSE",       0,        ATTACH | HIER, TRANSPORT, nullptr,               "accept windows in ordinary device memory although a peer is on another device (not coherent while a kernel polls); HIER: the gather window of the coarsest level") \
    X(GAMG_GATHER_WIN,         "MI_GAMG_GATHER_WIN",         1,        HIER,          TRANSPORT, nullptr,               "the coarsest level of a decomposed case is gathered through a peer window") \
    X(PERSIST_LITMUS,          "MI_PERSIST_LITMUS",          1,        PERSIST,       TRANSPORT, nullptr,               "grid-barrier litmus before a context's first persistent launch") \
    X(PERSIST_GRID,            "MI_PERSIST_GRID",            0,        CTX,           TRANSPORT, nullptr,               "workgroups of the persistent kernel; 0: one per CU") \
    X(PERSIST_SHARED,          "MI_PERSIST_SHARED",          0,        CTX,           TRANSPORT, nullptr,               "1 lets ranks that share a device use the persistent kernel -- tests only: their grids (MI_PERSIST_GRID) must fit the device TOGETHER") \
    X(PERSIST_ZP,              "MI_PERSIST_ZP",              1,        CALL,          TRANSPORT, nullptr,               "tiles per workgroup up to which the persistent PCG kernel publishes z = rD o rA and the second pA buffer (persist.inc, ZP)") \
    X(EVENT_ATTACH,            "MI_EVENT_ATTACH",            1,        CTX,           TRANSPORT, nullptr,               "0: plain hipEventRecord pairs around the Amul launch instead of kernel-attached events") \
    \
    X(PERSIST_SKIP_ARRIVAL,    "MI_PERSIST_SKIP_ARRIVAL",    0,        CALL,          DIAG,      nullptr,               "fault injection, n > 0: the last workgroup of the persistent kernel never arrives at its n-th barrier") \
    X(PERSIST_BAR_POLLS,       "MI_PERSIST_BAR_POLLS",       4000000,  CALL,          DIAG,      nullptr,               "polls before a grid-barrier wait gives up (persist.inc: BAR_POLLS, a few seconds); the fault tests shorten it") \
    X(PCG_FUSE_POLLS,          "MI_PCG_FUSE_POLLS",          1000,     ONCE,          DIAG,      nullptr,               "polls before a workgroup of the fused PCG launch leaves its barrier (pcg_fused.inc: FUSED_WAIT_POLLS)") \
    X(PCG_FUSE_TEST,           nullptr,                      0,        CTX,           DIAG,      "pcg_fuse_test",       "option only: workgroups of the fused launch that leave its barrier at once (pcg_fused.inc)") \
    X(ROW_CAP,                 "MI_ROW_CAP",                 0,        ROWS,          DIAG,      nullptr,               "forced staging capacity of the assembly row passes: a small value sends blocks down the unstaged path") \
    X(ROW_BS,                  "MI_ROW_BS",                  1024,     ROWS,          DIAG,      nullptr,               "cells per block of the one- and two-array row passes when the numbering is not tile-contiguous: 256, 512 or 1024") \
    X(GRAD_BS,                 "MI_GRAD_BS",                 256,      ROWS,          DIAG,      nullptr,               "... of the four-array gradient pass") \
    X(FACE_GRID,               "MI_FACE_GRID",               8192,     CTX,           DIAG,      nullptr,               "the most workgroups (of 256 threads) a face pass or a unique-cell patch pass of assembly.inc is launched with (grid_for); below 1 = 1; a small value makes every such kernel walk its loop on a small mesh (tests)") \
    X(GAMG_ALWAYS_AGGLOMERATE, "MI_GAMG_ALWAYS_AGGLOMERATE", 0,        CTX,           DIAG,      nullptr,               "1: the level matrices are agglomerated again at every solve, also for unchanged coefficients") \
    X(MATCH_PARALLEL,          "MI_MATCH_PARALLEL",          0,        ADDR | HIER,   DIAG,      nullptr,               "1: large levels of the tile clustering (tiling.cpp) and of the pair agglomeration (gamg.cpp) are matched by the host threads; measured slower (profiles/r04_p_*)") \
    X(MATCH_LATER_ONLY,        "MI_MATCH_LATER_ONLY",        1,        HIER,          DIAG,      nullptr,               "the pair agglomeration looks only at faces to later cells (forward sweep over owned faces); 0 = every face of a cell") \
    X(DEBUG_MULTI,             "MI_DEBUG_MULTI",             0,        CALL,          DIAG,      nullptr,               "prints the multi-vector launches and their fall-backs to stderr") \
    X(DEBUG_PERSIST,           "MI_DEBUG_PERSIST",           0,        PERSIST,       DIAG,      nullptr,               "prints why persistent kernels were refused on a context to stderr")
// clang-format on

enum Switch : int {
#define X(id, env, dflt, when, group, option, meaning) SW_##id,
    MI_SWITCHES(X)
#undef X
    SW_COUNT
};

// the value of environment variable `name` as an int; `dflt` when it is unset or empty
inline int env_int(const char* name, int dflt)
{
    const char* v = name ? std::getenv(name) : nullptr;
    return (v && *v) ? std::atoi(v) : dflt;
}

namespace sw {
enum When : unsigned { ONCE = 1, CTX = 2, ADDR = 4, ROWS = 8, HIER = 16, ATTACH = 32, PERSIST = 64, CALL = 128 };
enum Group { USER, AB, TRANSPORT, DIAG };
struct Row { const char* env; int dflt; unsigned when; Group group; const char* option; };
constexpr Row table[SW_COUNT] = {
#define X(id, env, dflt, when, group, option, meaning) {env, dflt, when, group, option},
    MI_SWITCHES(X)
#undef X
};
inline int get(Switch s) { return env_int(table[s].env, table[s].dflt); }
inline const char* text(Switch s) { return table[s].env ? std::getenv(table[s].env) : nullptr; }   // the raw value, or nullptr: the two switches that are not read as an int
} // namespace sw
} // namespace mi
